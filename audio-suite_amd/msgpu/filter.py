"""The delivery filter on the device (msg_filter, DESIGN.md "4j. Filter"): a rumble high-pass,
a low-pass, two shelves and peaking bands, or a caller's own biquad cascade, run over signals
where they lie in HBM.

A ``Filter`` says what is wanted in Hz, dB and Q; ``Filter.design(sr)`` turns it into the
(S, 6) float64 cascade in scipy's ``sos`` layout that the library takes, at most 8 sections.
High- and low-passes are Butterworth designs by the bilinear transform with pre-warping
(K = tan(pi f / sr)); shelves and peaks are the Audio EQ Cookbook's in their Q form.  The
formulas are evaluated in extended precision and rounded once to float64: at 20 Hz and
384 kHz a float64 evaluation already loses five digits of the poles' distance from z = 1.

The recurrence is csrc/filter.h's: transposed direct form II in float64 on float32 samples,
the cascade's output rounded once to float32, in place.  ``zero_phase`` is, by definition, the
forward call followed by the reverse call with the same cascade: no phase shift, twice every
band's gain in dB, and a symmetric click stays symmetric.  :func:`filter_reference` restates
the definition with ``scipy.signal.sosfilt`` for the tests; nothing on the product path uses it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._signal import device_signal

# csrc/filter.h
MAX_SECTIONS = 8
REVERSE = 1
TILE = 4096              # frames per workgroup
MAX_ORDER = 8
Q_MAX = 100.0            # a band narrower than f / 100 is a resonator, not an equaliser
GAIN_MAX_DB = 60.0

_R = np.longdouble       # the designs' arithmetic: x87 extended where the platform has it


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(float(v))


def _cut(v, what):
    """``f`` or ``(f, order)`` of a high- or low-pass as (f, order)."""
    if _number(v):
        v = (v, 2)
    if not isinstance(v, (tuple, list)) or len(v) != 2 or not _number(v[0]) or isinstance(v[1], bool) or \
            not isinstance(v[1], (int, np.integer)):
        raise ValueError(f"{what} must be a frequency in Hz or (frequency, order)")
    f, order = float(v[0]), int(v[1])
    if not 1 <= order <= MAX_ORDER:
        raise ValueError(f"the order of {what} must be 1 to {MAX_ORDER}")
    if not f > 0.0:
        raise ValueError(f"the frequency of {what} must lie in (0, sr / 2)")
    return f, order


def _band(v, what):
    """``(f, gain_db, q)`` of a shelf or a peak."""
    if not isinstance(v, (tuple, list)) or len(v) != 3 or not all(_number(a) for a in v):
        raise ValueError(f"{what} must be (frequency, gain_db, q)")
    f, gain, q = (float(a) for a in v)
    if not f > 0.0:
        raise ValueError(f"the frequency of {what} must lie in (0, sr / 2)")
    if not 0.0 < q <= Q_MAX:
        raise ValueError(f"the Q of {what} must lie in (0, {Q_MAX:g}]")
    if abs(gain) > GAIN_MAX_DB:
        raise ValueError(f"the gain of {what} must lie within {GAIN_MAX_DB:g} dB of 0")
    return f, gain, q


def _pi():
    return 4 * np.arctan(_R(1))


def butterworth(kind, f, order, sr):
    """The sections of an ``order``-pole Butterworth "highpass" or "lowpass" at ``f`` Hz, bilinear
    transform with pre-warping, in extended precision: conjugate pole pairs k = 0 .. order // 2 - 1
    with 1 / Q = 2 sin(pi (2 k + 1) / (2 order)), then the real pole of an odd order as one
    first-order section (b2 = a2 = 0)."""
    K = np.tan(_pi() * _R(f) / _R(sr))
    rows = []
    for k in range(order // 2):
        iq = 2 * np.sin(_pi() * (2 * k + 1) / (2 * _R(order)))
        d = 1 + K * iq + K * K
        b = (K * K / d, 2 * K * K / d, K * K / d) if kind == "lowpass" else (1 / d, -2 / d, 1 / d)
        rows.append((*b, _R(1), 2 * (K * K - 1) / d, (1 - K * iq + K * K) / d))
    if order % 2:
        d = 1 + K
        b = (K / d, K / d, _R(0)) if kind == "lowpass" else (1 / d, -1 / d, _R(0))
        rows.append((*b, _R(1), (K - 1) / d, _R(0)))
    return rows


def cookbook(kind, f, gain_db, q, sr):
    """One Audio EQ Cookbook section in its Q form, "peak", "low_shelf" or "high_shelf", normalised
    to a0 = 1, in extended precision: A = 10^(gain_db / 40), w0 = 2 pi f / sr, alpha = sin w0 / (2 Q)."""
    A = _R(10) ** (_R(gain_db) / 40)
    w0 = 2 * _pi() * _R(f) / _R(sr)
    cs, alpha = np.cos(w0), np.sin(w0) / (2 * _R(q))
    if kind == "peak":
        b = (1 + alpha * A, -2 * cs, 1 - alpha * A)
        a = (1 + alpha / A, -2 * cs, 1 - alpha / A)
    else:
        r = 2 * np.sqrt(A) * alpha
        sg = 1 if kind == "low_shelf" else -1            # the high shelf mirrors the low one: cos -> -cos
        c = sg * cs
        b = (A * ((A + 1) - (A - 1) * c + r), sg * 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - r))
        a = ((A + 1) + (A - 1) * c + r, sg * -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - r)
    return (b[0] / a[0], b[1] / a[0], b[2] / a[0], _R(1), a[1] / a[0], a[2] / a[0])


@dataclass
class Filter:
    highpass: object = None       # f or (f, order), order 1 .. 8 (default 2): Butterworth
    lowpass: object = None        # the same
    low_shelf: object = None      # (f, gain_db, q)
    high_shelf: object = None     # (f, gain_db, q)
    peaks: object = ()            # [(f, gain_db, q), ...]
    sos: object = None            # a raw (S, 6) cascade, b0 b1 b2 a0 a1 a2 with a0 == 1, run last
    zero_phase: bool = False      # forward, then reverse with the same cascade

    def _parts(self):
        """(kind, values) of every design asked for, in cascade order; ValueError for a value out of
        range.  The order: high-pass, low shelf, peaks, high shelf, low-pass, then ``sos``."""
        parts = []
        if self.highpass is not None:
            parts.append(("highpass", _cut(self.highpass, "highpass")))
        if self.low_shelf is not None:
            parts.append(("low_shelf", _band(self.low_shelf, "low_shelf")))
        if not isinstance(self.peaks, (tuple, list)):
            raise ValueError("peaks must be a list of (frequency, gain_db, q)")
        for i, pk in enumerate(self.peaks):
            parts.append(("peak", _band(pk, f"peaks[{i}]")))
        if self.high_shelf is not None:
            parts.append(("high_shelf", _band(self.high_shelf, "high_shelf")))
        if self.lowpass is not None:
            parts.append(("lowpass", _cut(self.lowpass, "lowpass")))
        return parts

    def _raw(self):
        if self.sos is None:
            return np.zeros((0, 6), dtype=np.float64)
        s = np.array(self.sos, dtype=np.float64)
        if s.ndim != 2 or s.shape[1] != 6 or s.shape[0] < 1:
            raise ValueError("sos must be an (S, 6) array of sections b0 b1 b2 a0 a1 a2")
        if not np.all(np.isfinite(s)):
            raise ValueError("the coefficients of sos must be finite")
        if np.any(s[:, 3] != 1.0):
            raise ValueError("every section of sos must have a0 == 1")
        if np.any(~(np.abs(s[:, 5]) < 1.0)) or np.any(~(np.abs(s[:, 4]) < 1.0 + s[:, 5])):
            raise ValueError("every section of sos must lie inside the stability triangle |a2| < 1, |a1| < 1 + a2")
        return s

    def n_sections(self):
        return sum((v[1] + 1) // 2 if kind in ("highpass", "lowpass") else 1 for kind, v in self._parts()) + len(self._raw())

    def check(self, sr=None):
        """ValueError for a value out of range, an empty filter or more than 8 sections; with ``sr``
        also for a frequency outside (0, sr / 2).  Returns self."""
        if not isinstance(self.zero_phase, (bool, np.bool_)):
            raise ValueError("zero_phase must be True or False")
        n = self.n_sections()
        if n < 1:
            raise ValueError("the filter is empty: give a high-pass, a low-pass, a shelf, a peak or sos")
        if n > MAX_SECTIONS:
            raise ValueError(f"the filter has {n} sections, more than {MAX_SECTIONS}")
        if sr is not None:
            sr = int(sr)
            if sr < 1:
                raise ValueError("the sample rate must be positive")
            for kind, v in self._parts():
                if not 0.0 < v[0] < sr / 2.0:
                    raise ValueError(f"the frequency of {kind} must lie in (0, sr / 2): {v[0]:g} Hz at {sr} Hz")
        return self

    def design(self, sr):
        """The (S, 6) float64 cascade at ``sr`` Hz in scipy's sos layout (a0 == 1)."""
        self.check(sr)
        rows = []
        for kind, v in self._parts():
            rows += butterworth(kind, v[0], v[1], sr) if kind in ("highpass", "lowpass") else [cookbook(kind, *v, sr)]
        designed = np.array([[float(c) for c in row] for row in rows], dtype=np.float64).reshape(len(rows), 6)
        return np.concatenate([designed, self._raw()], axis=0)

    def opts(self, sr, reverse=False):
        """The msg_filter_opts of this filter at ``sr`` Hz, one direction."""
        return _opts(self.design(sr), reverse)

    def passes(self):
        """The directions of the calls this filter makes, in order (False forward, True reverse)."""
        return (False, True) if self.zero_phase else (False,)


def _opts(sos, reverse):
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    o = L.MsgFilterOpts()
    o.n_sections, o.flags = int(sos.shape[0]), REVERSE if reverse else 0
    for k in range(min(int(sos.shape[0]), MAX_SECTIONS)):
        for i in range(6):
            o.sos[k][i] = float(sos[k, i])
    return o


def _signal(x):
    a = np.array(x, dtype=np.float32, order="C")
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
        raise ValueError("x must be (n,) or (n, 2)")
    return a, 1 if a.ndim == 1 else int(a.shape[1])


def sos_host(x, sos, reverse=False):
    """msg_filter_host with a raw cascade, one direction: a filtered float32 copy of x."""
    a, channels = _signal(x)
    o = _opts(sos, reverse)
    L.check(L.lib().msg_filter_host(a.ctypes.data_as(C.c_void_p), channels, int(a.shape[0]), C.byref(o)), None)
    return a


def filter_host(x, sr, flt, reverse=False):
    """msg_filter_host: the library's sequential loop on the host (no device).  Returns a filtered
    float32 copy of x; ``reverse``: a one-direction filter runs from the last frame to the first."""
    sos = flt.design(sr)
    a, _ = _signal(x)
    for rev in ((False, True) if flt.zero_phase else (bool(reverse),)):
        a = sos_host(a, sos, rev)
    return a


def sos_reference(x, sos, reverse=False):
    """The definition with scipy.signal.sosfilt in float64 on the float32 input, not rounded: (n,) or (n, 2)."""
    from scipy.signal import sosfilt
    a, _ = _signal(x)
    v = a.astype(np.float64)
    if not len(v):
        return v
    if reverse:
        return sosfilt(sos, v[::-1], axis=0)[::-1].copy()
    return sosfilt(sos, v, axis=0)


def filter_reference(x, sr, flt, reverse=False):
    """The definition in float64 NumPy / scipy, rounded once per call to float32 as the library does."""
    sos = flt.design(sr)
    a, _ = _signal(x)
    for rev in ((False, True) if flt.zero_phase else (bool(reverse),)):
        a = sos_reference(a, sos, rev).astype(np.float32)
    return a


def filter(x, sr, flt, device: int = 0, reverse=False):
    """Filter x, (n,) mono or (n, 2) stereo at ``sr`` Hz, on the device with a ``Filter``.  NumPy in:
    a filtered float32 copy out.  A device tensor in: filtered in place where it lies, enqueued on
    the current stream (no host synchronise), and returned."""
    from .engine import default_engine

    flt.check(sr)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x, in_place=True)
    eng.filter(t, [0], [int(t.shape[0])], channels, int(sr), flt, reverse=reverse)
    return t.cpu().numpy() if on_host else t
