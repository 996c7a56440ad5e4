"""True peak of renders on the device (msg_truepeak, DESIGN.md "True peak").

ITU-R BS.1770-4 Annex 2: the peak of the signal oversampled to at least 192 kHz, by
4 below 96 kHz, by 2 below 192 kHz and not at all from there on.  The interpolator is
a Nyquist filter with 12 zero crossings per side under a Kaiser window (beta = 7),
each phase normalised to unit DC gain; phase 0 is the identity, so the sample peak
covers it.  The device and ``msg_truepeak_host`` run it in float32 with one fixed
order of fused steps and agree to the bit; :func:`true_peak_reference` restates the
definition in float64 NumPy for the tests, and nothing on the product path uses it.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records

# csrc/truepeak.h: zero crossings per side, taps per phase, positions per tile workgroup
Z = 12
TAPS = 2 * Z
TILE = 2048
BETA = 7.0

# msg_truepeak_rec as a numpy record
TRUEPEAK_DTYPE = np.dtype([("true_peak", "<f8"), ("peak", "<f8"), ("dbtp", "<f8"), ("gain", "<f8"),
                           ("os", "<i4"), ("pad", "<i4")])


def oversampling(sr):
    """The oversampling factor at ``sr`` Hz: 4, 2 or 1."""
    sr = int(sr)
    if sr < 1:
        raise ValueError("the sample rate must be positive")
    return 4 if sr < 96000 else (2 if sr < 192000 else 1)


def taps(os):
    """The interpolator's phases 1 .. os - 1 in float64, shape (os - 1, 24), each of unit
    sum; phase p is the mirror image of phase os - p."""
    os = int(os)
    if os not in (1, 2, 4):
        raise ValueError("the oversampling factor is 1, 2 or 4")
    half = Z * os
    i = np.arange(0, half + 1)
    g = np.sinc(i / os) * np.kaiser(2 * half + 1, BETA)[half:]        # i >= 0; g is even
    out = np.zeros((os - 1, TAPS))
    for p in range(1, os // 2 + 1):
        t = g[np.abs(p + (np.arange(TAPS) - Z) * os)]
        t = t / t.sum()
        out[p - 1] = t
        out[os - p - 1] = t[::-1] if os - p != p else t
    return out


def true_peak_reference(x, sr):
    """The definition in float64 NumPy: the true peak (linear) of x, (n,) or
    (n, channels), with float64 taps and float64 sums.  NaN in, NaN out."""
    os = oversampling(sr)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n = x.shape[0]
    if n == 0:
        return 0.0
    if np.isnan(x).any():
        return math.nan
    tp = float(np.abs(x).max())
    for t in taps(os):
        for c in range(x.shape[1]):
            # y[m] = sum_q t[q] x[m + Z - q] is entry m + Z of the full convolution; m = -1 .. n - 1
            y = np.convolve(x[:, c], t)[Z - 1:Z + n]
            tp = max(tp, float(np.abs(y).max()))
    return tp


def _signal(x):
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
        raise ValueError("x must be (n,) or (n, 2)")
    return a, (1 if a.ndim == 1 else int(a.shape[1]))


def true_peak_host(x, sr):
    """msg_truepeak_host: the library's loop on the host (no device), the device's
    arithmetic to the bit; returns the record (a TRUEPEAK_DTYPE scalar)."""
    oversampling(sr)
    a, channels = _signal(x)
    rec = np.zeros(1, dtype=TRUEPEAK_DTYPE)
    L.check(L.lib().msg_truepeak_host(a.ctypes.data_as(C.c_void_p), channels, int(a.shape[0]), int(sr),
                                      rec.ctypes.data_as(C.c_void_p)), None)
    return rec[0]


def records(rec):
    """Device records (Engine.true_peak) as a TRUEPEAK_DTYPE array on the host; waits for them."""
    return read_records(rec, TRUEPEAK_DTYPE)


def true_peak(x, sr, device: int = 0, db: bool = False):
    """True peak of x, (n,) mono or (n, 2) stereo, at ``sr`` Hz, measured on the device:
    linear, or in dBTP with ``db``.  NumPy in, a float out; a device tensor in, a
    one-element device tensor out, enqueued on the current stream (no host synchronise)."""
    from .engine import default_engine

    oversampling(sr)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x)
    rec = eng.true_peak(t, [0], [int(t.shape[0])], channels, int(sr))
    col = 2 if db else 0
    if not on_host:
        return rec[0, col:col + 1]
    return float(records(rec)["dbtp" if db else "true_peak"][0])
