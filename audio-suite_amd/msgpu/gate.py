"""A gate (downward expander) on the device (msg_gate_apply, DESIGN.md "4m. Gate").

Per frame: the level p, the largest |x| over the channels (the channels are linked); the state,
open at or above the threshold, closed under threshold - hysteresis and the state of the frame
before in between; a hold that keeps the state open for ``hold_ms`` after its last open frame; the
openness o, RANGE where the held state is open and RANGE less the expander's reduction
``(ratio - 1) (threshold - level)`` elsewhere, as an integer in units of 2^-32 dB; a closing ramp
that lets the openness fall along a straight line in dB, forward, and an opening ramp that raises
it along a straight line ahead of every opening, backward (the pass is offline: the gate is fully
open where the state opens); the envelope E is RANGE less the larger of the two and the gain is
``10^(-E / 20)``, zero where ``range_db`` is infinite and the gate is shut.  State, hold and ramps
compose exactly over integers, so the device's tiled scans and ``msg_gate_host``'s sequential loop
agree to the bit, alone or in any batch; :func:`gate_reference` restates the definition in float64
NumPy with libm for the tests, and nothing on the product path uses it.

The C entry point is ``msg_gate_apply`` and the engine's method ``Engine.gate_apply``: ``msg_gate``
and ``Engine.gate`` are the stream gate between two contexts.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records
from .dynamics import E_MAX, UNIT, _maxplus, _number, _signal, step
from .edges import frames

# msg_gate_rec as a numpy record
GATE_DTYPE = np.dtype([("max_e", "<i8"), ("sum_e16", "<i8"), ("reduced_frames", "<i8"), ("open_frames", "<i8"),
                       ("opens", "<i8"), ("state", "<i4"), ("hold_frames", "<i4")])
# records(): the record and the dB columns that follow from it
GATE_ROW_DTYPE = np.dtype(GATE_DTYPE.descr + [("max_reduction_db", "<f8"), ("mean_reduction_db", "<f8")])

_FIELDS = ("threshold_db", "hysteresis_db", "ratio", "range_db", "attack_ms", "release_ms", "hold_ms")


@dataclass
class Gate:
    threshold_db: object = -50.0   # dBFS at or above which the gate opens, -150 .. 24
    hysteresis_db: object = 6.0    # it closes this far under the threshold, 0 .. 48
    ratio: object = math.inf       # >= 1; finite: an expander's slope under the threshold
    range_db: object = 60.0        # the most the gate takes away, (0, 240] or math.inf: silence
    attack_ms: object = 0.5        # the time the gain takes to rise 10 dB ahead of an opening
    release_ms: object = 50.0      # the time it takes to fall 10 dB
    hold_ms: object = 10.0         # the state is held open this long after its last open frame

    def check(self, rate=None):
        """ValueError, naming the field, for a value out of range.  Returns self."""
        for k in _FIELDS:
            v = getattr(self, k)
            if not _number(v) or math.isnan(float(v)):
                raise ValueError(f"{k} must be a number")
        if not math.isfinite(float(self.threshold_db)) or not -150.0 <= float(self.threshold_db) <= 24.0:
            raise ValueError("threshold_db must be a finite number of dB from -150 to 24")
        if not math.isfinite(float(self.hysteresis_db)) or not 0.0 <= float(self.hysteresis_db) <= 48.0:
            raise ValueError("hysteresis_db must be a finite number of dB from 0 to 48")
        if not float(self.ratio) >= 1.0:
            raise ValueError("ratio must be at least 1 (math.inf: a gate)")
        if not float(self.range_db) > 0.0 or (float(self.range_db) > 240.0 and not math.isinf(float(self.range_db))):
            raise ValueError("range_db must be a number of dB above 0 up to 240, or math.inf")
        for k in ("attack_ms", "release_ms", "hold_ms"):
            if not math.isfinite(float(getattr(self, k))) or float(getattr(self, k)) < 0.0:
                raise ValueError(f"{k} must be a finite number of milliseconds from 0 up")
        if rate is not None:
            if int(rate) < 1:
                raise ValueError("the sample rate must be positive")
            if frames(self.hold_ms, rate) >= 2 ** 31:
                raise ValueError(f"hold_ms is more than 2^31 - 1 frames at {int(rate)} Hz")
        return self

    def opts(self, rate):
        """The msg_gate_opts of this gate at ``rate`` Hz: the milliseconds as steps and frames."""
        self.check(rate)
        return L.MsgGateOpts(float(self.threshold_db), float(self.hysteresis_db), float(self.ratio), float(self.range_db),
                             step(self.attack_ms, rate), step(self.release_ms, rate), frames(self.hold_ms, rate), 0)


def level_up(db):
    """The smallest float32 at or above the linear level of ``db`` dB: p_open, and p_close."""
    lin = 10.0 ** (float(db) / 20.0)
    p = np.float32(lin)
    if float(p) < lin:
        p = np.nextafter(p, np.float32(np.inf))
    return p


def range_units(range_db):
    return E_MAX if math.isinf(float(range_db)) else int(math.floor(float(range_db) * UNIT + 0.5))


def gate_reference(x, sr, gate):
    """The definition restated in float64 NumPy with libm: returns (y, E, sh), the gated signal
    (x's shape, float64), the envelope per frame (int64, units of 2^-32 dB) and the held state per
    frame (bool).  A NaN or an infinity in x: (x, E, sh) of the levels as they compare."""
    o = gate.opts(sr)
    xin = np.asarray(x, dtype=np.float64)
    v = xin.reshape(len(xin), -1)
    n = v.shape[0]
    if n == 0:
        return xin.copy(), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    with np.errstate(invalid="ignore"):
        p = np.fmax.reduce(np.abs(v), axis=1)
    finite = np.isfinite(v).all(axis=1)
    p = np.where(finite, p, np.inf)
    is_open = p >= float(level_up(o.threshold_db))
    is_closed = p < float(level_up(o.threshold_db - o.hysteresis_db))
    # the state: the last decided frame's; the hold: the frames since the last open state
    idx = np.arange(n)
    last = np.maximum.accumulate(np.where(is_open | is_closed, idx, -1))
    s = np.where(last >= 0, is_open[np.maximum(last, 0)], False)
    since = idx - np.maximum.accumulate(np.where(s, idx, -(1 << 40)))
    sh = since <= int(o.hold_frames)
    rng = range_units(o.range_db)
    if math.isinf(o.ratio):
        r = np.full(n, rng, dtype=np.int64)
    else:
        with np.errstate(divide="ignore"):
            under = o.threshold_db - 20.0 * np.log10(np.where(finite & (p > 0), p, 1.0))
        val = np.floor((o.ratio - 1.0) * under * UNIT + 0.5)
        r = np.where(p > 0, np.clip(val, 0.0, float(rng)), float(rng)).astype(np.int64)
    op = np.where(sh, rng, rng - r).astype(np.int64)
    e = rng - np.maximum(_maxplus(op, int(o.release_step)), _maxplus(op, int(o.attack_step), reverse=True))
    if not finite.all():
        return xin.copy(), e, sh
    g = np.where(e >= E_MAX, 0.0, 10.0 ** (-e.astype(np.float64) / UNIT / 20.0))
    return xin * (g[:, None] if xin.ndim == 2 else g), e, sh


def host(y, channels, opts, env=False):
    """msg_gate_host over y in place with the msg_gate_opts given; returns (y, rec), or, ``env``,
    (y, rec, E, sh) through the library's test entry point."""
    rec = np.zeros(1, dtype=GATE_DTYPE)
    n = int(y.shape[0])
    yp, rp = y.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)
    if not env:
        L.check(L.lib().msg_gate_host(yp, channels, n, C.byref(opts), rp), None)
        return y, rec[0]
    fn = L.lib().msg_debug_gate_env
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(L.MsgGateOpts), C.c_void_p, C.c_void_p, C.c_void_p]
    e = np.zeros(n, dtype=np.int64)
    sh = np.zeros(n, dtype=np.uint8)
    L.check(fn(yp, channels, n, C.byref(opts), rp, e.ctypes.data_as(C.c_void_p), sh.ctypes.data_as(C.c_void_p)), None)
    return y, rec[0], e, sh.astype(bool)


def gate_host(x, sr, gate, env=False):
    """msg_gate_host: the library's loop on the host (no device), the device's arithmetic to the
    bit.  Returns (y, rec): a gated float32 copy of x and the record (a GATE_DTYPE scalar);
    ``env``: (y, rec, E, sh) with the envelope and the held state per frame."""
    a, channels = _signal(x)
    return host(a.copy(), channels, gate.opts(sr), env)


def derive(rec):
    """A GATE_DTYPE array with the dB columns: ``max_reduction_db = max_e 2^-32`` and
    ``mean_reduction_db = sum_e16 2^-16 / reduced_frames``, the mean over the frames that were
    reduced (0 without one)."""
    rec = np.asarray(rec, dtype=GATE_DTYPE)
    out = np.zeros(rec.shape, dtype=GATE_ROW_DTYPE)
    for k in GATE_DTYPE.names:
        out[k] = rec[k]
    out["max_reduction_db"] = rec["max_e"] / UNIT
    out["mean_reduction_db"] = rec["sum_e16"] / 65536.0 / np.maximum(rec["reduced_frames"], 1)
    return out


def records(rec):
    """Device records (Engine.gate_apply) as a GATE_ROW_DTYPE array on the host, the dB columns
    added; waits for them."""
    return derive(read_records(rec, GATE_DTYPE))


def gate(x, sr, gate, device: int = 0):
    """Gate x, (n,) mono or (n, 2) stereo at ``sr`` Hz, with ``gate`` on the device.  NumPy in:
    (a gated float32 copy, its record).  A device tensor in: gated in place, enqueued on the
    current stream (no host synchronise); returns the device record tensor (gate.records reads it)."""
    from .engine import default_engine

    gate.check(sr)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x, in_place=True)
    rec = eng.gate_apply(t, [0], [int(t.shape[0])], channels, int(sr), gate)
    if not on_host:
        return rec
    return t.cpu().numpy(), records(rec)[0]
