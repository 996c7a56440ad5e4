"""A compressor on the device (msg_dynamics, DESIGN.md "4l. Dynamics").

Per frame: the level p, the largest |x| over the channels (the channels are linked: one gain
serves both); the gain-reduction demand d in dB from the soft-knee curve of Giannoulis,
Massberg and Reiss (JAES 2012), as an integer in units of 2^-32 dB; its maximum over the hold;
a release that lets the reduction fall along a straight line in dB, forward, and an attack that
raises it along a straight line ahead of every peak, backward (the pass is offline: the gain has
fully arrived at a peak); the envelope E is the larger of the two, and the gain is
``10^((makeup_db - E) / 20)``.  The ballistics are integer max-plus recurrences, so the device's
tiled scans and ``msg_dynamics_host``'s sequential loop agree to the bit, alone or in any batch;
:func:`dynamics_reference` restates the definition in float64 NumPy with libm for the tests,
and nothing on the product path uses it.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records
from .edges import frames

# csrc/dynamics.h
TILE = 4096              # frames per workgroup
HOLD_MAX = 4096          # frames
UNIT = 2.0 ** 32         # envelope units per dB
E_MAX = 1 << 40          # the largest envelope value and step: 256 dB

# msg_dynamics_rec as a numpy record
DYNAMICS_DTYPE = np.dtype([("max_e", "<i8"), ("sum_e16", "<i8"), ("reduced_frames", "<i8"), ("state", "<i4"),
                           ("hold_frames", "<i4")])
# records(): the record and the dB columns that follow from it
DYNAMICS_ROW_DTYPE = np.dtype(DYNAMICS_DTYPE.descr + [("max_reduction_db", "<f8"), ("mean_reduction_db", "<f8")])

_FIELDS = ("threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "hold_ms", "makeup_db")


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def step(ms, sr):
    """Envelope units per frame of a ramp that moves 10 dB in ``ms`` milliseconds at ``sr`` Hz:
    round(10 2^32 / (sr ms / 1000)) within 1 .. 2^40; 0 ms is 2^40, instant."""
    span = float(sr) * float(ms) / 1000.0
    if not span > 0.0:
        return E_MAX
    return int(min(max(math.floor(10.0 * UNIT / span + 0.5), 1.0), float(E_MAX)))


@dataclass
class Dynamics:
    threshold_db: object = -18.0  # dBFS above which the level is reduced, -150 .. 24
    ratio: object = 3.0           # >= 1; math.inf pins the level at the threshold
    knee_db: object = 6.0         # width of the soft knee around the threshold, 0 .. 48
    attack_ms: object = 5.0       # the time the gain takes to come down 10 dB ahead of a peak
    release_ms: object = 150.0    # the time it takes to recover 10 dB
    hold_ms: object = 0.0         # the reduction is held this long before it recovers
    makeup_db: object = 0.0       # -48 .. 48, applied to every frame

    def check(self, rate=None):
        """ValueError, naming the field, for a value out of range; with ``rate`` also for a hold
        beyond 4096 frames at that rate.  Returns self."""
        for k in _FIELDS:
            v = getattr(self, k)
            if not _number(v) or math.isnan(float(v)):
                raise ValueError(f"{k} must be a number")
        if not math.isfinite(float(self.threshold_db)) or not -150.0 <= float(self.threshold_db) <= 24.0:
            raise ValueError("threshold_db must be a finite number of dB from -150 to 24")
        if not float(self.ratio) >= 1.0:
            raise ValueError("ratio must be at least 1 (math.inf: the level is pinned at the threshold)")
        if not math.isfinite(float(self.knee_db)) or not 0.0 <= float(self.knee_db) <= 48.0:
            raise ValueError("knee_db must be a finite number of dB from 0 to 48")
        for k in ("attack_ms", "release_ms", "hold_ms"):
            if not math.isfinite(float(getattr(self, k))) or float(getattr(self, k)) < 0.0:
                raise ValueError(f"{k} must be a finite number of milliseconds from 0 up")
        if not math.isfinite(float(self.makeup_db)) or abs(float(self.makeup_db)) > 48.0:
            raise ValueError("makeup_db must be a finite number of dB from -48 to 48")
        if rate is not None:
            if int(rate) < 1:
                raise ValueError("the sample rate must be positive")
            if frames(self.hold_ms, rate) > HOLD_MAX:
                raise ValueError(f"hold_ms is more than {HOLD_MAX} frames at {int(rate)} Hz")
        return self

    def opts(self, rate):
        """The msg_dynamics_opts of this compressor at ``rate`` Hz: the milliseconds as steps and frames."""
        self.check(rate)
        return L.MsgDynamicsOpts(float(self.threshold_db), float(self.ratio), float(self.knee_db), float(self.makeup_db),
                                 step(self.attack_ms, rate), step(self.release_ms, rate), frames(self.hold_ms, rate), 0)


def p0(threshold_db, knee_db):
    """The float32 at or just under the linear level of threshold_db - knee_db / 2: no frame at
    or under it asks for a reduction."""
    lin = 10.0 ** ((float(threshold_db) - 0.5 * float(knee_db)) / 20.0)
    p = np.float32(lin)
    if float(p) > lin:
        p = np.nextafter(p, np.float32(0))
    return p


def curve_reference(level_db, threshold_db, ratio, knee_db):
    """The static curve: the reduction in dB at a level in dBFS, float64 NumPy."""
    over = np.asarray(level_db, dtype=np.float64) - float(threshold_db)
    s = 1.0 - 1.0 / float(ratio)
    w = float(knee_db)
    with np.errstate(divide="ignore", invalid="ignore"):
        knee = s * (over + 0.5 * w) ** 2 / (2.0 * w) if w > 0.0 else np.zeros_like(over)
    return np.where(2.0 * over > w, s * over, np.where((2.0 * over < -w) | (w <= 0.0), 0.0, knee))


def _maxplus(d, step_, reverse=False):
    """y[f] = max(y[f - 1] - step, d[f]) from 0 (``reverse``: from the last frame), in Python ints."""
    out = np.zeros(len(d), dtype=np.int64)
    y = 0
    order = range(len(d) - 1, -1, -1) if reverse else range(len(d))
    for f in order:
        y = max(y - step_, int(d[f]), 0)
        out[f] = y
    return out


def dynamics_reference(x, sr, dyn):
    """The definition restated in float64 NumPy with libm: returns (y, E), the compressed signal
    (x's shape, float64) and the envelope per frame (int64, units of 2^-32 dB).  A NaN or an
    infinity in x: (x, E of the finite frames' demands)."""
    o = dyn.opts(sr)
    xin = np.asarray(x, dtype=np.float64)
    v = xin.reshape(len(xin), -1)
    n = v.shape[0]
    if n == 0:
        return xin.copy(), np.zeros(0, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        p = np.fmax.reduce(np.abs(v), axis=1)
    finite = np.isfinite(v).all(axis=1)
    lvl = np.where(finite & (p > float(p0(o.threshold_db, o.knee_db))), p, 1.0)
    red = curve_reference(20.0 * np.log10(lvl), o.threshold_db, o.ratio, o.knee_db)
    red = np.where(finite & (p > float(p0(o.threshold_db, o.knee_db))), red, 0.0)
    d = np.clip(np.floor(red * UNIT + 0.5), 0.0, float(E_MAX)).astype(np.int64)
    h = int(o.hold_frames)
    dh = d.copy()
    have = 1                                               # dh[f] = max of d[f - have + 1 .. f]
    while have < h + 1:
        s = min(have, h + 1 - have)
        if s < n:
            dh[s:] = np.maximum(dh[s:], dh[:-s])
        have += s
    e = np.maximum(_maxplus(dh, int(o.release_step)), _maxplus(d, int(o.attack_step), reverse=True))
    if not finite.all():
        return xin.copy(), e
    g = 10.0 ** ((o.makeup_db - e.astype(np.float64) / UNIT) / 20.0)
    return xin * (g[:, None] if xin.ndim == 2 else g), e


def _signal(x):
    a = np.array(x, dtype=np.float32, order="C")
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
        raise ValueError("x must be (n,) or (n, 2)")
    return a, 1 if a.ndim == 1 else int(a.shape[1])


def host(y, channels, opts, env=False):
    """msg_dynamics_host over y in place with the msg_dynamics_opts given; returns (y, rec), or,
    ``env``, (y, rec, E) through the library's test entry point."""
    rec = np.zeros(1, dtype=DYNAMICS_DTYPE)
    n = int(y.shape[0])
    yp, rp = y.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)
    if not env:
        L.check(L.lib().msg_dynamics_host(yp, channels, n, C.byref(opts), rp), None)
        return y, rec[0]
    fn = L.lib().msg_debug_dynamics_env
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(L.MsgDynamicsOpts), C.c_void_p, C.c_void_p]
    e = np.zeros(n, dtype=np.int64)
    L.check(fn(yp, channels, n, C.byref(opts), rp, e.ctypes.data_as(C.c_void_p)), None)
    return y, rec[0], e


def dynamics_host(x, sr, dyn, env=False):
    """msg_dynamics_host: the library's loop on the host (no device), the device's arithmetic to
    the bit.  Returns (y, rec): a compressed float32 copy of x and the record (a DYNAMICS_DTYPE
    scalar); ``env``: (y, rec, E) with the envelope per frame."""
    a, channels = _signal(x)
    return host(a.copy(), channels, dyn.opts(sr), env)


def derive(rec):
    """A DYNAMICS_DTYPE array with the dB columns: ``max_reduction_db = max_e 2^-32`` and
    ``mean_reduction_db = sum_e16 2^-16 / reduced_frames``, the mean over the frames that were
    reduced (0 without one)."""
    rec = np.asarray(rec, dtype=DYNAMICS_DTYPE)
    out = np.zeros(rec.shape, dtype=DYNAMICS_ROW_DTYPE)
    for k in DYNAMICS_DTYPE.names:
        out[k] = rec[k]
    out["max_reduction_db"] = rec["max_e"] / UNIT
    out["mean_reduction_db"] = rec["sum_e16"] / 65536.0 / np.maximum(rec["reduced_frames"], 1)
    return out


def records(rec):
    """Device records (Engine.dynamics) as a DYNAMICS_ROW_DTYPE array on the host, the dB columns
    added; waits for them."""
    return derive(read_records(rec, DYNAMICS_DTYPE))


def dynamics(x, sr, dyn, device: int = 0):
    """Compress x, (n,) mono or (n, 2) stereo at ``sr`` Hz, with ``dyn`` on the device.  NumPy in:
    (a compressed float32 copy, its record).  A device tensor in: compressed in place, enqueued
    on the current stream (no host synchronise); returns the device record tensor
    (dynamics.records reads it)."""
    from .engine import default_engine

    dyn.check(sr)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x, in_place=True)
    rec = eng.dynamics(t, [0], [int(t.shape[0])], channels, int(sr), dyn)
    if not on_host:
        return rec
    return t.cpu().numpy(), records(rec)[0]
