"""Look-ahead true-peak limiter on the device (msg_limit, DESIGN.md "4f. Limiter").

Per frame: the envelope e, the larger of the sample and of the oversampled values on both
sides of it (truepeak.py's interpolator) over the channels; the demand r = min(1, c / e);
its minimum over +-(L + Z) frames; that smoothed by a Hann window of 2 L + 1 unit-sum
weights; the gain g is the smaller of the result and r, 1 (and the frame not written) where
no over-ceiling frame lies within 2 L + Z frames.  The device and ``msg_limit_host`` run it in
float32 in one fixed order and agree to the bit; :func:`limit_reference` restates the
definition in float64 NumPy for the tests, and nothing on the product path uses it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records
from .truepeak import Z, _signal, oversampling, taps

# csrc/limit.h
L_MAX = 4096
ENV_TILE = 2048

# msg_limit_rec as a numpy record
LIMIT_DTYPE = np.dtype([("min_gain", "<f8"), ("reduction_db", "<f8"), ("limited_frames", "<i8"),
                        ("lookahead", "<i4"), ("state", "<i4")])


def tile(lookahead):
    """Frames per workgroup of the apply kernel at a look-ahead of ``lookahead`` frames."""
    la = int(lookahead)
    return 2048 if la <= 256 else (4096 if la <= 512 else (8192 if la <= 1024 else 16384))


def lookahead_frames(sr, ms):
    """The look-ahead of ``ms`` milliseconds in frames at ``sr`` Hz, at least one."""
    return max(1, int(round(float(sr) * float(ms) / 1000.0)))


def _ceiling(ceiling_dbtp):
    v = float(ceiling_dbtp)
    if not np.isfinite(v):
        raise ValueError("the true-peak ceiling must be a number of dBTP")
    return 10.0 ** (v / 20.0)


def weights(lookahead):
    """The smoothing window in float64: 2 L + 1 Hann weights of unit sum."""
    la = int(lookahead)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(2 * la + 1) + 1.0) / (2 * la + 2))
    return w / w.sum()


def envelope_reference(x, sr):
    """e of the definition in float64: per frame the largest of |x| and of the oversampled
    values on both sides, over the channels."""
    os = oversampling(sr)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n = x.shape[0]
    if n == 0:
        return np.zeros(0)
    e = np.abs(x).max(axis=1)
    for t in taps(os):
        for c in range(x.shape[1]):
            y = np.abs(np.convolve(x[:, c], t)[Z - 1:Z + n])     # y[i] = |y_p[i - 1]|, i = 0 .. n
            e = np.maximum(e, np.maximum(y[:-1], y[1:]))
    return e


def limit_reference(x, sr, c, lookahead):
    """The definition in float64 NumPy with float64 taps and weights: returns (y, g), the
    limited signal (x's shape, float64) and the gain per frame.  A NaN in x: (x, ones)."""
    la = int(lookahead)
    xin = np.asarray(x, dtype=np.float64)
    n = xin.shape[0]
    if n == 0 or np.isnan(xin).any():
        return xin.copy(), np.ones(n)
    e = envelope_reference(xin, sr)
    r = np.where(e > c, c / np.where(e > c, e, 1.0), 1.0)
    h = _window_min(np.concatenate([np.ones(la), r, np.ones(la)]), la + Z)      # h[j], j = -L .. n + L - 1
    s = np.convolve(h, weights(la))[2 * la:2 * la + n]                          # symmetric weights
    reach = _window_min(r, 2 * la + Z) < 1.0
    g = np.where(reach, np.minimum(np.minimum(s, r), 1.0 - 2.0 ** -24), 1.0)
    y = xin * (g[:, None] if xin.ndim == 2 else g)
    return y, g


def _window_min(v, radius):
    """min of v over |k - j| <= radius for every j (ones outside), by doubling shifts."""
    n = len(v)
    p = np.concatenate([np.ones(radius), v, np.ones(radius)])
    want, have = 2 * radius + 1, 1                                 # p[j] = min over p[j .. j + have - 1]
    while have < want:
        s = min(have, want - have)
        p = np.minimum(p[:len(p) - s], p[s:])
        have += s
    return p[:n]


def limit_host(x, sr, ceiling_dbtp, lookahead_ms=5.0, lookahead=None):
    """msg_limit_host: the library's loop on the host (no device), the device's arithmetic
    to the bit.  Returns (y, rec): a limited float32 copy of x and the record (a LIMIT_DTYPE
    scalar).  ``lookahead``: the look-ahead in frames instead of ``lookahead_ms``."""
    oversampling(sr)
    a, channels = _signal(x)
    y = a.copy()
    la = lookahead_frames(sr, lookahead_ms) if lookahead is None else int(lookahead)
    rec = np.zeros(1, dtype=LIMIT_DTYPE)
    L.check(L.lib().msg_limit_host(y.ctypes.data_as(C.c_void_p), channels, int(y.shape[0]), int(sr),
                                   _ceiling(ceiling_dbtp), la, rec.ctypes.data_as(C.c_void_p)), None)
    return y, rec[0]


def records(rec):
    """Device records (Engine.limit) as a LIMIT_DTYPE array on the host; waits for them."""
    return read_records(rec, LIMIT_DTYPE)


def limit(x, sr, ceiling_dbtp=-1.0, lookahead_ms=5.0, device: int = 0):
    """Limit x, (n,) mono or (n, 2) stereo at ``sr`` Hz, to ``ceiling_dbtp`` dBTP with a
    look-ahead of ``lookahead_ms`` on the device.  NumPy in: (a limited float32 copy, its
    record).  A device tensor in: limited in place, enqueued on the current stream (no host
    synchronise); returns the device record tensor (limit.records reads it)."""
    from .engine import default_engine

    oversampling(sr)
    c = _ceiling(ceiling_dbtp)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x, in_place=True)
    rec = eng.limit(t, [0], [int(t.shape[0])], channels, int(sr), c, lookahead_frames(sr, lookahead_ms))
    if not on_host:
        return rec
    return t.cpu().numpy(), records(rec)[0]
