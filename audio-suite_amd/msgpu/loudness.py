"""Integrated loudness of renders on the device (msg_loudness, DESIGN.md "Loudness").

ITU-R BS.1770-4: K-weighting (a high shelf and a high-pass biquad, designed here
for any rate with ``sr % 10 == 0`` from the analogue prototype, so that 48 kHz gives
the standard's table), 400 ms blocks at 75 % overlap (complete blocks only, channel
weights 1), the absolute gate at -70 LUFS and the relative gate 10 LU under the mean
of the blocks that pass it.  The device measures float32 signals where they lie, in
float64; :func:`loudness_reference` restates the definition in float64 NumPy for the
tests, and nothing on the product path uses it.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records

# Tiles of the kernels (csrc/loudness.h): every hop of sr / 10 frames is cut into
# tiles of TILE frames with a shorter last one, a tile into lane chunks of CHUNK frames.
TILE = 4096
CHUNK = 16
SR_MIN = 4000

# msg_loudness_rec as a numpy record
LOUDNESS_DTYPE = np.dtype([("lufs", "<f8"), ("mean_sq", "<f8"), ("peak", "<f8"), ("gain", "<f8"),
                           ("n_blocks", "<i4"), ("n_kept", "<i4")])


def _check_rate(sr):
    sr = int(sr)
    if sr < SR_MIN or sr % 10:
        raise ValueError("the sample rate must be a multiple of 10, at least 4000")
    return sr


def kweight(sr):
    """The K-weighting at ``sr`` in float64: ((b_shelf, a_shelf), (b_highpass, a_highpass)),
    each three coefficients with a[0] = 1."""
    sr = _check_rate(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    d = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d])
    return (b1, a1), (b2, a2)


def _biquad(b, a, x):
    try:
        from scipy.signal import lfilter
    except ImportError:
        y = np.empty_like(x)
        z1 = z2 = 0.0
        b0, b1, b2, a1, a2 = float(b[0]), float(b[1]), float(b[2]), float(a[1]), float(a[2])
        for i, v in enumerate(x.tolist()):
            o = b0 * v + z1
            z1 = b1 * v - a1 * o + z2
            z2 = b2 * v - a2 * o
            y[i] = o
        return y
    return lfilter(b, a, x)


def block_levels(x, sr):
    """(z, l): every complete block's mean square z_j and level l_j of x, (n,) or (n, channels)."""
    sr = _check_rate(sr)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    hop = sr // 10
    n = x.shape[0]
    nb = 0 if n < 4 * hop else (n - 4 * hop) // hop + 1
    if nb == 0:
        return np.zeros(0), np.zeros(0)
    (b1, a1), (b2, a2) = kweight(sr)
    e = np.zeros(n)
    for c in range(x.shape[1]):
        y = _biquad(b2, a2, _biquad(b1, a1, x[:, c]))
        e += y * y
    hs = e[:(nb + 3) * hop].reshape(nb + 3, hop).sum(axis=1)
    z = (hs[0:nb] + hs[1:nb + 1] + hs[2:nb + 2] + hs[3:nb + 3]) / (4.0 * hop)
    with np.errstate(divide="ignore"):
        return z, -0.691 + 10.0 * np.log10(z)


def gate_levels(x, sr):
    """(z, l, gamma): block_levels and the relative gate (None when no block passes -70)."""
    z, l = block_levels(x, sr)
    k1 = l > -70.0
    if not k1.any():
        return z, l, None
    return z, l, -0.691 + 10.0 * math.log10(float(z[k1].mean())) - 10.0


def loudness_reference(x, sr):
    """The definition in float64 NumPy: integrated loudness of x, (n,) or (n, channels), in
    LUFS; -inf when no block survives the gates."""
    z, l, gamma = gate_levels(x, sr)
    if gamma is None:
        return -math.inf
    k2 = (l > -70.0) & (l > gamma)
    if not k2.any():
        return -math.inf
    return -0.691 + 10.0 * math.log10(float(z[k2].mean()))


def loudness_host(x, sr):
    """msg_loudness_host: the library's sequential float64 loop on the host (no device);
    returns the record (a LOUDNESS_DTYPE scalar)."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
        raise ValueError("x must be (n,) or (n, 2)")
    channels = 1 if a.ndim == 1 else int(a.shape[1])
    rec = np.zeros(1, dtype=LOUDNESS_DTYPE)
    L.check(L.lib().msg_loudness_host(a.ctypes.data_as(C.c_void_p), channels, int(a.shape[0]), int(sr),
                                      rec.ctypes.data_as(C.c_void_p)), None)
    return rec[0]


def records(rec):
    """Device records (Engine.loudness) as a LOUDNESS_DTYPE array on the host; waits for them."""
    return read_records(rec, LOUDNESS_DTYPE)


def loudness(x, sr, device: int = 0):
    """Integrated loudness of x, (n,) mono or (n, 2) stereo, at ``sr`` Hz, measured on the
    device.  NumPy in, a float out; a device tensor in, a one-element device tensor of
    LUFS out, enqueued on the current stream (no host synchronise)."""
    from .engine import default_engine

    sr = _check_rate(sr)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x)
    rec = eng.loudness(t, [0], [int(t.shape[0])], channels, sr)
    if not on_host:
        return rec[0, :1]
    return float(records(rec)["lufs"][0])
