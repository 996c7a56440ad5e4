"""Sample-rate conversion of renders on the device (msg_resample, DESIGN.md "Resampler").

Rational resampling by ``up / down`` with a Kaiser-windowed sinc prototype designed
here in float64; the device runs it as a float32 polyphase FIR where the audio lies.
The output is zero-phase and zero-extended at both ends::

    y[k] = up * sum_m h[k*down + half - m*up] * x[m],   n_out = ceil(n * up / down)

which is ``scipy.signal.resample_poly(x, up, down, window=h)`` with its default
constant padding.  :func:`resample_reference` restates the formula in float64
NumPy for the tests; nothing on the product path uses it.
"""
from __future__ import annotations

import math

import numpy as np

from ._signal import device_signal

ZEROS, BETA, ROLLOFF = 32, 12.0, 0.9

# Output tiles of the kernels (csrc/resample.h).  Integer decimation by 2, 4 or 8
# runs on its own kernel with tiles of TILE_DECIMATE output frames; every other
# ratio on the general kernel, whose tile is BLOCK outputs for each of up * G
# lanes (G phase periods, see tile_frames).
TILE_DECIMATE = 512
BLOCK = 4
LANES = 256
LDS_BYTES = 65536
TABLE_MAX = 1 << 20      # phase-major tap table, floats


def ratio(sr_in, sr_out):
    """(up, down) with up / down = sr_out / sr_in in lowest terms."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError("sample rates must be positive")
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def resample_len(n, up, down):
    """Output frames of n input frames: ceil(n * up / down)."""
    return -((-int(n) * int(up)) // int(down))


def design(up, down, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """The prototype low-pass at the rate up x the input rate: K = 2*zeros*max(up, down) + 1
    float64 taps, Kaiser-windowed sinc with cutoff rolloff / max(up, down), unit sum."""
    D = max(int(up), int(down))
    half = int(zeros) * D
    i = np.arange(-half, half + 1, dtype=np.float64)
    fc = float(rolloff) / D
    h = fc * np.sinc(fc * i) * np.kaiser(2 * half + 1, float(beta))
    return h / h.sum()


def resample_reference(x, up, down, h):
    """The formula above in float64: x (n,) or (n, channels), h odd-length taps."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    if x.ndim == 2:
        return np.stack([resample_reference(x[:, c], up, down, h) for c in range(x.shape[1])], axis=1)
    up, down = int(up), int(down)
    K, n = h.size, x.size
    half = (K - 1) // 2
    n_out = resample_len(n, up, down)
    if n_out == 0:
        return np.zeros(0, dtype=np.float64)
    # output k: taps h[p + q*up] against x[m0 - q], p = (k*down + half) mod up, m0 = (k*down + half) // up
    num = np.arange(n_out, dtype=np.int64) * down + half
    m0, p = num // up, num % up
    Q = (K + up - 1) // up
    hp = np.zeros(Q * up, dtype=np.float64)
    hp[:K] = h
    xp = np.concatenate([np.zeros(Q), x, np.zeros(max(0, int(m0.max()) + 1 - n))])
    y = np.zeros(n_out, dtype=np.float64)
    for q in range(Q):
        y += hp[p + q * up] * xp[m0 - q + Q]
    return up * y


def tile_frames(up, down, K, channels):
    """Output frames per workgroup tile for this ratio (csrc/resample.h, rs_plan);
    raises NotImplementedError beyond the kernels' limits."""
    up, down, K, channels = int(up), int(down), int(K), int(channels)
    if up == 1 and down in (2, 4, 8):
        A = ((K - 1) // down + 1 + 7) & ~7
        row = TILE_DECIMATE + A
        if ((row >> 2) & 1) == 0:
            row += 4
        if channels * down * row * 4 <= LDS_BYTES:
            return TILE_DECIMATE
    Q4 = ((K + up - 1) // up + 3) & ~3
    G = 1 if up >= LANES else LANES // up
    while True:
        L, step = G * up, G * down
        span = Q4 + ((L - 1) * down) // up + 2 + (BLOCK - 1) * step
        nbytes = (span * channels + 8) * 4
        if nbytes <= LDS_BYTES or G == 1:
            break
        G //= 2
    if nbytes > LDS_BYTES or up * Q4 > TABLE_MAX:
        raise NotImplementedError("ratio beyond the resampler's tap-table or LDS limit")
    return BLOCK * L


def resample(x, sr_in, sr_out, device: int = 0, **design_kw):
    """Resample x, (n,) mono or (n, 2) stereo, from sr_in to sr_out on the device.
    A NumPy input returns float32 NumPy; a device tensor returns a device tensor
    enqueued on the current stream (no host synchronise)."""
    from .engine import default_engine

    up, down = ratio(sr_in, sr_out)
    eng = default_engine(device)
    torch = eng.torch
    t, channels, on_host = device_signal(eng, x)
    n = int(t.shape[0])
    h = None
    if up != down:      # the limits first: a ratio beyond them would design millions of taps
        tile_frames(up, down, 2 * int(design_kw.get("zeros", ZEROS)) * max(up, down) + 1, channels)
        h = design(up, down, **design_kw)
    y, _, _ = eng.resample(t, [0], [n], channels, up, down, h)
    y = y.reshape((resample_len(n, up, down),) + tuple(t.shape[1:]))
    if not on_host:
        return y
    torch.cuda.synchronize(eng.device)
    return y.cpu().numpy()
