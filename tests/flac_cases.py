"""The signals the FLAC tests share (test_flac_host.py, test_gpu_flac.py): integer audio by content
and length, made once per (name, length, channels, bits)."""
import functools

import numpy as np

SR = 48000
LENGTHS = (0, 1, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8192 + 17)
CONTENT = ("constant", "noise", "alternation", "sine", "lone", "equal", "gauss", "opposite", "silent_right", "extreme")


def int_dtype(bits):
    return np.int16 if bits == 16 else np.int32


def tpdf(rng, shape):
    return rng.random(shape) - rng.random(shape)


@functools.lru_cache(maxsize=None)
def _content(name, n, channels, bits):
    S = 1 << (bits - 1)
    rng = np.random.default_rng(len(name) * 7919 + n * 31 + channels * 3 + bits)
    i = np.arange(n)
    if name == "constant":                       # every sample equal: a constant subframe
        x = np.stack([np.full(n, 1234), np.full(n, -77)], axis=1)
    elif name == "noise":                        # full-scale uniform noise: verbatim
        x = rng.integers(-S, S, (n, 2))
    elif name == "alternation":                  # +- full scale: verbatim
        a = np.where(i & 1, S - 1, -S)
        x = np.stack([a, a], axis=1)
    elif name == "sine":                         # -20 dBFS, 440 Hz, TPDF
        s = 0.1 * S * np.sin(2 * np.pi * 440.0 * i / SR)
        x = np.rint(np.stack([s, 0.7 * s], axis=1) + tpdf(rng, (n, 2)))
    elif name == "lone":                         # a lone full-scale sample in silence
        a = np.zeros(n)
        if n:
            a[n // 2] = S - 1
        x = np.stack([a, a * 0], axis=1)
    elif name == "equal":                        # L = R: a constant side channel
        a = np.rint(0.05 * S * rng.standard_normal(n))
        x = np.stack([a, a], axis=1)
    elif name == "gauss":                        # Gaussian noise at 0.1 of full scale
        x = np.clip(np.rint(0.1 * S * rng.standard_normal((n, 2))), -S, S - 1)
    elif name == "opposite":                     # L = -R
        a = np.clip(np.rint(0.05 * S * rng.standard_normal(n)), -S + 1, S - 1)
        x = np.stack([a, -a], axis=1)
    elif name == "silent_right":
        x = np.stack([np.rint(0.02 * S * rng.standard_normal(n)), np.zeros(n)], axis=1)
    elif name == "extreme":                      # +- full-scale alternation with L = -R: the largest residuals
        a = np.where(i & 1, S - 1, -(S - 1))
        x = np.stack([a, -a], axis=1)
    else:
        raise KeyError(name)
    q = np.ascontiguousarray(x[:, :channels].astype(int_dtype(bits)))
    q.setflags(write=False)
    return q


def signal(name, n, channels, bits):
    """(n, channels) integer audio (int16, or int32 at 24 bits), read-only."""
    return _content(name, int(n), int(channels), int(bits))
