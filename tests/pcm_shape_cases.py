"""Seeded signals of the noise-shaped quantiser's tests (tests/test_pcm_shape_host.py on the
CPU, tests/test_gpu_pcm_shape.py on the device).

Every comparison between the host loop, the NumPy restatement and the device is for equal
bits, so there are no tolerances here; the spectral and statistical bounds are stated with
the tests that hold them.
"""
import functools

import numpy as np

from msgpu.pcm import PCM_DTYPE, SHAPE_CHUNK, SHAPES, pack

CHUNK = SHAPE_CHUNK          # words a lane of the kernel loads ahead (PCM_SHAPE_CHUNK)
# words per signal: empty, below and around one lane's four words, around the longest
# history (K = 9), around one chunk, more than two chunks at no multiple of anything, long
SHORT = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
LONG = (20011,)
WORDS = SHORT + LONG
SCALES = (0.3, 1.2)          # 1.2: clipping occurs
BITS = (16, 24)
DITHERS = ("tpdf", "none")
NAMES = tuple(SHAPES)        # "e3", "lipshitz5", "f9"
SEED = 7


@functools.lru_cache(maxsize=None)
def signal(words, channels, scale):
    """Seeded normals scaled by ``scale``: (words / channels, channels) or (words,) float32;
    None where ``words`` is no multiple of ``channels``.  Shared: do not write to it."""
    if words % channels:
        return None
    rng = np.random.default_rng(300000 * channels + 10 * words + int(scale * 10))
    x = (rng.standard_normal(words) * scale).astype(np.float32)
    if channels == 2:
        x = x.reshape(-1, 2)
    x.setflags(write=False)
    return x


def signals(channels, words=WORDS):
    """Every signal of one channel count: both scales at every length of ``words`` that fits."""
    out = [signal(w, channels, s) for w in words for s in SCALES]
    return [x for x in out if x is not None]


def runs(channels, frames=WORDS):
    """Both scales at every length of ``frames`` taken as frames: every channel run has each of
    the lengths, whatever the channel count."""
    return [signal(n * channels, channels, s) for n in frames for s in SCALES]


def same(q, rec, q2, rec2, bits, what=""):
    """Two quantiser results agree to the bit: packed bytes and records."""
    assert q.shape == q2.shape and q.dtype == q2.dtype, (what, q.shape, q2.shape, q.dtype, q2.dtype)
    assert np.array_equal(pack(q, bits), pack(q2, bits)), what
    a, b = np.asarray(rec, dtype=PCM_DTYPE).reshape(1), np.asarray(rec2, dtype=PCM_DTYPE).reshape(1)
    assert a.tobytes() == b.tobytes(), (what, rec, rec2)


def ntf_power(shape, n_fft):
    """|NTF(f)|^2 at the n_fft // 2 + 1 bin frequencies, formed from the integer table:
    NTF(z) = 1 + sum_k (H_k / 65536) z^-k."""
    h = np.zeros(n_fft)
    h[0] = 1.0
    taps = np.array(SHAPES[shape][1], dtype=np.float64) / 65536.0
    h[1:1 + taps.size] = taps
    return np.abs(np.fft.rfft(h)) ** 2
