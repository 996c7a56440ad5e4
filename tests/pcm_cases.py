"""Seeded signals of the PCM quantiser's tests (tests/test_pcm_host.py on the CPU,
tests/test_gpu_pcm.py on the device).

Every comparison between the host loop, the NumPy restatement and the device is for
equal bits, so there are no tolerances here; the statistical bounds of the dither stream
and of the dithered error are stated with the tests that hold them.
"""
import functools

import numpy as np

from msgpu.pcm import PCM_DTYPE, pack

# words per signal: empty, below and around one lane's four words and one store's
# dwords, around one tile (4096 words), more than two tiles at no multiple of anything
WORDS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 4095, 4096, 4097, 8195, 20011)
SCALES = (0.3, 1.2)          # 1.2: clipping occurs
BITS = (16, 24)
DITHERS = ("tpdf", "none")
SEED = 7


@functools.lru_cache(maxsize=None)
def signal(words, channels, scale):
    """Seeded normals scaled by ``scale``: (words / channels, channels) or (words,) float32;
    None where ``words`` is no multiple of ``channels``.  Shared: do not write to it."""
    if words % channels:
        return None
    rng = np.random.default_rng(100000 * channels + 10 * words + int(scale * 10))
    x = (rng.standard_normal(words) * scale).astype(np.float32)
    if channels == 2:
        x = x.reshape(-1, 2)
    x.setflags(write=False)
    return x


def signals(channels):
    """Every signal of one channel count: both scales at every length that fits."""
    out = [signal(w, channels, s) for w in WORDS for s in SCALES]
    return [x for x in out if x is not None]


def same(q, rec, q2, rec2, bits, what=""):
    """Two quantiser results agree to the bit: packed bytes and records."""
    assert q.shape == q2.shape and q.dtype == q2.dtype, (what, q.shape, q2.shape, q.dtype, q2.dtype)
    assert np.array_equal(pack(q, bits), pack(q2, bits)), what
    a, b = np.asarray(rec, dtype=PCM_DTYPE).reshape(1), np.asarray(rec2, dtype=PCM_DTYPE).reshape(1)
    assert a.tobytes() == b.tobytes(), (what, rec, rec2)
