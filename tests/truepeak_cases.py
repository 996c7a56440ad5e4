"""Seeded signals and bounds of the true-peak tests (tests/test_truepeak_host.py on the
CPU, tests/test_gpu_truepeak.py on the device).

The bounds come from the taps, not from what the code gives:

L1     max over the phases of sum |t_p[q]| (2.249 for both factors): no oversampled value
       exceeds L1 x the sample peak;
E      (2 Z + 1) 2^-24 L1: one rounding of each float32 tap and 24 fused float32 steps,
       each at most 2^-24 of a partial sum that L1 x peak bounds, relative to the sample
       peak (which is <= the true peak): 3.35e-6, or 2.9e-5 dB.  The float32 restatement
       measured at most 1.3e-7 on these lengths, so the bound is a roof, not a fit.
"""
import functools
import math
from decimal import Decimal, getcontext

import numpy as np

from msgpu.truepeak import TILE, Z, oversampling, taps, true_peak_reference

RATES = (48000, 96000)
LENGTHS = (0, 1, 2, 11, 12, 13, 23, 24, 25, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 20011)


def l1(os):
    return float(np.abs(taps(os)).sum(axis=1).max()) if os > 1 else 0.0


L1 = max(l1(2), l1(4))
E = (2 * Z + 1) * 2.0 ** -24 * L1
# after a gain: the device's reading, the rounding of g to float32 and of every scaled
# sample (each 2^-24 of a sample, L1 of them at worst in one oversampled value)
E_GAIN = E + (2 + L1) * 2.0 ** -24


def db_exact(v):
    """20 log10(v) rounded once to float64 (60 digits, then one rounding); -inf for 0."""
    v = float(v)
    if math.isnan(v):
        return math.nan
    if v == 0.0:
        return -math.inf
    getcontext().prec = 60
    return float(20 * Decimal(v).log10())


def noise(n, channels, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 2) if channels == 2 else n) * 0.1).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case(n, channels, sr):
    """(signal, reference true peak, sample peak) of a seeded signal, computed once per
    session; the arrays are shared: do not write to them."""
    x = noise(n, channels, 1000 * channels + n % 997)
    peak = float(np.max(np.abs(x))) if n else 0.0
    return x, true_peak_reference(x, sr), peak


def faded_sine():
    """0.5 fade sin(2 pi n / 4 + pi / 4): 4800 frames, raised-cosine fades of 1200 (an
    abrupt start overshoots by 0.1 dB).  The samples sit at 0.35355, the sine's peaks
    half way between them."""
    n = np.arange(4800)
    fade = np.ones(4800)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(1200) + 0.5) / 1200)
    fade[:1200] = ramp
    fade[-1200:] = ramp[::-1]
    return (0.5 * fade * np.sin(2 * np.pi * n / 4 + np.pi / 4)).astype(np.float32)


def pair_signal(n, at, channels):
    """[1, 1] at frames at, at + 1 amid zeros; the stereo right channel is -0.5 x the left."""
    x = np.zeros((n, 2) if channels == 2 else n, dtype=np.float32)
    if channels == 2:
        x[at:at + 2] = (1.0, -0.5)
    else:
        x[at:at + 2] = 1.0
    return x


def check_record(r, x, sr, ref=None, host=None):
    """A record (host's or device's) against the reference within E x peak, and the
    record's own consistency; returns the reference."""
    ref = true_peak_reference(x, sr) if ref is None else ref
    peak = float(np.max(np.abs(x))) if len(x) else 0.0
    assert r["peak"] == peak
    assert r["os"] == oversampling(sr)
    assert r["true_peak"] >= r["peak"]
    assert abs(float(r["true_peak"]) - ref) <= E * peak, (float(r["true_peak"]), ref, E * peak)
    assert r["dbtp"] == db_exact(r["true_peak"]), (float(r["dbtp"]), db_exact(r["true_peak"]))
    assert r["gain"] == 0.0
    if host is not None:                                   # to the bit
        assert np.array_equal(np.asarray(r).reshape(1).view(np.uint8), np.asarray(host).reshape(1).view(np.uint8))
    return ref
