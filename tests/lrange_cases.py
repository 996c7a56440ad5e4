"""Seeded signals of the loudness-range tests (tests/test_lrange_host.py on the CPU,
tests/test_gpu_lrange.py on the device) with their float64 NumPy reference
(msgpu.lrange.lrange_reference).

Input rule: no short-term level of a case lies within 1e-3 LU of -70 or of the case's
relative gate (``margin`` of the reference, asserted by ``case`` and again by every test),
so a perturbation of 1e-6 LU, the bar of the comparisons, cannot move a window across a gate.

Bars: 1e-6 LU on every level, the project's loudness bar (float64 on both sides over the
same float32 samples, tests/test_loudness_host.py); an order statistic moves no more than
its inputs, and lra is the difference of two levels: 2e-6.
"""
import functools
import math

import numpy as np

from loudness_cases import db
from msgpu.lrange import hops_reference, lrange_reference

TOL = 1e-6
TOL_LRA = 2e-6
MARGIN = 1e-3
LEVELS = ("lo", "hi", "max_momentary", "max_short")
COUNTS = ("n_momentary", "n_short", "n_abs", "n_kept")
ZS = ("z_lo", "z_hi", "z_max_m", "z_max_s")

# EBU Tech 3342 tone sequences: (segment levels in dBFS, the expected LRA in LU, within 1 LU)
TECH_3342 = {"10": ((-20, -30), 10.0), "5": ((-20, -15), 5.0), "20": ((-40, -20), 20.0),
             "15": ((-50, -35, -20, -35, -50), 15.0)}


def tone_steps(sr, levels, seg_s, f):
    """A stereo sine at f Hz, one phase throughout, stepping through ``levels`` dBFS every seg_s seconds."""
    n = int(round(seg_s * sr))
    amp = np.concatenate([np.full(n, db(a)) for a in levels])
    x = (amp * np.sin(2 * np.pi * f * np.arange(amp.size) / sr)).astype(np.float32)
    return np.stack([x, x], axis=1)


def noise_steps(sr, dur_s, channels, seed, step_s=0.5, levels=(-45, -30, -18, -12, -24, -36)):
    """Seeded Gaussian noise whose RMS steps through ``levels`` dB every step_s seconds."""
    rng = np.random.default_rng(seed)
    n, k = int(round(dur_s * sr)), int(round(step_s * sr))
    amp = db(np.asarray(levels, dtype=np.float64))[(np.arange(n) // k) % len(levels)]
    x = rng.standard_normal((n, 2) if channels == 2 else n) * (amp[:, None] if channels == 2 else amp)
    return x.astype(np.float32)


def kept_257(sr=4000):
    """A 500 Hz tone at -20 dBFS for 25.7 s after 5 s at -60: of the 278 short-term windows the
    21 that lie wholly in the quiet part fall under the relative gate, 257 are kept."""
    return tone_steps(sr, (-60,), 5.0, 500.0), tone_steps(sr, (-20,), 25.7, 500.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """(signal, sr, reference dict) of a named case, computed once per session; the arrays are
    shared: do not write to them."""
    kind, _, arg = name.partition(":")
    if kind == "tech48k":                       # the Tech 3342 sequences as published: 20 s segments at 48 kHz
        x, sr = tone_steps(48000, TECH_3342[arg][0], 20.0, 1000.0), 48000
    elif kind == "tech4k":                      # their small shape: 6 s segments of a 500 Hz tone at 4 kHz
        x, sr = tone_steps(4000, TECH_3342[arg][0], 6.0, 500.0), 4000
    elif kind == "noise48k":                    # 8 s: two tiles per hop
        x, sr = noise_steps(48000, 8.0, 2, 11, step_s=0.9), 48000
    elif kind == "noise384k":                   # 3.3 s: ten tiles per hop, four windows
        x, sr = noise_steps(384000, 3.3, 2, 12, step_s=0.4), 384000
    elif kind == "long4k":                      # 120 s: 1171 windows, more than the workgroup has threads
        x, sr = noise_steps(4000, 120.0, int(arg or 2), 13, step_s=7.0), 4000
    elif kind == "kept257":
        x, sr = np.concatenate(kept_257()), 4000
    elif kind == "len4k":                       # hops:extra frames:channels at 4 kHz
        hops, extra, ch = (int(v) for v in arg.split(":"))
        x, sr = noise_steps(4000, (hops * 400 + extra) / 4000.0, ch, 100 + hops + extra, step_s=0.7), 4000
    else:
        raise KeyError(name)
    x.setflags(write=False)
    ref = lrange_reference(x, sr)
    assert ref["margin"] >= MARGIN, (name, ref["margin"])
    return x, sr, ref


LENGTHS_4K = [(29, 0), (30, 0), (31, 0), (30, 399), (3, 0), (0, 0)]     # (hops, extra frames)


def close(a, b, tol):
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol


def check_record(r, ref, what=""):
    """A record (a LRANGE_DTYPE scalar) against a reference dict at the bars above; prints the figures first."""
    assert ref["margin"] >= MARGIN, (what, ref["margin"])
    print(f"{what}: lra {float(r['lra']):.9f} ref {ref['lra']:.9f} diff {float(r['lra']) - ref['lra']:.2e}; " +
          " ".join(f"{k} {float(r[k]) - ref[k]:.2e}" for k in LEVELS if math.isfinite(ref[k])) +
          f"; kept {int(r['n_kept'])}/{int(r['n_short'])} margin {ref['margin']:.3g}")
    for k in COUNTS:
        assert int(r[k]) == ref[k], (what, k, int(r[k]), ref[k])
    for k in LEVELS + ("gate",):
        assert close(float(r[k]), ref[k], TOL), (what, k, float(r[k]), ref[k])
    assert close(float(r["lra"]), ref["lra"], TOL_LRA), (what, float(r["lra"]), ref["lra"])


def same_bits(a, b):
    return np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))


__all__ = ["case", "check_record", "hops_reference", "same_bits"]
