"""Seeded signals of the loudness tests (tests/test_loudness_host.py on the CPU,
tests/test_gpu_loudness.py on the device), with the two input rules they are built
to meet, asserted on the reference's own block values:

rule 1  no block level lies within 1e-3 LU of -70 or of the signal's relative gate,
        so a rounding difference cannot flip a gate;
rule 2  (normalisation) every block is above -50 LUFS and the shift is at most 15 dB,
        so the absolute gate selects the same blocks after scaling.
"""
import functools
import math

import numpy as np

from msgpu.loudness import gate_levels, loudness_reference

RATES = (44100, 48000, 384000)
TOL = 1e-6            # LU, float64 against float64 on the same float32 samples


def db(x):
    return 10.0 ** (x / 20.0)


def sine(sr, dur, dbfs, f=1000.0, channels=2, phase0=0):
    t = (np.arange(int(round(dur * sr))) + phase0) / sr
    x = (db(dbfs) * np.sin(2 * np.pi * f * t)).astype(np.float32)
    return np.stack([x] * channels, axis=1) if channels == 2 else x


def tone_sequence(sr):
    """1 kHz stereo tones at -36 / -23 / -36 dBFS for 1 / 3 / 1 s, one phase throughout:
    the relative gate drops the quiet parts."""
    n = [d * sr for d in (1, 3, 1)]
    amp = np.concatenate([np.full(k, db(a)) for k, a in zip(n, (-36, -23, -36))])
    x = (amp * np.sin(2 * np.pi * 1000.0 * np.arange(sum(n)) / sr)).astype(np.float32)
    return np.stack([x, x], axis=1)


def flanked(sr):
    """tone_sequence between 1 s of the tone at -72 dBFS on either side: the absolute
    gate drops the flanks.  The middle holds tone_sequence's samples, ten hops later."""
    f = sine(sr, 1.0, -72.0)
    return np.concatenate([f, tone_sequence(sr), f])


def noise_steps(sr, channels, seed, step_s=0.5, steps=8):
    """Seeded Gaussian noise whose RMS steps through -60, -40, -20, -10 dB every step_s."""
    rng = np.random.default_rng(seed)
    k = int(round(step_s * sr))
    lv = [(-60, -40, -20, -10)[i % 4] for i in range(steps)]
    amp = np.concatenate([np.full(k, db(a)) for a in lv])
    shape = (k * steps, 2) if channels == 2 else (k * steps,)
    x = rng.standard_normal(shape) * (amp[:, None] if channels == 2 else amp)
    return x.astype(np.float32)


def dc_tone_noise(sr=384000, dur=0.6, seed=5):
    """DC 0.5 + a 20 Hz tone + 1e-3 noise: the states of the high-pass stand far above
    its output, where a float32 cascade at 384 kHz is 0.285 LU off."""
    n = int(round(dur * sr))
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    return (0.5 + 0.25 * np.sin(2 * np.pi * 20.0 * t) + 1e-3 * rng.standard_normal(n)).astype(np.float32)


def programme(sr, dur, channels, seed):
    """Noise around -20 dB with a slow level wobble of a few dB: every block far above
    -50 LUFS (rule 2)."""
    rng = np.random.default_rng(seed)
    n = int(round(dur * sr))
    env = db(-20.0 + 4.0 * np.sin(2 * np.pi * 0.7 * np.arange(n) / sr + seed))
    x = rng.standard_normal((n, 2) if channels == 2 else n) * (env[:, None] if channels == 2 else env)
    return x.astype(np.float32)


def check_rule1(x, sr):
    z, l, gamma = gate_levels(x, sr)
    fin = l[np.isfinite(l)]
    assert fin.size == 0 or np.min(np.abs(fin + 70.0)) > 1e-3, "rule 1: a block at the absolute gate"
    if gamma is not None:
        assert np.min(np.abs(fin - gamma)) > 1e-3, "rule 1: a block at the relative gate"
    return l


def check_rule2(x, sr, target):
    l = check_rule1(x, sr)
    assert l.size and float(l.min()) > -50.0, "rule 2: a block at or under -50 LUFS"
    ref = loudness_reference(x, sr)
    assert abs(target - ref) <= 15.0, "rule 2: a shift beyond 15 dB"
    return ref


def check_export_shift(x, sr, target):
    """The export cases: rule 1, every block above -50 LUFS, and what rule 2 is there
    for, asserted directly: moved by the shift, every block stays 5 LU and more above
    the absolute gate, so it selects the same blocks after scaling.  (The C2 renders
    lie at -3.5 and -2.3 LUFS, so delivering them at -23 LUFS is a shift of 19.5 and
    20.7 dB, beyond the 15 dB rule 2 allows; their quietest block lands at -25 LUFS.)"""
    l = check_rule1(x, sr)
    assert l.size and float(l.min()) > -50.0, "rule 2: a block at or under -50 LUFS"
    ref = loudness_reference(x, sr)
    assert float(l.min()) + (target - ref) > -65.0, "a block within 5 LU of the absolute gate after the shift"
    return ref


@functools.lru_cache(maxsize=None)
def case(name, sr):
    """(signal, reference LUFS) of a named case, computed once per session; the arrays
    are shared: do not write to them."""
    kind, _, arg = name.partition(":")
    if kind == "sine":
        x = sine(sr, 3.0, float(arg))
    elif kind == "sequence":
        x = tone_sequence(sr)
    elif kind == "flanked":
        x = flanked(sr)
    elif kind == "noise":
        x = noise_steps(sr, int(arg), seed=sr % 1000 + int(arg), step_s=0.375 if sr == 384000 else 0.5,
                        steps=4 if sr == 384000 else 8)
    elif kind == "dc":
        x = dc_tone_noise(sr)
    else:
        raise KeyError(name)
    x.setflags(write=False)
    check_rule1(x, sr)
    return x, loudness_reference(x, sr)


# (name, rates): the CPU signals; the 384 kHz ones stay at or under 1.5 s apart from the
# 3 s sine anchors the standard's conformance window is quoted for, so the 5 and 7 s
# tone sequences run at 44.1 and 48 kHz
CPU_CASES = [("sequence", (44100, 48000)), ("flanked", (44100, 48000)), ("noise:1", RATES), ("noise:2", RATES)]


def lengths_48k():
    hop = 4800
    return [(0, 0), (1, 0), (4 * hop - 1, 0), (4 * hop, 1), (4 * hop + 1, 1), (5 * hop - 1, 1), (5 * hop, 2)]


def close_lu(a, b, tol=TOL):
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= tol
