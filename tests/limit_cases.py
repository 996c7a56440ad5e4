"""Seeded signals and bounds of the limiter tests (tests/test_limit_host.py on the CPU,
tests/test_gpu_limit.py on the device).

The bounds come from the taps and the weights, not from what the code gives.

The host's distance from limit_reference, per sample:

    |y - y_ref| <= |x| (E peak / c + (2 L + 4) 2^-24)

E peak / c  E is truepeak_cases.E: the float32 envelope lies within E x (sample peak) of the
            float64 one.  r = min(1, c / e) is continuous with slope c / e^2 <= 1 / c where it
            binds (e >= c), so r moves by at most E peak / c.  The hold is a minimum and the
            smoothing a sum with positive weights of unit sum, on values in (0, 1]: neither
            enlarges a sup-norm error, nor does g = min(s, r).
(2 L + 4) 2^-24  the roundings, each at most 2^-25 of a value that 1 bounds: c to float32,
            the quotient, the weights (2^-25 of each, unit sum: one in all), the 2 L + 1
            fused steps of the chain, the product g x: 2 L + 5 of them, and
            (2 L + 5) 2^-25 < (2 L + 4) 2^-24.  The cap of g at 1 - 2^-24 is in the reference too.
A frame whose float64 envelope lies within E peak of c may be over the ceiling on one side
and not on the other (a "borderline" frame).  Its r is within E peak / c of 1 on both sides,
so the bound above still holds for every sample; what can differ is which frames count as
limited, and only within the reach (2 L + Z) of a borderline frame.  The tests list the
borderline frames of each case and hold their share under 0.1 %.

After the limiter on an isolated peak the true peak is g tp with one g over the
interpolator's window: c to within truepeak_cases.E_GAIN (the reading, the rounding of g and
of every scaled sample).
"""
import functools

import numpy as np

import truepeak_cases as TC
from msgpu.limit import envelope_reference, limit_reference, tile
from msgpu.truepeak import Z

RATES = (48000, 96000, 192000)               # OS 4, 2, 1
LOOKAHEADS = (1, 12, 72, 240)
CEILING_DB = -1.0
C = 10.0 ** (CEILING_DB / 20.0)              # what the library forms from -1 dBTP
C32 = float(np.float32(C))
PEAK_ROOF = C32 * (1.0 + 2.0 ** -22)         # the sample-peak guarantee (csrc/limit.h)
BORDERLINE_SHARE = 1e-3


def lengths(la):
    t = tile(la)
    return (0, 1, 2, 12, 25, la, 2 * la + 13, t - 1, t, t + 1, 2 * t + 1, 20011)


def gain_bound(peak, la, c=C):
    """The bound on |g - g_ref|, and per unit of |x| on |y - y_ref|."""
    return TC.E * peak / c + (2 * la + 4) * 2.0 ** -24


def spiky(n, channels, seed):
    """Seeded noise at 0.1 with a handful of spikes at 1 .. 2 (both signs); read-only."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, 2) if channels == 2 else n) * 0.1).astype(np.float32)
    k = min(5, n)
    if k:
        at = rng.choice(n, size=k, replace=False)
        v = (rng.uniform(1.0, 2.0, size=k) * rng.choice([-1.0, 1.0], size=k)).astype(np.float32)
        if channels == 2:
            x[at, rng.integers(0, 2, size=k)] = v
        else:
            x[at] = v
    x.setflags(write=False)
    return x


def dense(n, seed=7):
    """Spiky noise on which the limiter alone overshoots: noise at 0.5 with a spike every few frames."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.5).astype(np.float32)
    at = np.arange(3, n, 7)
    x[at] = (rng.uniform(1.0, 2.0, size=len(at)) * rng.choice([-1.0, 1.0], size=len(at))).astype(np.float32)
    return x


def boundary_distances(la):
    t = tile(la)
    return (t - 1, t, 2 * la + Z, 2 * la + Z + 1)


def boundary_signals(la, channels):
    """Quiet signals of three tiles and a bit, each with one over-ceiling frame d frames
    before or after the tile boundary at frame 2 TILE: a tile that ignores its neighbour's
    peak, or reaches one frame too far, gets a frame wrong."""
    t = tile(la)
    out = []
    for d in boundary_distances(la):
        for at in (2 * t - d, 2 * t + d):
            x = np.array(spiky(3 * t + 5, channels, 31 + d)) * np.float32(0.25)     # its spikes stay under c
            if channels == 2:
                x[at] = (1.5, -0.25)
            else:
                x[at] = 1.5
            x.setflags(write=False)
            out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def envelope(n, channels, sr):
    return envelope_reference(spiky(n, channels, 500 * channels + n % 991), sr)


@functools.lru_cache(maxsize=None)
def case(n, channels, sr, la):
    """(signal, y_ref, g_ref, borderline frames) of a seeded spiky signal, computed once per
    session; the arrays are shared: do not write to them."""
    x = spiky(n, channels, 500 * channels + n % 991)
    y, g = limit_reference(x, sr, C, la)
    return x, y, g, borderline(x, envelope(n, channels, sr))


def borderline(x, e):
    """Frames whose float64 envelope lies within E x peak of the ceiling."""
    peak = float(np.max(np.abs(x))) if len(x) else 0.0
    return np.flatnonzero(np.abs(e - C) <= TC.E * peak)


def check_against_reference(x, y, rec, sr, la, ref=None, what=""):
    """A limited signal and its record (host's or device's) against limit_reference within
    the bound, and the record's own consistency.  Returns the reference's (y, g)."""
    x64 = np.asarray(x, dtype=np.float64)
    n = len(x)
    if ref is None:
        y_ref, g_ref = limit_reference(x, sr, C, la)
        border = borderline(x, envelope_reference(x, sr))
    else:
        y_ref, g_ref, border = ref
    peak = float(np.max(np.abs(x64))) if n else 0.0
    tol = gain_bound(peak, la)
    err = np.abs(np.asarray(y, dtype=np.float64) - y_ref)
    worst = float((err - np.abs(x64) * tol).max()) if n else 0.0
    assert worst <= 0.0, (what, worst, float(err.max()), tol)
    assert float(np.max(np.abs(y))) <= PEAK_ROOF if n else True, what
    limited_ref = int((g_ref < 1.0).sum())
    g_min_ref = float(g_ref.min()) if n else 1.0
    assert rec["lookahead"] == la
    assert abs(float(rec["min_gain"]) - g_min_ref) <= tol, (what, float(rec["min_gain"]), g_min_ref)
    assert rec["reduction_db"] == 0.0 - TC.db_exact(rec["min_gain"]), what
    # the count may differ only within the reach of a borderline frame
    slack = min(n, len(border) * (2 * (2 * la + Z) + 1))
    if len(border):
        print(f"{what}: borderline frames {border.tolist()}")
    assert len(border) <= BORDERLINE_SHARE * max(n, 1), (what, border)
    assert abs(int(rec["limited_frames"]) - limited_ref) <= slack, (what, int(rec["limited_frames"]), limited_ref)
    assert rec["state"] == (1 if rec["limited_frames"] else 0)
    if not rec["limited_frames"]:
        assert rec["min_gain"] == 1.0 and np.array_equal(np.asarray(y).view(np.uint32), np.asarray(x).view(np.uint32))
    return y_ref, g_ref


def pack(signals, channels, gap=3):
    """The signals back to back with `gap` frames of NaN around and between them (an odd gap:
    mono signals start at odd floats): (buffer, offsets, lens)."""
    offs, lens, parts = [], [], []
    at = gap
    nan = lambda k: np.full((k, 2) if channels == 2 else k, np.nan, dtype=np.float32)
    parts.append(nan(gap))
    for s in signals:
        offs.append(at)
        lens.append(len(s))
        parts += [np.asarray(s, dtype=np.float32), nan(gap)]
        at += len(s) + gap
    return np.concatenate(parts), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)
