"""What the gate's host and device tests share: the signals, the option sets and the tolerances of
the host loop against the float64 reference (msgpu/gate.py, csrc/gate.h).

Tolerances.  The states come from comparisons with the same two float32 thresholds on both sides, so
sh is equal exactly.  The host's reduction r is (ratio - 1)(threshold - level) rounded to the nearest
unit of 2^-32 dB from the library's own log2, the reference's from libm's; both are within 2^-40 dB
times (ratio - 1) of the value, so for the ratios used here (up to 4) the two roundings differ by at
most one unit where the value lies that close to a tie.  A ramp carries that difference unchanged
and the maximum of two ramps keeps it, so E agrees within E_UNITS = 2 units per frame, the
compressor's bound by the same argument (tests/dynamics_cases.py); with ratio = inf nothing is
rounded and E is equal exactly.  A sample is x g: one float32 rounding of the gain (2 units of E
move it by 2^-31 dB, nothing beside 2^-24) and one of the product, so
|y - y_ref| <= 1.01 2^-23 |y_ref| + 2^-149."""
import math

import numpy as np

from dynamics_cases import E_UNITS, LENGTHS, SR, TILE, Y_ABS, Y_REL, bits, hold_ms, spike, within  # noqa: F401
from msgpu.gate import Gate

N3 = 3 * TILE + 5


def texture(n, channels, seed):
    """Sparse grains over a bed of residue, the material a gate is for: noise near -70 dBFS with bursts of
    1 to 400 frames whose level runs from -60 to -20 dB, so that they end on every side of the thresholds
    used here (-40 to -55 dB), and with decaying tails, so that levels linger between the two."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, channels)) * 3e-4
    for _ in range(max(1, n // 1500)):
        at, ln = int(rng.integers(0, max(n, 1))), int(rng.integers(1, 400))
        seg = x[at:at + ln]
        decay = np.exp(-np.arange(len(seg)) / rng.uniform(20.0, 300.0))[:, None]
        seg += rng.standard_normal(seg.shape) * decay * 10.0 ** (rng.uniform(-60.0, -20.0) / 20.0)
    return np.clip(x, -1.0, 1.0).astype(np.float32).reshape((n, channels) if channels == 2 else (n,))


# slow: 10 dB take 24000 frames, so a ramp crosses every tile of N3
OPTIONS = {
    "default": Gate(threshold_db=-46.0),
    "local": Gate(threshold_db=-46.0, hysteresis_db=0.0, hold_ms=0.0),
    "hysteresis alone": Gate(threshold_db=-46.0, hysteresis_db=9.0, hold_ms=0.0),
    "hold alone": Gate(threshold_db=-44.0, hysteresis_db=0.0, hold_ms=hold_ms(37)),
    "ratio 2": Gate(threshold_db=-40.0, ratio=2.0, range_db=24.0, attack_ms=1.0, release_ms=20.0, hold_ms=hold_ms(5)),
    "slow": Gate(threshold_db=-40.0, attack_ms=500.0, release_ms=500.0, hold_ms=0.0),
    "instant": Gate(threshold_db=-44.0, ratio=4.0, attack_ms=0.0, release_ms=0.0),
    "range inf": Gate(threshold_db=-42.0, range_db=math.inf, attack_ms=0.25, release_ms=8.0, hold_ms=1.0),
}


def between(n, channels, opener=10, closer=None, level=0.007):
    """``level`` (between -40 and -46 dB) in every frame, a frame at 0.5 at ``opener`` and a frame at 1e-4
    at ``closer``: the state is open from the one to the other with nothing in between deciding it."""
    x = np.full((n, channels), level, dtype=np.float32)
    if opener is not None:
        x[opener] = 0.5
    if closer is not None:
        x[closer] = 1e-4
    return x.reshape((n, channels) if channels == 2 else (n,))


def middle(gate):
    """The linear level half way (in dB) between the gate's two thresholds."""
    return 10.0 ** ((float(gate.threshold_db) - 0.5 * float(gate.hysteresis_db)) / 20.0)


def seam_signals(channels, gate):
    """Every length at a tile's edges as texture; a single opening frame at frame 0, at both sides of the
    first seam and at the last frame of a signal of three tiles and five frames; and an opener at frame 10,
    more than two tiles between ``gate``'s thresholds, one closing frame."""
    sig = [texture(n, channels, 40 + i) for i, n in enumerate(LENGTHS)]
    sig += [spike(N3, channels, at) for at in (0, TILE - 1, TILE, N3 - 1)]
    return sig + [between(N3, channels, 10, N3 - 100, middle(gate))]
