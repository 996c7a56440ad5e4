"""What the compressor's host and device tests share: the signals, the option sets and the
tolerances of the host loop against the float64 reference (msgpu/dynamics.py, csrc/dynamics.h).

Tolerances.  The host's demand d is the curve rounded to the nearest unit of 2^-32 dB from the
library's own log2, the reference's from libm's; both are within 2^-40 dB of the curve, so the
two roundings differ by at most one unit where the curve lies that close to a tie.  A ramp
carries that difference unchanged and the maximum of two envelopes keeps it, so E agrees within
2 units per frame (one is the bound, the second is headroom for the knee's own float64 roundings).
A sample is x g: one float32 rounding of the gain (2 units of E move it by 2^-31 dB, nothing
beside 2^-24) and one of the product, so |y - y_ref| <= 1.01 2^-23 |y_ref| + 2^-149."""
import numpy as np

from msgpu.dynamics import Dynamics
from msgpu.edges import frames

SR = 48000
TILE = 4096
LENGTHS = [0, 1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
E_UNITS = 2                       # |E_host - E_ref| per frame
Y_REL, Y_ABS = 1.01 * 2.0 ** -23, 2.0 ** -149


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def hold_ms(hold_frames, sr=SR):
    """Milliseconds that are exactly ``hold_frames`` frames at ``sr`` Hz."""
    ms = hold_frames * 1000.0 / sr
    assert frames(ms, sr) == hold_frames
    return ms


def texture(n, channels, seed):
    """Sparse strikes over a quiet bed: noise at about -50 dBFS with bursts that reach from under
    the knee to full scale, the material a compressor is for."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, channels)) * 0.003
    for _ in range(max(1, n // 700)):
        at, ln = int(rng.integers(0, max(n, 1))), int(rng.integers(1, 400))
        seg = x[at:at + ln]
        seg += rng.standard_normal(seg.shape) * 10.0 ** (rng.uniform(-36.0, -3.0) / 20.0)
    return np.clip(x, -1.0, 1.0).astype(np.float32).reshape((n, channels) if channels == 2 else (n,))


def spike(n, channels, at):
    """A quiet bed under every threshold used here and one full-scale frame at ``at``."""
    x = np.full((n, channels), 1e-4, dtype=np.float32)
    if n:
        x[at] = -1.0 if at % 2 else 1.0
    return x.reshape((n, channels) if channels == 2 else (n,))


# the option sets: slow enough to cross every tile of 3 TILE + 5 frames from a 12 dB reduction
# (10 dB take 24000 frames), instant, hard and soft knee, a limiter's slope, makeup alone, holds
SLOW = Dynamics(threshold_db=-18.0, ratio=3.0, knee_db=6.0, attack_ms=500.0, release_ms=500.0)
OPTIONS = {
    "default": Dynamics(),
    "slow": SLOW,
    "instant": Dynamics(attack_ms=0.0, release_ms=0.0),
    "hard knee": Dynamics(threshold_db=-24.0, ratio=4.0, knee_db=0.0, attack_ms=1.0, release_ms=20.0),
    "wide knee": Dynamics(threshold_db=-30.0, ratio=2.0, knee_db=24.0, attack_ms=2.0, release_ms=60.0, makeup_db=4.5),
    "ratio inf": Dynamics(threshold_db=-20.0, ratio=float("inf"), knee_db=3.0, attack_ms=0.5, release_ms=80.0),
    "makeup alone": Dynamics(threshold_db=24.0, knee_db=0.0, makeup_db=-7.25),
    "hold 1": Dynamics(attack_ms=3.0, release_ms=40.0, hold_ms=hold_ms(1)),
    "hold 100": Dynamics(attack_ms=3.0, release_ms=40.0, hold_ms=hold_ms(100)),
    "hold 4096": Dynamics(attack_ms=3.0, release_ms=40.0, hold_ms=hold_ms(4096)),
}


def within(y, y_ref):
    """The largest |y - y_ref| over its allowance (<= 1 passes)."""
    y, y_ref = np.asarray(y, dtype=np.float64), np.asarray(y_ref, dtype=np.float64)
    if not y.size:
        return 0.0
    return float(np.max(np.abs(y - y_ref) / (Y_REL * np.abs(y_ref) + Y_ABS)))
