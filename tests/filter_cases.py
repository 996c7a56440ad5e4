"""What the tests of the delivery filter share (tests/test_filter_host.py, tests/test_gpu_filter.py):
the definition of csrc/filter.h restated, the designs restated in extended precision, the cascades,
signals and bars.  No device is touched here.

The definition (csrc/filter.h): a cascade is 1 .. 8 second-order sections b0 b1 b2 a0 a1 a2, float64,
a0 == 1; each runs in transposed direct form II with two float64 state words per channel; sections in
series, channels independent, zero state at the signal's own first frame; the float64 output is rounded
once to float32; REVERSE runs the recurrence from the last frame to the first.  The reference is
scipy.signal.sosfilt in float64 on the same float32 input.

The bar against it: with e32 = rms(float32(ref) - ref), rms(out - ref) <= 2 e32.  A correct float64
recurrence adds nothing visible to the one output rounding, and two independent errors of at most e32
add to sqrt(2) e32.
"""
import numpy as np
from scipy.signal import butter, sosfilt

from msgpu.filter import TILE, Filter

T = TILE
assert T == 4096
R = np.longdouble
PI = 4 * np.arctan(R(1))

# ---- the designs, restated in extended precision -----------------------------------------------------
BUTTER_ORDERS = (1, 2, 3, 4, 8)
BUTTER_FREQS = (20.0, 18000.0)
BUTTER_RATES = (44100, 48000, 384000)
BUTTER_CASES = [(n, f, kind, sr) for kind in ("highpass", "lowpass") for n in BUTTER_ORDERS for f in BUTTER_FREQS
                for sr in BUTTER_RATES]
IMPULSE_FRAMES = 1 << 16


def butter_extended(order, f, kind, sr):
    """The Butterworth design by the bilinear transform with pre-warping, written from the poles: the
    analogue prototype's pole p = -sin t + j cos t, t = pi (2 k + 1) / (2 order), scaled by K = tan(pi f / sr)
    maps to z = (1 + K p) / (1 - K p), for both kinds; a pair gives a1 = -2 Re z, a2 = |z|^2 and
    the numerator g (1, +-2, 1) with unit gain at DC or at Nyquist.  Extended precision, rounded once."""
    K = np.tan(PI * R(f) / R(sr))
    sign = 1 if kind == "lowpass" else -1
    rows = []
    for k in range(order // 2):
        t = PI * (2 * k + 1) / (2 * R(order))
        re, im = -np.sin(t), np.cos(t)                 # |p| = 1: the high-pass's K / p is K conj(p), the same pair
        den = (1 - K * re) ** 2 + (K * im) ** 2        # z = (1 + K p) / (1 - K p)
        zr = ((1 + K * re) * (1 - K * re) - (K * im) ** 2) / den
        zi = (2 * K * im) / den
        a1, a2 = -2 * zr, zr * zr + zi * zi
        g = (K * K if kind == "lowpass" else 1) / den  # |1 -+ z|^2 / 4, without the cancellation
        rows.append([g, sign * 2 * g, g, R(1), a1, a2])
    if order % 2:
        z = (1 - K) / (1 + K)                           # the real pole at s = -1: both kinds
        g = (K if kind == "lowpass" else 1) / (1 + K)   # (1 -+ z) / 2
        rows.append([g, sign * g, R(0), R(1), -z, R(0)])
    return np.array([[float(c) for c in r] for r in rows], dtype=np.float64)


def impulse_response(sos, n=IMPULSE_FRAMES):
    x = np.zeros(n)
    x[0] = 1.0
    return sosfilt(np.asarray(sos, dtype=np.float64), x)


def rms(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.sqrt(np.mean(v * v))) if v.size else 0.0


def design_distances(order, f, kind, sr):
    """(the design under test, scipy's own) as the relative RMS distance of the float64 sosfilt impulse
    response over 2^16 frames from that of the extended-precision design.  Section order and pairing
    differ between the three; the responses do not care."""
    ref = impulse_response(butter_extended(order, f, kind, sr))
    mine = impulse_response(Filter(**{kind: (f, order)}).design(sr))
    theirs = impulse_response(butter(order, f, kind, fs=sr, output="sos"))
    return rms(mine - ref) / rms(ref), rms(theirs - ref) / rms(ref)


# The bar: the design under test may lie at most DESIGN_FACTOR times as far from the extended-precision
# design as scipy's does, both being float64 roundings of the same design.  MEASURED_SCIPY holds
# scipy's distances as design_distances measured them over BUTTER_CASES (relative RMS of the impulse
# response); the test measures both again and prints them.  Where scipy measures 0 the bar is 0.
DESIGN_FACTOR = 4.0
MEASURED_SCIPY = {
    # (order, f, kind): scipy's distance at 44.1, 48 and 384 kHz; the design under test measured 0 in
    # every case (it evaluates the formulas in extended precision too and rounds to the same float64)
    (1, 20.0, 'highpass'): (1.11e-16, 1.10e-15, 3.07e-15),
    (1, 18000.0, 'highpass'): (5.80e-17, 0.00e+00, 1.50e-16),
    (2, 20.0, 'highpass'): (2.10e-13, 2.39e-13, 5.55e-12),
    (2, 18000.0, 'highpass'): (2.28e-16, 1.80e-16, 4.94e-16),
    (3, 20.0, 'highpass'): (3.15e-13, 3.69e-13, 6.16e-12),
    (3, 18000.0, 'highpass'): (5.79e-16, 2.98e-16, 8.89e-16),
    (4, 20.0, 'highpass'): (5.91e-13, 4.66e-13, 9.46e-12),
    (4, 18000.0, 'highpass'): (3.49e-16, 4.92e-16, 8.20e-16),
    (8, 20.0, 'highpass'): (1.06e-12, 8.48e-13, 2.02e-11),
    (8, 18000.0, 'highpass'): (7.01e-16, 1.21e-15, 1.89e-15),
    (1, 20.0, 'lowpass'): (0.00e+00, 3.09e-14, 2.39e-13),
    (1, 18000.0, 'lowpass'): (1.46e-16, 1.48e-16, 4.01e-16),
    (2, 20.0, 'lowpass'): (1.22e-11, 1.41e-11, 8.80e-10),
    (2, 18000.0, 'lowpass'): (8.63e-17, 2.00e-16, 1.49e-15),
    (3, 20.0, 'lowpass'): (1.09e-12, 1.07e-12, 1.09e-09),
    (3, 18000.0, 'lowpass'): (3.03e-16, 4.99e-16, 6.36e-16),
    (4, 20.0, 'lowpass'): (1.53e-11, 1.41e-11, 8.60e-10),
    (4, 18000.0, 'lowpass'): (3.44e-16, 4.00e-16, 1.84e-15),
    (8, 20.0, 'lowpass'): (3.55e-11, 3.58e-12, 1.03e-09),
    (8, 18000.0, 'lowpass'): (5.00e-16, 4.51e-16, 9.24e-15),
}


def cookbook_reference(kind, f, gain_db, q, sr):
    """The Audio EQ Cookbook section in its Q form in float64 NumPy, normalised to a0 = 1."""
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * np.pi * f / sr
    cs, alpha = np.cos(w0), np.sin(w0) / (2.0 * q)
    if kind == "peak":
        b = [1 + alpha * A, -2 * cs, 1 - alpha * A]
        a = [1 + alpha / A, -2 * cs, 1 - alpha / A]
    elif kind == "low_shelf":
        r = 2 * np.sqrt(A) * alpha
        b = [A * ((A + 1) - (A - 1) * cs + r), 2 * A * ((A - 1) - (A + 1) * cs), A * ((A + 1) - (A - 1) * cs - r)]
        a = [(A + 1) + (A - 1) * cs + r, -2 * ((A - 1) + (A + 1) * cs), (A + 1) + (A - 1) * cs - r]
    else:
        r = 2 * np.sqrt(A) * alpha
        b = [A * ((A + 1) + (A - 1) * cs + r), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - r)]
        a = [(A + 1) - (A - 1) * cs + r, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - r]
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], 1.0, a[1] / a[0], a[2] / a[0]])


def gain_db_at(sos, f, sr):
    """|H(e^jw)| of a cascade in dB at f Hz, evaluated in extended precision."""
    w = 2 * PI * R(f) / R(sr)
    c1, s1, c2, s2 = np.cos(w), np.sin(w), np.cos(2 * w), np.sin(2 * w)
    h = R(1)
    for b0, b1, b2, a0, a1, a2 in np.asarray(sos, dtype=np.float64):
        num = (R(b0) + R(b1) * c1 + R(b2) * c2) ** 2 + (R(b1) * s1 + R(b2) * s2) ** 2
        den = (R(a0) + R(a1) * c1 + R(a2) * c2) ** 2 + (R(a1) * s1 + R(a2) * s2) ** 2
        h = h * num / den
    return float(10 * np.log10(h))


# ---- the cascades of the sosfilt comparisons -----------------------------------------------------------
EIGHT = Filter(highpass=(20, 4), low_shelf=(120, 3.0, 0.7), peaks=[(400, -4.0, 1.4), (3000, 2.5, 2.0)],
               high_shelf=(9000, -2.0, 0.7), lowpass=(18000, 4))
# name -> (Filter, rate): 1, 2, 3 and 8 sections; the device's option sets are the first four
FILTERS = {
    "hp2 20 Hz @ 48k": (Filter(highpass=(20, 2)), 48000),
    "hp4 20 Hz @ 384k": (Filter(highpass=(20, 4)), 384000),
    "eight sections @ 48k": (EIGHT, 48000),
    "first order @ 48k": (Filter(highpass=(30, 1)), 48000),
    "three sections @ 44.1k": (Filter(highpass=(25, 3), peaks=[(1000, 6.0, 4.0)]), 44100),
}
DEVICE_SETS = ("hp2 20 Hz @ 48k", "hp4 20 Hz @ 384k", "eight sections @ 48k", "first order @ 48k")
assert [FILTERS[k][0].n_sections() for k in FILTERS] == [1, 2, 8, 1, 3]

LENGTHS = (0, 1, 2, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5)
N_LONG = 3 * T + 5
IMPULSES = (0, 15, 16, T - 1, T, N_LONG - 1)       # the chunk, wave and tile seams, and the last frame
N_COND = 40000                                       # the conditioning case: DC 0.5 + 1e-3 noise


def noise(n, channels, seed, amp=0.25):
    rng = np.random.default_rng(seed)
    return (amp * rng.standard_normal((n, 2) if channels == 2 else n)).astype(np.float32)


def conditioning(channels, seed=7):
    """DC 0.5 + 1e-3 noise over 40 000 frames: at 384 kHz the 20 Hz high-pass keeps its states far above
    its output, and a tile scan with float64 matrix powers is 6e-7 relative RMS off."""
    rng = np.random.default_rng(seed)
    return (0.5 + 1e-3 * rng.standard_normal((N_COND, 2) if channels == 2 else N_COND)).astype(np.float32)


def impulse(n, at, channels):
    x = np.zeros((n, 2) if channels == 2 else n, dtype=np.float32)
    x[at] = 1.0
    return x


def signals(channels):
    """[(name, signal)]: noise of every length, the impulses, the conditioning case; computed per call,
    seeded, so two calls give the same arrays."""
    out = [(f"noise n={n}", noise(n, channels, 100 + i)) for i, n in enumerate(LENGTHS)]
    out += [(f"impulse at {at}", impulse(N_LONG, at, channels)) for at in IMPULSES]
    out.append(("conditioning", conditioning(channels)))
    return out


def e32(ref):
    """rms(float32(ref) - ref): what the one output rounding costs."""
    ref = np.asarray(ref, dtype=np.float64)
    return rms(ref.astype(np.float32).astype(np.float64) - ref)


def check_against(name, out, ref):
    """rms(out - ref) <= 2 e32(ref); returns (error, e32) for the caller's log."""
    assert out.dtype == np.float32 and out.shape == ref.shape, name
    err, bar = rms(out.astype(np.float64) - ref), e32(ref)
    assert err <= 2.0 * bar, f"{name}: rms error {err:.3e} over 2 x e32 = {2 * bar:.3e}"
    return err, bar


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
