"""Cases of the float32 spectral chain's tests (test_gpu_spectral32.py on the device,
test_spectral32_host.py without one), the host restatement of the plan arithmetic that
routes a grain length to a kernel, and a float32 reference of the chain.

A case is one tiny preset: one event (``event_process="Single"``), no ER cloud, no space
IR, 0.05 s.  Its grain length n comes from ``micro_ms = (n + 0.01) * 1000 / design_sr``
(grain floor 16, MS:221); ``route`` names the kernel the length and the parameters must
reach (msgpu._lib.SPEC_ROUTES), ``env`` the switches the render needs.

The routes are restated here from csrc/fftplan.h (factor), csrc/msgpu.hip (real_plan),
csrc/launch.h (the kernels' limits) and csrc/spec3.h / k_spec3.hip (k_spec3's
eligibility), so the case list can be checked without a device; on the device the route
counter (msg_last_spec_routes) confirms every one of them.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from oracle import msound_oracle as O

Case = namedtuple("Case", "id n route env params")

SR48, UNFOLD48 = 48000, 25.0            # design rate 1.2 MHz: n = 1500 at the factory micro_ms
SR384, UNFOLD384 = 384000, 100.0        # design rate capped at 30 MHz (MS:597): n = 37500 (C3)
CT_LENGTHS = {37500: "ct37500", 30000: "ct30000", 2400: "ct2400", 1920: "ct1920", 1500: "ct1500", 480: "ct480"}


# ---------------------------------------------------------------------------
# plan arithmetic (fftplan::factor, real_plan, stage_event_records)
# ---------------------------------------------------------------------------
RADICES = (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 15, 16, 20, 25)
TW_LO, LDS_MAX, SMALL_BYTES, M_SMALL, M_BIG = 128, 163840, 65536, 8192, 20480


def factor(m):
    """fftplan::factor: the radix sequence (sorted, as the merge loop leaves it), or None."""
    r, a = m, {}
    for q in (2, 3, 5, 7):
        a[q] = 0
        while r % q == 0:
            r //= q
            a[q] += 1
    if r != 1:
        return None
    rad = [25] * (a[5] // 2) + [5] * (a[5] % 2) + [9] * (a[3] // 2) + [3] * (a[3] % 2) + [7] * a[7]
    rad += [16] * (a[2] // 4) + {0: [], 1: [2], 2: [4], 3: [8]}[a[2] % 4]
    merged = True
    while merged:
        merged = False
        rad.sort()
        for i in range(len(rad)):
            for j in range(i + 1, len(rad)):
                if rad[i] * rad[j] in RADICES:
                    rad[i] *= rad[j]
                    del rad[j]
                    merged = True
                    break
            if merged:
                break
    return rad


def real_plan(n):
    """real_plan's shape for n samples: dict(even, m, size, blue, rad, lds_bytes)."""
    even = n % 2 == 0
    m = n // 2 if even else n
    rad = factor(m)
    blue = rad is None
    size = m
    if blue:
        size = 1
        while size < 2 * m - 1:
            size *= 2
        rad = factor(size)
    tw_hi = (size + TW_LO - 1) // TW_LO
    lds_c = (max(m + 1 if even else m, size) + 15) & ~15
    rt_hi = (m + 1 + TW_LO - 1) // TW_LO
    lds = (lds_c + TW_LO + tw_hi + ((TW_LO + rt_hi) if even else 0)) * 8
    return dict(even=even, m=m, size=size, blue=blue, rad=rad, lds_bytes=lds)


def runtime_route(n):
    """The runtime-plan kernel of an n-sample grain, "f64" beyond the LDS engine."""
    p = real_plan(n)
    if p["lds_bytes"] <= SMALL_BYTES and p["size"] <= M_SMALL:
        return "small"
    if p["lds_bytes"] <= LDS_MAX and p["size"] <= M_BIG:
        return "big"
    return "f64"


def _first_bin(val, x, K, strict):
    g = math.floor(x / val)
    k = 0 if g < 0 else (K if g > K else int(g))
    if strict:
        while k > 0 and (k - 1) * val > x:
            k -= 1
        while k < K and k * val <= x:
            k += 1
    else:
        while k > 0 and (k - 1) * val >= x:
            k -= 1
        while k < K and k * val < x:
            k += 1
    return k


def spec3_eligible(p, ev):
    """spec3_eligible for an event at an even float offset (a single-event preset)."""
    M, BUF = 18750, 19014                # Spec3P18750: BUF = (M - 1) + ((M - 1) / 750) * 11 + 1
    if ev.n != 2 * M or p["gen_mode"] != "Resonant strike" or p["nl_warp_on"] or not p["bandlimit_on"]:
        return False
    K, sr = ev.n // 2 + 1, ev.gen_sr
    nyq = 0.5 * sr
    c = min(max(ev.cutoff_out * ev.ufac, 1.0), nyq)
    r = max(0.0, float(p["bandlimit_roll_hz"]))
    val = 1.0 / (ev.n * (1.0 / sr))
    lim = c if r <= 0 else min(nyq, c + r)
    kz = _first_bin(val, lim, K, True)
    stretch = abs(ev.stretch - 1.0) >= 1e-9
    ky = kz
    if stretch:
        e = math.ceil(kz * max(1e-12, ev.stretch)) + 2.0
        ky = int(e) if e < K else K
    if kz > ky:
        return False
    r16 = lambda v: (v + 15) & ~15
    if ky <= M // 2:
        return r16(kz) + 2 * r16(ky) + 16 <= BUF and 2 * r16(kz) <= BUF
    return not (2 * r16(kz) > BUF or ky > BUF or (stretch and ev.stretch <= 1.0))


def the_event(p):
    plan = O.plan_render(p)
    assert len(plan.events) == 1
    return plan.events[0]


def has_ops(p, ev):
    """specshare::spec_ops != 0 for a float32-chain preset."""
    return (p["gen_mode"] in ("Noise burst", "Skewed transient") or (p["bandlimit_on"] and ev.n >= 8) or
            (p["nl_warp_on"] and ev.n >= 16) or (ev.n >= 16 and abs(ev.stretch - 1.0) >= 1e-9))


def predicted_route(case):
    """The route stage_event_records gives the case's one event (restated)."""
    p, ev = case.params, the_event(case.params)
    if not has_ops(p, ev):
        return "copy"
    use_ct = case.env.get("MSGPU_SPEC_CT", "1") != "0"
    use_s3 = use_ct and case.env.get("MSGPU_SPEC3", "1") != "0"
    if use_ct and ev.n in CT_LENGTHS:
        return "spec3" if use_s3 and spec3_eligible(p, ev) else CT_LENGTHS[ev.n]
    return runtime_route(ev.n)


# ---------------------------------------------------------------------------
# presets
# ---------------------------------------------------------------------------
def preset(gen, n, base_sr=SR48, unfold=UNFOLD48, **kw):
    import msgpu
    design = O.design_sr(base_sr, unfold)
    p = msgpu.merged(gen_mode=gen, event_process="Single", er_cloud_on=False, space_ir_on=False, out_dur_s=0.05,
                     base_sr=base_sr, time_unfold=unfold, micro_ms=(n + 0.01) * 1000.0 / design, seed=4000 + n % 997)
    p.update(kw)
    p["_ir_audio"] = None
    p["_img_gray"] = None
    return p


GEN_TAG = {"Resonant strike": "res", "Noise burst": "noise", "Skewed transient": "skew"}

# ---- section 3: the length sweep (stretch 1.3, default band limit: forward and inverse run)
# (n, radix sequence of the half-length) / (n, Bluestein inner size, None for a radix-only odd length)
SINGLE_PASS = [(16, [8]), (18, [9]), (20, [10]), (24, [12]), (28, [2, 7]), (30, [15]), (32, [16]), (40, [20]),
               (50, [25])]
MIXED_PASS = [(98, [7, 7]), (162, [9, 9]), (1024, [2, 16, 16]), (1458, [9, 9, 9]), (2058, [3, 7, 7, 7]),
              (4802, [7, 7, 7, 7]), (8192, [16, 16, 16]), (32768, [4, 16, 16, 16])]
# 16 382 stands for the 16 386 first thought of: its half-length 8193 needs 2 m - 1 = 16 385
# points, one over 16 384, so its inner size is 32 768 and it leaves the float32 engine
# (checked below as a float64 boundary); 16 382 = 2 x 8191 (prime) has inner size 16 384
BLUE_EVEN = [(34, 64), (402, 512), (2402, 4096), (4098, 8192), (16382, 16384)]
ODD = [(17, 64), (21, None), (2401, None), (1267, 4096), (8191, 16384), (19683, None)]
SWEEP_ROUTES = {16: "small", 18: "small", 20: "small", 24: "small", 28: "small", 30: "small", 32: "small",
                40: "small", 50: "small", 98: "small", 162: "small", 1024: "small", 1458: "small", 2058: "small",
                4802: "small", 8192: "small", 32768: "big", 34: "small", 402: "small", 2402: "small", 4098: "big",
                16382: "big", 17: "small", 21: "small", 2401: "small", 1267: "small", 8191: "big", 19683: "big",
                # routing boundaries: the last small and first big radix-only even lengths, the
                # last lengths of the big kernel, and the first ones past the float32 engine
                15552: "small", 15680: "big", 39690: "big", 40000: "f64", 16386: "f64"}
SWEEP_LENGTHS = sorted(SWEEP_ROUTES)


def sweep_cases(n):
    return [Case(f"sweep-{n}-{GEN_TAG[g]}", n, SWEEP_ROUTES[n], {}, preset(g, n, partial_stretch=1.3))
            for g in ("Resonant strike", "Noise burst")]


# ---- section 4: mask and gather edges
# (tag, n, base_sr, unfold, generator, env, bin of the hard cutoff or None)
EDGE_CONFIGS = [
    ("1500ct", 1500, SR48, UNFOLD48, "Noise burst", {"MSGPU_SPEC_CT": "1"}, 500),     # 16 kHz x 25 = bin 500
    ("1500rt", 1500, SR48, UNFOLD48, "Noise burst", {"MSGPU_SPEC_CT": "0"}, 500),
    ("1267", 1267, SR48, UNFOLD48, "Noise burst", {}, None),
    ("2402", 2402, SR48, UNFOLD48, "Noise burst", {}, None),
    ("4802", 4802, SR48, UNFOLD48, "Noise burst", {}, None),                           # K = 2402 > 8 x 256: two chunks
    ("16382", 16382, SR48, UNFOLD48, "Noise burst", {}, None),                         # K = 8192 > 8 x 512: two chunks
    ("32768", 32768, SR48, UNFOLD48, "Noise burst", {}, None),                         # K = 16385: five chunks
    # 37 500 at the design-rate cap.  k_spec3 takes no tilt generator, so Noise burst runs the
    # compile-time plan under either switch; the Resonant strike (C3's generator: a decaying
    # white excitation under the ring, so a bin at a hard edge still weighs ~1e-3) reaches
    # k_spec3 and its host-side band kb / kz / ky
    ("37500noise-s3on", 37500, SR384, UNFOLD384, "Noise burst", {"MSGPU_SPEC3": "1"}, 2250),   # 18 kHz x 100 = bin 2250
    ("37500noise-s3off", 37500, SR384, UNFOLD384, "Noise burst", {"MSGPU_SPEC3": "0"}, 2250),
    ("37500res-s3on", 37500, SR384, UNFOLD384, "Resonant strike", {"MSGPU_SPEC3": "1"}, 2250),
    ("37500res-s3off", 37500, SR384, UNFOLD384, "Resonant strike", {"MSGPU_SPEC3": "0"}, 2250),
]
EDGE_TAGS = [c[0] for c in EDGE_CONFIGS]
EDGE_GROUPS = ("cutoff", "stretch", "warp")


def exact_bin(n, sr, ufac, kc):
    """(k, cutoff_out) with cutoff_out * ufac == rfftfreq(n, 1 / sr)[k] in float64, the
    first such k from kc up."""
    f = O.bin_freqs(n, float(sr))
    for k in range(kc, len(f)):
        c = float(f[k]) / ufac
        if c * ufac == float(f[k]):
            return k, c
    raise AssertionError("no exactly representable bin")


def edge_cases(tag, group):
    _, n, base_sr, unfold, gen, env, kc = next(c for c in EDGE_CONFIGS if c[0] == tag)
    sr = O.design_sr(base_sr, unfold)
    K, nyq = n // 2 + 1, 0.5 * sr
    val = 1.0 / (n * (1.0 / sr))          # the bin spacing as rfftfreq forms it
    out = []

    def add(name, **kw):
        c = Case(f"{tag}-{group}-{name}", n, None, dict(env), preset(gen, n, base_sr, unfold, **kw))
        out.append(c._replace(route=predicted_route(c)))

    if group == "cutoff":
        k, c0 = exact_bin(n, sr, unfold, kc if kc is not None else int(round(0.4 * (K - 1))))
        fk = c0 * unfold
        add("on-bin", bandlimit_roll_hz=0.0, bandlimit_out_hz=c0)
        add("under-bin", bandlimit_roll_hz=0.0, bandlimit_out_hz=(fk - 1e-6) / unfold)
        add("over-bin", bandlimit_roll_hz=0.0, bandlimit_out_hz=(fk + 1e-6) / unfold)
        add("above-nyquist", bandlimit_out_hz=1.5 * nyq / unfold)                    # clipped: everything passes
        add("half-hertz", bandlimit_roll_hz=0.0, bandlimit_out_hz=0.5 / unfold)      # clipped to 1 Hz: DC only
        add("roll-past-nyquist", bandlimit_out_hz=0.9 * nyq / unfold, bandlimit_roll_hz=0.2 * nyq)
        add("roll-between-bins", bandlimit_out_hz=(k + 0.35) * val / unfold, bandlimit_roll_hz=0.3 * val)
        add("roll-holds-one-bin", bandlimit_out_hz=(k - 0.1) * val / unfold, bandlimit_roll_hz=0.3 * val)
    elif group == "stretch":
        for name, st in (("0.5", 0.5), ("2", 2.0), ("4", 4.0), ("1+2e-9", 1.0 + 2e-9), ("1+5e-10", 1.0 + 5e-10)):
            add(name, partial_stretch=st)
    elif group == "warp":
        for pw in (1.0, 0.8, 1.25):
            add(f"{pw}", nl_warp_on=True, nl_warp_power=pw, partial_stretch=1.0)
            add(f"{pw}-stretch0.7", nl_warp_on=True, nl_warp_power=pw, partial_stretch=0.7)
    else:
        raise KeyError(group)
    return out


# tilt step: the generator's own rfft / irfft pair (MS:224-233), micro_last included
TILT_LENGTHS = (16, 1267, 4802)
# Skewed transient at -12 dB / octave is left out at 1267 and 4802 samples: x = diff(max(0, w))
# of a w that is nearly its lowest bins divides float32's rounding of w by |diff w| / |w| ~ 2 pi / n.
# The float32 reference of the tilt step (micro32 below, pocketfft) is itself 5.0e-5 and 9.6e-5
# from the oracle's micro_last there, and the device 5.2e-5 and 1.2e-4: no float32 transform
# holds 1e-5 (test_spectral32_host.py keeps the two figures checked)
TILT_DROPPED = ((1267, "Skewed transient", -12.0), (4802, "Skewed transient", -12.0))


def tilt_case(n, g, t):
    # seed: at 16 samples a -12 dB/octave noise is nearly its DC term, and where that is negative
    # the skewed transient's max(0, w) is zero throughout (nothing to compare): a seed where it is not
    return Case(f"tilt-{n}-{GEN_TAG[g]}-{t:+g}", n, "small", {},
                preset(g, n, noise_tilt=t, partial_stretch=1.3, seed=5001 + n))


def tilt_cases(n):
    return [tilt_case(n, g, t) for g in ("Noise burst", "Skewed transient") for t in (0.0, -12.0, 6.0)
            if (n, g, t) not in TILT_DROPPED]


# ---- section 5: hot grains at odd float offsets of the pool
def odd_offset_preset(hot):
    """A Poisson preset whose bp_unfold lane shortens the grains before 20 ms: five
    odd-length grains, then four hot ones, all at odd float offsets of the pool."""
    import msgpu
    common = dict(event_process="Poisson", grains_per_sec=200.0, er_cloud_on=False, space_ir_on=False,
                  out_dur_s=0.05, seed=7000, _ir_audio=None, _img_gray=None)
    if hot == 1500:      # 48 kHz x 24.99 -> 1499 samples (prime: Bluestein, small), x 25 -> 1500
        p = msgpu.merged(common, gen_mode="Noise burst", base_sr=48000, time_unfold=25.0, partial_stretch=1.3,
                         bp_unfold="0:24.99, 0.02:24.99, 0.0201:25, 1:25")
        return p, 1499, {"small": 5, "ct1500": 4}
    # 384 kHz x 17.06 -> 8189 samples (19 x 431: Bluestein through 16 384, big), x 100 -> 37 500
    p = msgpu.merged(common, gen_mode="Resonant strike", base_sr=384000, time_unfold=100.0, partial_stretch=2.0,
                     bp_unfold="0:17.06, 0.02:17.06, 0.0201:100, 1:100")
    return p, 8189, {"big": 5, "ct37500": 4}


def all_single_cases():
    for n in SWEEP_LENGTHS:
        yield from sweep_cases(n)
    for tag in EDGE_TAGS:
        for group in EDGE_GROUPS:
            yield from edge_cases(tag, group)
    for n in TILT_LENGTHS:
        yield from tilt_cases(n)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.sqrt(np.mean((a - ref) ** 2)) / max(1e-30, np.sqrt(np.mean(ref ** 2))))


def _interp32(k_in, X):
    """np.interp of complex64 bins at float64 positions, zero outside, back to complex64."""
    k = np.arange(X.size, dtype=np.float64)
    re = np.interp(k_in, k, X.real, left=0.0, right=0.0)
    im = np.interp(k_in, k, X.imag, left=0.0, right=0.0)
    return (re + 1j * im).astype(np.complex64)


def chain32(p, ev, micro):
    """The oracle's lowpass_fft, fft_warp_power and fft_partial_stretch (MS:39-59, 103-128)
    on float32 data with scipy's float32 transforms; the masks and the interpolation
    positions stay in float64.  What a correct float32 chain can be expected to reach."""
    import scipy.fft as sfft
    x = np.asarray(micro, np.float64).astype(np.float32)
    n, sr = x.size, float(ev.gen_sr)
    if p["bandlimit_on"] and n >= 8:
        nyq = 0.5 * sr
        c = float(np.clip(ev.cutoff_out * ev.ufac, 1.0, nyq))
        r = float(max(0.0, p["bandlimit_roll_hz"]))
        f = O.bin_freqs(n, sr)
        w = np.ones(f.size)
        if r <= 0:
            w[f > c] = 0.0
        else:
            f1 = min(nyq, c + r)
            w[f > f1] = 0.0
            band = (f >= c) & (f <= f1)
            w[band] *= 0.5 * (1.0 + np.cos(np.pi * (f[band] - c) / max(1e-12, f1 - c)))
        x = sfft.irfft(sfft.rfft(x) * w.astype(np.float32), n=n)
    if p["nl_warp_on"] and n >= 16:
        X = sfft.rfft(x)
        k = np.arange(X.size, dtype=np.float64)
        kmax = max(1.0, k[-1])
        x = sfft.irfft(_interp32(np.power(k / kmax, 1.0 / max(1e-6, float(p["nl_warp_power"]))) * kmax, X), n=n)
    if n >= 16 and abs(float(ev.stretch) - 1.0) >= 1e-9:
        X = sfft.rfft(x)
        k = np.arange(X.size, dtype=np.float64)
        x = sfft.irfft(_interp32(k / max(1e-12, float(ev.stretch)), X), n=n)
    assert x.dtype == np.float32
    return x.astype(np.float64)


def micro32(p, ev):
    """gen_basic's Noise burst / Skewed transient (MS:224-255, 265-268) with the tilt step's
    transform pair in float32 (scipy); the normals, the tilt weights, the envelope and the
    fade are formed in float64 and rounded once, as chain32's masks are."""
    import scipy.fft as sfft
    n, sr, mm = ev.n, ev.gen_sr, float(p["micro_ms"])
    w = np.random.default_rng(int(p["seed"]) + ev.index).standard_normal(n).astype(np.float32)
    f = O.bin_freqs(n, sr)
    if f.size > 1:
        f[0] = f[1]
    alpha = math.log(10.0 ** (float(p["noise_tilt"]) / 20.0), 2.0)
    w = sfft.irfft(sfft.rfft(w) * ((f / max(1e-12, f[1])) ** alpha).astype(np.float32), n=n)
    t = np.arange(n, dtype=np.float64) / sr
    if p["gen_mode"] == "Skewed transient":
        w = np.maximum(np.float32(0.0), w)
        w = np.diff(w, prepend=w[0])
    tau = max(1e-6, (mm / 1000.0) * (0.2 if p["gen_mode"] == "Skewed transient" else 0.25))
    x = w * (np.exp(-t / tau) * O.edge_fade(n)).astype(np.float32)
    assert x.dtype == np.float32
    return x.astype(np.float64)


def tilted(p):
    return p["gen_mode"] in ("Noise burst", "Skewed transient")


# What grain_last is held to besides the project's 1e-5: F32_FACTOR times the float32
# reference's own error, on a Bluestein plan times sqrt(3) (each device transform is three
# inner power-of-two transforms of 2 to 4 times the length and three products with rounded
# chirps), never under F32_FLOOR.  For a tilt generator the device's grain has been through a
# second float32 transform pair, the tilt step's, which a reference fed the oracle's
# micro_last never sees: its error (micro32 against the oracle, e32_micro) reaches the grain
# through a chain that is linear -- masks of weight at most 1, and gathers that treat an
# error as they treat the grain -- so relative to the grain it is about kappa = rms(micro) /
# rms(grain) times as large (for a DC-only grain, the mean of the error over the mean of
# the grain: Cauchy-Schwarz), and the two add in quadrature.
F32_FACTOR, F32_FLOOR = 4.0, 5e-7
Ref = namedtuple("Ref", "ev micro grain e32 e32_micro kappa factor")


def grain_bar(ref):
    return max(ref.factor * math.hypot(ref.e32, ref.kappa * ref.e32_micro), F32_FLOOR)


def micro_bar(ref):
    return max(ref.factor * ref.e32_micro, F32_FLOOR)


_REF = {}


def reference(case):
    """Ref of a single-event case, computed once: the oracle's event, generator output and
    grain, and the float32 references' errors against them."""
    if case.id not in _REF:
        p = case.params
        ev = the_event(p)
        micro, _ = O.synth_micro(p, ev)
        grain = O.spectral_chain(p, ev, micro.copy())
        rms = lambda v: float(np.sqrt(np.mean(np.asarray(v, np.float64) ** 2)))
        blue = ev.n not in CT_LENGTHS and real_plan(ev.n)["blue"]
        _REF[case.id] = Ref(ev, micro, grain, rel_rms(chain32(p, ev, micro), grain),
                            rel_rms(micro32(p, ev), micro) if tilted(p) else 0.0,
                            rms(micro) / max(1e-300, rms(grain)), F32_FACTOR * (math.sqrt(3.0) if blue else 1.0))
    return _REF[case.id]
