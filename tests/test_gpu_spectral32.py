"""The float32 spectral chain on the device at every FFT route and mask edge.

The chain (tilt step, band limit, power warp, partial stretch) runs in k_spectral<256,8192>
(runtime plan, small), k_spectral<512,20480> (runtime plan, big), k_spectral_ct (six
compile-time plans) and k_spec3 (band-pruned, 37 500 samples).  Each case here is one tiny
single-event preset (spectral32_cases.py) whose grain length and parameters pick the
kernel, the FFT plan (each register radix, Bluestein, odd lengths) and the mask or gather
edge; the route counter (msg_last_spec_routes) must name that kernel and no other, so a
length that silently fell to another route fails instead of passing vacuously.

Two bars, against the float64 oracle (oracle/msound_oracle.py):
  * the project's: micro_last, grain_last (relative RMS) and the audio (RMS) within 1e-5;
  * grain_last within spectral32_cases.grain_bar: 4 times the error e32 of a float32
    reference of the same chain (scipy float32 transforms, float64 masks and positions, fed
    the oracle's micro_last) against the oracle, never under 5e-7.  The factor 4 allows for
    the device's two-level table twiddles (about two more roundings per twiddle).  Measured
    on the device, two things that bar left out:
      - a tilt generator's grain has been through the tilt step's float32 transform pair as
        well; the float32 reference of that step (micro32) has its own error e32_micro, which
        the chain carries to the grain at most kappa = rms(micro) / rms(grain) times as
        large: the bar is 4 hypot(e32, kappa e32_micro), and micro_last itself is held to
        4 e32_micro.  (With the oracle-fed e32 alone, Noise burst on the Bluestein plans 1267
        and 2402 stood at 4.0 to 7.3 e32, and the DC-only grains of the 0.5 Hz cutoff, whose
        error is the mean of the tilt step's error over a mean that is ~1 / sqrt(n) of the
        rms, at up to 300 e32.)
      - on a Bluestein plan every transform is three inner transforms and three chirp
        products: the factor is 4 sqrt(3) there.
Every case prints its device errors, e32, e32_micro and the ratios
(profiles/spectral32_gpu_tests.txt).
"""
import numpy as np
import pytest

import spectral32_cases as S

pytestmark = pytest.mark.gpu

HARD_TOL = 1e-5          # the project's parity bar


@pytest.fixture(scope="module")
def msgpu():
    import msgpu as m
    m.render(m.merged(out_dur_s=0.05, er_cloud_on=False))   # initialise the engine
    assert "libmsgpu" in open("/proc/self/maps").read()     # the HIP library
    return m


def routes_of_last_batch():
    from msgpu.engine import default_engine
    return {k: v for k, v in default_engine(0).last_spec_routes().items() if v}


def rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.sqrt(np.mean((a - b) ** 2)))


def check_case(msgpu, monkeypatch, case):
    """Render one single-event case; its route, then micro_last, grain_last and the audio
    against the oracle, and grain_last against the float32 reference's own error."""
    for k in ("MSGPU_SPEC_CT", "MSGPU_SPEC3"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    p = case.params
    ref = S.reference(case)
    ev, micro, grain, e32 = ref.ev, ref.micro, ref.grain, ref.e32
    assert ev.n == case.n                                   # the oracle's plan gives the wanted length
    audio, meta = msgpu.render(p)
    got = routes_of_last_batch()
    assert got == {case.route: 1}, (case.id, got)
    ref_audio, ref_meta = S.O.render(p)
    assert np.array_equal(ref_meta["grain_last"], grain) and np.array_equal(ref_meta["micro_last"], micro)
    assert meta["micro_last"].shape == micro.shape and meta["grain_last"].shape == grain.shape
    m_err = S.rel_rms(meta["micro_last"], micro)
    g_err = S.rel_rms(meta["grain_last"], grain)
    a_err = rms(audio, ref_audio)
    bar, mbar = S.grain_bar(ref), S.micro_bar(ref)
    over = ("" if g_err <= bar else "  GRAIN OVER THE FLOAT32 BAR") + \
        ("" if not S.tilted(p) or m_err <= mbar else "  MICRO OVER THE FLOAT32 BAR")
    print(f"{case.id:<44} {case.route:<8} audio {a_err:.2e} micro {m_err:.2e} e32_micro {ref.e32_micro:.2e} "
          f"grain {g_err:.3e} e32 {e32:.3e} ratio {g_err / max(e32, 1e-30):6.2f} kappa {ref.kappa:8.3g} "
          f"bar {bar:.3e} of-bar {g_err / bar:4.2f}{over}")
    return case.id, m_err, g_err, a_err, bar, (mbar if S.tilted(p) else HARD_TOL)


def check_cases(msgpu, monkeypatch, cases):
    res = [check_case(msgpu, monkeypatch, c) for c in cases]       # print every figure, then assert
    hard = [r for r in res if not (r[1] <= HARD_TOL and r[2] <= HARD_TOL and r[3] <= HARD_TOL)]
    assert not hard, hard
    over = [r for r in res if not (r[2] <= r[4] and r[1] <= r[5])]
    assert not over, over


# ---- section 3: every FFT plan shape and routing boundary
@pytest.mark.parametrize("n", S.SWEEP_LENGTHS)
def test_length_sweep(msgpu, monkeypatch, n):
    """Resonant strike and Noise burst (tilt step) at stretch 1.3 under the default band
    limit: forward and inverse transforms of the length's plan (spectral32_cases.py lists
    the radix sequences; test_spectral32_host.py checks them).  40 000 and 16 386 samples
    are past the LDS engine: the float64 chain must take them and still match."""
    check_cases(msgpu, monkeypatch, S.sweep_cases(n))


# ---- section 4: mask and gather edges
@pytest.mark.parametrize("group", S.EDGE_GROUPS)
@pytest.mark.parametrize("tag", S.EDGE_TAGS)
def test_mask_and_gather_edges(msgpu, monkeypatch, tag, group):
    """cutoff: a hard cutoff exactly on a bin and 1e-6 Hz to either side of it (one bin kept
    or dropped is ~1 / sqrt(K) relative), a cutoff above Nyquist (clipped, all pass) and of
    0.5 Hz (clipped to 1 Hz, DC only), a roll-off that overshoots Nyquist and ones narrower
    than a bin (holding no bin, and one).  stretch: 0.5 and 2 (integer and half-integer
    sources, the j >= K - 1 edge), 4, 1 + 2e-9 (a stretch) and 1 + 5e-10 (none).  warp:
    powers 1 (identity gather), 0.8 and 1.25, alone and before stretch 0.7.  Lengths 4802,
    16 382 and 32 768 have more bins than one chunk of spectral_gather (8 x 256, 8 x 512):
    stretch 0.5 / warp 1.25 walk the chunks upwards, stretch 2 / warp 0.8 downwards."""
    check_cases(msgpu, monkeypatch, S.edge_cases(tag, group))


@pytest.mark.parametrize("n", S.TILT_LENGTHS)
def test_tilt_step(msgpu, monkeypatch, n):
    """noise_tilt 0, -12 and +6 dB / octave for Noise burst and Skewed transient: the
    generator's own transform pair, micro_last included.  Skewed transient at -12 is left
    out at 1267 and 4802 samples: the float32 reference of the tilt step is itself 5.0e-5 and
    9.6e-5 from the oracle there (device 5.2e-5 and 1.2e-4; spectral32_cases.TILT_DROPPED).
    At +6 and 4802 samples the audio is at 6.5e-6 (Noise burst) and 8.8e-6 (Skewed) with the
    grain at 4e-7: the tilt grows the samples to ~1e3 and the tanh clip saturates."""
    check_cases(msgpu, monkeypatch, S.tilt_cases(n))


# ---- section 5: layout and batching
@pytest.mark.parametrize("hot", [1500, 37500])
def test_hot_grains_at_odd_float_offsets(msgpu, monkeypatch, hot):
    """Odd-length grains ahead of the hot ones put these at odd float offsets: k_spectral_ct
    stores them one float at a time and load_real_segment shifts its quads (the odd grains
    themselves start at shifts 0, 3, 2, 1, 0).  k_spec3 reads and writes 8-byte pairs: it
    must decline the 37 500-sample grains, and the compile-time plan must take them."""
    for k in ("MSGPU_SPEC_CT", "MSGPU_SPEC3"):
        monkeypatch.delenv(k, raising=False)
    from msgpu.engine import default_engine
    p, odd, routes = S.odd_offset_preset(hot)
    plan = S.O.plan_render(p)
    assert [e.n for e in plan.events] == [odd] * 5 + [hot] * 4
    audio, meta = msgpu.render(p)
    assert routes_of_last_batch() == routes                 # no spec3 run among them
    events = default_engine(0).last_events(0)
    assert [(e.n, e.pool_off) for e in events] == [(odd, odd * i) for i in range(5)] + \
        [(hot, 5 * odd + hot * i) for i in range(4)]
    assert all(e.pool_off % 2 == 1 for e in events if e.n == hot)
    assert {e.pool_off % 4 for e in events if e.n == odd} == {0, 1, 2, 3}
    ref_audio, ref_meta = S.O.render(p)
    g_err = S.rel_rms(meta["grain_last"], ref_meta["grain_last"])
    m_err = S.rel_rms(meta["micro_last"], ref_meta["micro_last"])
    a_err = rms(audio, ref_audio)
    print(f"odd offsets, hot length {hot}: micro {m_err:.2e} grain {g_err:.3e} audio {a_err:.2e}")
    assert g_err <= HARD_TOL and m_err <= HARD_TOL and a_err <= HARD_TOL


def test_all_routes_in_one_batch(msgpu, monkeypatch):
    """Copy, small, big, a compile-time plan, k_spec3 and the float64 chain in one batch:
    the runtime kernels' launches are sized by the largest plan's LDS, whatever the grain.
    Every preset equals its own render alone, bit for bit."""
    for k in ("MSGPU_SPEC_CT", "MSGPU_SPEC3"):
        monkeypatch.delenv(k, raising=False)
    res = "Resonant strike"
    params = [S.preset(res, 1267, bandlimit_on=False, partial_stretch=1.0),            # copy
              S.preset("Noise burst", 1267, partial_stretch=1.3),                      # small (Bluestein, odd)
              S.preset(res, 16, partial_stretch=1.3),                                  # small, the shortest
              S.preset("Noise burst", 16382, partial_stretch=0.5),                     # big (Bluestein)
              S.preset(res, 39690, partial_stretch=1.3),                               # big, the longest
              S.preset("Noise burst", 1500, partial_stretch=1.3),                      # ct1500
              S.preset(res, 37500, S.SR384, S.UNFOLD384, partial_stretch=2.0),         # k_spec3
              S.preset("Noise burst", 40000, partial_stretch=1.3)]                     # float64 chain
    outs = msgpu.render_batch(params)
    assert routes_of_last_batch() == {"copy": 1, "small": 2, "big": 2, "ct1500": 1, "spec3": 1, "f64": 1}
    for i, p in enumerate(params):
        single, _ = msgpu.render(p)
        assert np.array_equal(single, outs[i]), i
        assert np.isfinite(single).all() and float(np.abs(single).max()) > 0.5
