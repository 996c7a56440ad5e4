"""Host-only companion of test_gpu_spectral32.py: the case list is what it claims to be,
without a device.

For every single-event case (spectral32_cases.py) the oracle's plan gives exactly the
wanted grain length, the restated plan arithmetic sends it to the route the case names,
and the float32 references of the chain and of the tilt step (scipy float32 transforms,
float64 masks and positions) stay within the project's 1e-5 of the float64 oracle -- so a
case the device misses is the device's fault, not an ill-conditioned case.  A case the
references themselves cannot hold is not in the list (TILT_DROPPED).
"""
import numpy as np
import pytest

import spectral32_cases as S

HARD_TOL = 1e-5


def test_sweep_plans_are_the_tabled_ones():
    """Half-lengths, radix sequences and Bluestein inner sizes of the length sweep, from
    the restated fftplan::factor / real_plan."""
    for n, rad in S.SINGLE_PASS + S.MIXED_PASS:
        p = S.real_plan(n)
        assert p["even"] and not p["blue"] and p["m"] == n // 2 and p["rad"] == rad, (n, p)
    for n, inner in S.BLUE_EVEN:
        p = S.real_plan(n)
        assert p["even"] and p["blue"] and p["size"] == inner, (n, p)
    for n, inner in S.ODD:
        p = S.real_plan(n)
        assert not p["even"] and p["m"] == n and p["blue"] == (inner is not None), (n, p)
        assert inner is None or p["size"] == inner, (n, p)
    # every register radix of fft_lds.h but 5 and 6 (hot lengths: 750 = 5 6 25) runs in the sweep
    seen = {r for n in S.SWEEP_LENGTHS for r in S.real_plan(n)["rad"]}
    assert seen >= set(S.RADICES) - {5, 6}, sorted(seen)


def test_routing_boundaries():
    """15 552 is the last even radix-only length of the small kernel and 15 680 the first of
    the big one; the big kernel ends at 39 690 among the even radix-only lengths."""
    smooth = [n for n in range(15000, 40100, 2) if S.factor(n // 2) is not None]
    routes = {n: S.runtime_route(n) for n in smooth}
    assert max(n for n in smooth if routes[n] == "small") == 15552
    assert min(n for n in smooth if routes[n] == "big") == 15680
    assert max(n for n in smooth if routes[n] == "big") == 39690
    assert routes[40000] == "f64"
    assert S.runtime_route(16382) == "big" and S.runtime_route(16386) == "f64"
    assert S.runtime_route(4098) == "big" and S.real_plan(4098)["lds_bytes"] > S.SMALL_BYTES


def _check(case):
    ref = S.reference(case)
    ev, micro, grain, e32 = ref.ev, ref.micro, ref.grain, ref.e32
    assert ev.n == case.n == micro.size == grain.size, (case.id, ev.n)
    assert S.predicted_route(case) == case.route, (case.id, S.predicted_route(case), case.route)
    assert np.isfinite(grain).all() and float(np.max(np.abs(grain))) > 0.0, case.id
    print(f"{case.id}: route {case.route}, e32 {e32:.3e}, tilt step {ref.e32_micro:.3e}, kappa {ref.kappa:.3g}")
    assert e32 <= HARD_TOL and ref.e32_micro <= HARD_TOL, (case.id, e32, ref.e32_micro)
    assert (ref.e32_micro > 0.0) == S.tilted(case.params)


@pytest.mark.parametrize("n", S.SWEEP_LENGTHS)
def test_sweep_cases(n):
    for case in S.sweep_cases(n):
        _check(case)


@pytest.mark.parametrize("group", S.EDGE_GROUPS)
@pytest.mark.parametrize("tag", S.EDGE_TAGS)
def test_edge_cases(tag, group):
    cases = S.edge_cases(tag, group)
    for case in cases:
        _check(case)
    if tag == "37500res-s3on":       # the band-pruned kernel is really reached; it takes no power warp
        assert any(c.route == "spec3" for c in cases) == (group != "warp"), [c.route for c in cases]
    if tag.startswith("37500noise"):
        assert all(c.route == "ct37500" for c in cases)


@pytest.mark.parametrize("n", S.TILT_LENGTHS)
def test_tilt_cases(n):
    for case in S.tilt_cases(n):
        _check(case)


@pytest.mark.parametrize("hot", [1500, 37500])
def test_odd_offset_presets(hot):
    """Five odd-length grains, then four hot ones at odd float offsets of the pool (the
    pool packs a preset's grains back to back); the odd length stays on the float32 engine."""
    p, odd, routes = S.odd_offset_preset(hot)
    ns = [e.n for e in S.O.plan_render(p).events]
    assert ns == [odd] * 5 + [hot] * 4 and odd % 2 == 1
    assert routes == {S.runtime_route(odd): 5, S.CT_LENGTHS[hot]: 4}
    offs = np.cumsum([0] + ns[:-1])
    assert all(o % 2 == 1 for o, n in zip(offs, ns) if n == hot)
    assert {int(o) % 4 for o, n in zip(offs, ns) if n == odd} == {0, 1, 2, 3}


def test_dropped_tilt_cases_are_beyond_float32():
    """The two cases left out of the tilt step's list: the float32 reference of the tilt step
    misses 1e-5 there by itself (measured 5.0e-5 and 9.6e-5), so no float32 kernel is asked to."""
    assert [c.id for c in S.tilt_cases(16)] != [] and len(S.tilt_cases(16)) == 6
    for n, g, t in S.TILT_DROPPED:
        ref = S.reference(S.tilt_case(n, g, t))
        print(f"dropped tilt-{n} {g} {t:+g}: float32 tilt step {ref.e32_micro:.3e}")
        assert ref.e32_micro > 3.0 * HARD_TOL
        assert len(S.tilt_cases(n)) == 5


def test_hard_cutoff_lands_on_the_bin():
    """The on-bin cases put cutoff_out * ufac on rfftfreq's own value of the bin, bit for
    bit, and the neighbours 1e-6 Hz to either side of it."""
    for tag, n, base_sr, unfold, _, _, _ in S.EDGE_CONFIGS:
        on, under, over = S.edge_cases(tag, "cutoff")[:3]
        sr = S.O.design_sr(base_sr, unfold)
        f = S.O.bin_freqs(n, float(sr))
        c = on.params["bandlimit_out_hz"] * unfold
        k = int(np.argmin(np.abs(f - c)))
        assert f[k] == c and 0 < k < f.size - 1, (tag, k)
        cu, co = under.params["bandlimit_out_hz"] * unfold, over.params["bandlimit_out_hz"] * unfold
        assert f[k - 1] < cu < f[k] < co < f[k + 1] and co - cu < 3e-6, (tag, cu, co)
    assert S.exact_bin(1500, 1200000, 25.0, 500)[0] == 500       # 16 kHz x 25 on bin 500
    assert S.exact_bin(37500, 30000000, 100.0, 2250) == (2250, 18000.0)
