"""The spectral owner assignment (csrc/gen_share.h, specshare; host function) against a
brute-force restatement of its rule (tests/spec_share_keys.py).

The float32 spectral chain of an event depends on its micro grain and on EventRt's ops,
n, gen_sr, cutoff_gen, roll, stretch, tilt_alpha, env_tau and warp_power only, so the
first event of a batch, in list order, with a generator owner, those fields' bits and a
kernel route runs the chain for all events that share them.  The last event of a
tilt-mode preset writes micro_last and always runs.  The events come from the host
planner (msg_plan_host), as in the render.
"""
import ctypes as C

import pytest

from msgpu import _lib as L
from msgpu.pack import Banks, pack_preset
from msgpu.params import config_params, merged

import spec_share_keys as K


def _fn():
    fn = L.lib().msg_debug_spec_owners
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(L.MsgPreset), C.c_int32, C.POINTER(L.MsgEvent), C.POINTER(C.c_int32),
                   C.POINTER(C.c_int32), C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                   C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    return fn


def plan_batch(params_list):
    """Presets, their planned events back to back, slot bases and event counts."""
    lib = L.lib()
    presets, events, base, count = [], [], [], []
    for p in params_list:
        banks = Banks()
        s = pack_preset(p, banks)
        info = L.MsgPlanInfo()
        assert lib.msg_plan_host(C.byref(s), banks.bp_array(), None, 0, C.byref(info), None, 0, None, None) == 0
        ev = (L.MsgEvent * max(1, info.n_slots))()
        assert lib.msg_plan_host(C.byref(s), banks.bp_array(), None, 0, C.byref(info), ev, info.n_slots,
                                 None, None) == 0
        base.append(len(events))
        count.append(info.n_events)
        presets.append(s)
        events.extend(list(ev)[:info.n_slots])      # reserved slots beyond n_events stay in the layout
    return presets, events, base, count


def owners(presets, events, base, count, gen_share=True, spec_share=True):
    n = len(events)
    pa = (L.MsgPreset * len(presets))(*presets)
    ea = (L.MsgEvent * max(1, n))(*events)
    ba = (C.c_int32 * len(base))(*base)
    ca = (C.c_int32 * len(count))(*count)
    out = (C.c_int32 * max(1, n))(*([-7] * max(1, n)))
    gen = (C.c_int32 * max(1, n))(*([-7] * max(1, n)))
    tot = C.c_int64(-1)
    assert _fn()(pa, len(presets), ea, ba, ca, n, int(gen_share), int(spec_share), out, gen, C.byref(tot)) == 0
    return list(out)[:n], list(gen)[:n], tot.value


def check(params_list):
    """The library's owners against the restated rule; returns the counts and the batch."""
    presets, events, base, count = plan_batch(params_list)
    got, gen, runs = owners(presets, events, base, count)
    want, want_runs, n_keys, n_gen = K.expected(presets, events, base, count)
    n_ev = sum(count)
    assert n_ev > 0
    for slot, o in want.items():
        assert got[slot] == o, (slot, got[slot], o)
        assert o <= slot and got[o] == o             # the owner precedes every sharer, and runs itself
        assert gen[o] == gen[slot]                   # and reads the same micro grain
    assert runs == want_runs == sum(1 for slot in want if got[slot] == slot)
    for p, s in enumerate(presets):                  # an event with a micro_last to write is always on a list
        last = base[p] + count[p] - 1
        if count[p] and K.spec_ops(s, events[last]) & K.TILT:
            assert got[last] == last
    tilt_last = sum(1 for p, s in enumerate(presets) if count[p] and K.spec_ops(s, events[base[p] + count[p] - 1]) & K.TILT)
    assert n_keys <= runs <= n_keys + tilt_last      # the owners, and the tilt presets' last events
    # share off (either switch): every event its own owner
    for kw in (dict(spec_share=False), dict(gen_share=False)):
        ident, _, runs0 = owners(presets, events, base, count, **kw)
        assert all(ident[s] == s for s in want) and runs0 == n_ev
    return n_ev, runs, n_keys, n_gen, (presets, events, base, count, got)


def c3(seed, irs, **kw):
    kw.setdefault("out_dur_s", 0.4)
    return config_params("C3", seed=seed, irs=irs, **kw)


def h48(seed, irs, **kw):
    kw.setdefault("out_dur_s", 0.45)
    return config_params("H48", seed=seed, irs=irs, **kw)


@pytest.mark.parametrize("cfg", [c3, h48])
def test_consecutive_seeds_share(irs, cfg):
    n_ev, runs, n_keys, n_gen, _ = check([cfg(1000 + s, irs) for s in range(6)])
    assert runs == n_keys == n_gen < n_ev            # flat lanes: one spectral run per generated grain


def test_three_stretches_share_the_generator_only(irs):
    n_ev, runs, n_keys, n_gen, (presets, events, base, count, got) = check(
        [c3(1000, irs, partial_stretch=st) for st in (2.0, 1.5, 3.0)])
    assert n_gen == count[0] and runs == n_keys == n_ev     # every event runs, on a third of the grains


def test_stretches_and_seeds(irs):
    n_ev, runs, n_keys, n_gen, _ = check([c3(1003 + s, irs, partial_stretch=st)
                                          for s in range(2) for st in (1.0, 1.5, 2.5)])
    assert n_gen < runs == n_keys < n_ev


@pytest.mark.parametrize("change", [dict(bandlimit_out_hz=12000.0), dict(bandlimit_roll_hz=1000.0),
                                    dict(nl_warp_on=True), dict(nl_warp_on=True, nl_warp_power=1.5),
                                    dict(noise_tilt=-4.5), dict(bandlimit_on=False)])
def test_other_parameters_are_separate(irs, change):
    """The same seed with another cutoff, roll, warp or tilt: the generator's grains are
    shared, the spectral runs are not.  (nl_warp_power against nl_warp_power: both presets warp.)"""
    kw = dict(nl_warp_on=True) if "nl_warp_power" in change else {}
    a, b = h48(1000, irs, **kw), h48(1000, irs, **{**kw, **change})
    n_ev, runs, n_keys, n_gen, (presets, events, base, count, got) = check([a, b])
    assert 2 * n_gen == n_ev and runs == n_ev
    # a third preset equal to the second shares with it, not with the first
    n_ev3, runs3, _, _, (_, _, base3, count3, got3) = check([a, b, dict(b)])
    assert runs3 == runs
    assert [got3[base3[2] + k] for k in range(count3[2])] == [base3[1] + k for k in range(count3[1])]


@pytest.mark.parametrize("lane", ["bp_stretch", "bp_cutoff"])
def test_a_lane_gives_per_event_keys(irs, lane):
    """A time-varying stretch or cutoff lane: the events of consecutive seeds that share a
    stream lie at different times, so their lane values differ and they do not share;
    equal seeds still do."""
    val = "0:1.2, 0.45:2.4" if lane == "bp_stretch" else "0:9000, 0.45:17000"
    n_ev, runs, n_keys, n_gen, _ = check([h48(1000 + s, irs, **{lane: val}) for s in range(4)])
    assert n_gen < n_ev and runs == n_keys
    assert runs > n_gen                              # fewer shares than the generator has
    n_ev2, runs2, _, n_gen2, _ = check([h48(1000, irs, **{lane: val})] * 2)
    assert 2 * runs2 == n_ev2 == 2 * n_gen2


@pytest.mark.parametrize("mode", ["Noise burst", "Skewed transient"])
def test_tilt_presets_last_events_always_run(irs, mode):
    params = [h48(1000 + s, irs, gen_mode=mode, partial_stretch=st) for s in range(3) for st in (1.0, 1.5)]
    n_ev, runs, n_keys, n_gen, (presets, events, base, count, got) = check(params)
    assert n_gen < n_keys <= runs < n_ev
    for p in range(len(params)):
        assert got[base[p] + count[p] - 1] == base[p] + count[p] - 1
    # equal presets: the second one's last event has an owner to borrow from, and runs all the same
    n_ev2, runs2, n_keys2, _, (_, _, base2, count2, got2) = check([params[0], dict(params[0])])
    assert runs2 == n_keys2 + 1 and got2[base2[1] + count2[1] - 1] == base2[1] + count2[1] - 1


def test_last_event_that_borrows(irs):
    """Equal presets outside the tilt modes: the second one's last event is no owner, so its
    grain_last is read from the first one's slot."""
    n_ev, runs, n_keys, n_gen, (presets, events, base, count, got) = check([h48(1000, irs), h48(1000, irs)])
    assert got[base[1] + count[1] - 1] == base[0] + count[0] - 1 and 2 * runs == n_ev


def test_unrelated_seeds_share_nothing(irs):
    n_ev, runs, n_keys, n_gen, _ = check([c3(1000 + 1000 * s, irs) for s in range(6)])
    assert runs == n_keys == n_gen == n_ev


def test_list_order_decides_the_owner(irs):
    seeds = [1003, 1000, 5_000_001, 1002, 1001, 5_000_000, 77_000, 1000]
    n_ev, runs, n_keys, n_gen, (presets, events, base, count, got) = check([h48(s, irs) for s in seeds])
    assert runs == n_keys < n_ev
    assert [got[base[7] + k] for k in range(count[7])] == [got[base[1] + k] for k in range(count[1])]


def test_lanes_vary_n_inside_a_preset():
    kw = dict(event_process="Poisson", out_dur_s=1.5, base_sr=48000, gen_mode="Resonant strike",
              grains_per_sec=30.0)
    a = [merged(seed=500 + s, bp_unfold="0:4, 1.5:12", **kw) for s in range(4)]
    n_ev, runs, n_keys, n_gen, (presets, events, base, count, got) = check(a + a)
    assert len({e.n for e in events}) > 2 and runs <= n_ev // 2
