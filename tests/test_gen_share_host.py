"""The generator's owner assignment (csrc/gen_share.h, host function) against a
brute-force restatement of its rule.

Event i of a render draws default_rng(seed + i) (MS:650-686), so two events of a
batch whose generator keys are equal -- the stream seed + i, the grain length n,
the design rate, the mode after the fallback mapping (MS:686), ring_hz,
ring_decay_ms and micro_ms, compared bitwise -- get the same grain from
k_gen_normal.  The first of them in list order is the owner and the only one
generated; the others read its slot.  The events come from the host planner
(msg_plan_host), as in the render.
"""
import ctypes as C
import struct

import pytest

from msgpu import _lib as L
from msgpu.pack import Banks, pack_preset
from msgpu.params import config_params, merged


def _fn():
    fn = L.lib().msg_debug_gen_owners
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(L.MsgPreset), C.c_int32, C.POINTER(L.MsgEvent), C.POINTER(C.c_int32),
                   C.POINTER(C.c_int32), C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
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


def owners(presets, events, base, count, share=True):
    n = len(events)
    pa = (L.MsgPreset * len(presets))(*presets)
    ea = (L.MsgEvent * max(1, n))(*events)
    ba = (C.c_int32 * len(base))(*base)
    ca = (C.c_int32 * len(count))(*count)
    out = (C.c_int32 * max(1, n))(*([-7] * max(1, n)))
    tot = C.c_int64(-1)
    assert _fn()(pa, len(presets), ea, ba, ca, n, int(share), out, C.byref(tot)) == 0
    return list(out)[:n], tot.value


def _bits(x):
    return struct.pack("<d", float(x))


def expected(presets, events, base, count):
    """First event in list order per key, by a dictionary over the full keys."""
    first, own = {}, {}
    for p, s in enumerate(presets):
        mode = 2 if s.gen_mode == L.GEN_FALLBACK else s.gen_mode       # Noise burst, MS:686
        for k in range(count[p]):
            slot = base[p] + k
            e = events[slot]
            key = ((s.seed + e.index) & (2 ** 64 - 1), e.n, e.gen_sr, mode, _bits(s.ring_hz),
                   _bits(s.ring_decay_ms), _bits(s.micro_ms))
            own[slot] = first.setdefault(key, slot)
    return own


def check(params_list):
    presets, events, base, count = plan_batch(params_list)
    got, tot = owners(presets, events, base, count)
    want = expected(presets, events, base, count)
    n_ev = sum(count)
    assert n_ev > 0
    for slot, o in want.items():
        assert got[slot] == o, (slot, got[slot], o)
        assert o <= slot and got[o] == o               # the owner is the first in list order, and its own
    assert tot == len(set(want.values()))
    # every event its own owner with sharing off
    ident, tot0 = owners(presets, events, base, count, share=False)
    assert all(ident[s] == s for s in want) and tot0 == n_ev
    return n_ev, tot, (presets, events, base, count, got)


def c3(seed, irs, **kw):
    kw.setdefault("out_dur_s", 0.4)
    return config_params("C3", seed=seed, irs=irs, **kw)


def test_consecutive_seeds(irs):
    n_ev, n_own, (presets, events, base, count, got) = check([c3(1000 + s, irs) for s in range(6)])
    streams = {presets[p].seed + events[base[p] + k].index for p in range(6) for k in range(count[p])}
    assert n_own == len(streams) < n_ev               # one grain per distinct stream
    # seed s + 1's event i - 1 reads seed s's event i (or an earlier owner of that stream)
    for k in range(1, min(count[0], count[1] + 1)):
        assert got[base[1] + k - 1] == got[base[0] + k]


def test_equal_seeds_share_everything(irs):
    n_ev, n_own, (presets, events, base, count, got) = check(
        [c3(1000, irs, partial_stretch=st) for st in (2.0, 1.5, 3.0)])
    assert count[0] == count[1] == count[2] and n_own == count[0]
    for p in (1, 2):
        assert [got[base[p] + k] for k in range(count[p])] == [base[0] + k for k in range(count[0])]


@pytest.mark.parametrize("change", [dict(time_unfold=50.0), dict(ring_hz=4200.5), dict(gen_mode="Gaussian click"),
                                    dict(ring_decay_ms=11.0), dict(micro_ms=1.0)])
def test_equal_stream_other_key_is_separate(irs, change):
    """The same streams with another n (time_unfold 50: a 19.2 MHz design rate), ring_hz,
    mode, ring_decay_ms or micro_ms: separate owners."""
    a, b = c3(1000, irs), c3(1000, irs, **change)
    n_ev, n_own, (presets, events, base, count, got) = check([a, b])
    assert n_own == n_ev
    if "time_unfold" in change:
        assert events[base[0]].n != events[base[1]].n
    # a third preset equal to the second shares with it, not with the first
    n_ev3, n_own3, (_, _, base3, count3, got3) = check([a, b, dict(b)])
    assert n_own3 == n_own
    assert [got3[base3[2] + k] for k in range(count3[2])] == [base3[1] + k for k in range(count3[1])]


def test_disjoint_seeds_share_nothing(irs):
    n_ev, n_own, _ = check([c3(1000 + 1000 * s, irs) for s in range(6)])
    assert n_own == n_ev


def test_list_order_decides_the_owner(irs):
    """Seeds out of order, two clusters far apart and a loner between them."""
    seeds = [1003, 1000, 5_000_001, 1002, 1001, 5_000_000, 77_000, 1000]
    n_ev, n_own, (presets, events, base, count, got) = check([c3(s, irs) for s in seeds])
    assert n_own < n_ev
    assert [got[base[6] + k] for k in range(count[6])] == [base[6] + k for k in range(count[6])]   # the loner
    assert [got[base[7] + k] for k in range(count[7])] == [got[base[1] + k] for k in range(count[1])]


def test_fallback_mode_shares_with_noise_burst():
    """An unknown mode renders as a Noise burst (MS:686): the same raw normals."""
    kw = dict(event_process="Poisson", out_dur_s=0.5, base_sr=48000, time_unfold=8.0, seed=31)
    n_ev, n_own, _ = check([merged(gen_mode="Noise burst", **kw), merged(gen_mode="no such mode", **kw),
                            merged(gen_mode="Skewed transient", **kw)])
    assert n_own * 3 == n_ev * 2


def test_lanes_vary_n_inside_a_preset():
    """An unfold lane gives the events of one preset different design rates and lengths:
    the stream alone does not make the key."""
    kw = dict(event_process="Poisson", out_dur_s=1.5, base_sr=48000, gen_mode="Resonant strike",
              grains_per_sec=30.0)
    a = [merged(seed=500 + s, bp_unfold="0:4, 1.5:12", **kw) for s in range(4)]
    b = [merged(seed=500 + s, bp_unfold="0:12, 1.5:4", **kw) for s in range(4)]
    n_ev, n_own, (presets, events, base, count, got) = check(a + b + a)
    assert len({e.n for e in events}) > 2
    assert n_own < n_ev


def test_large_and_negative_seeds(irs):
    """Seeds whose streams could wrap around 2^63 are left out of the sharing; nothing else changes."""
    presets, events, base, count = plan_batch([c3(1000, irs)] * 5)
    presets[1].seed = presets[2].seed = 2 ** 63 - 3
    presets[3].seed = presets[4].seed = -5
    got, tot = owners(presets, events, base, count)
    assert tot == sum(count) and all(got[base[p] + k] == base[p] + k for p in range(5) for k in range(count[p]))
