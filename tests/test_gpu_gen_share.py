"""Generator sharing on the device (csrc/gen_share.h): events of a batch
whose generator keys are equal read one grain, generated once.

The same kernel computes the same grain, so every batch below must give the same
bits as with MSGPU_GEN_SHARE=0 (every event generates its own) and as each
preset rendered alone -- the output, and micro_last / grain_last of each
preset's last event -- and the generated-grain count the library reports must be
the number of distinct keys among the planned events.  Grain lengths 480
(k_spectral_ct, plan 240), 2400 (plan 1200) and 37500 (k_spec3).
"""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 40000          # >= every grain length here


@pytest.fixture(scope="module")
def msgpu():
    import msgpu as m
    m.render(m.merged(out_dur_s=0.05, er_cloud_on=False))
    assert "libmsgpu" in open("/proc/self/maps").read()   # the HIP library
    return m


def _engine(env):
    from msgpu.engine import Engine
    os.environ.update(env)
    try:
        return Engine(0)                # the switches are read by msg_create
    finally:
        for k in env:
            os.environ.pop(k, None)


def _render(eng, params):
    """Output, per-preset (micro_last, grain_last), events and generated grains of one batch."""
    import torch
    from msgpu.pack import PackedBatch
    packed = PackedBatch(params)
    eng.set_profiling(1)
    o = eng.render_packed(packed)
    torch.cuda.synchronize(0)
    t = eng.stage_times()
    eng.set_profiling(False)
    out = o.cpu().numpy()
    outs = [out[int(packed.offsets[i]):int(packed.offsets[i]) + int(packed.out_n[i])] for i in range(len(params))]
    metas = [eng.last_meta(i, CAP) for i in range(len(params))]
    events = [eng.last_events(i) for i in range(len(params))]
    return outs, metas, events, int(round(t[19])), int(round(t[20]))


def _distinct_keys(params, events):
    """The generator keys of the planned events (gen_share.h), counted."""
    from msgpu import _lib as L
    keys = set()
    for p, evs in zip(params, events):
        mode = L.GEN_MODE.get(p["gen_mode"], 2)
        for e in evs:
            keys.add((int(p["seed"]) + e.index, e.n, e.gen_sr, mode,
                      struct.pack("<3d", p["ring_hz"], p["ring_decay_ms"], p["micro_ms"])))
    return len(keys)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def check_batch(params, lengths, fewer):
    shared = _engine({})
    outs, metas, events, n_ev, n_gen = _render(shared, params)
    assert {e.n for evs in events for e in evs} == set(lengths)     # the kernels this case is about
    assert n_ev == sum(len(evs) for evs in events) > 0
    want = _distinct_keys(params, events)
    print(f"{len(params)} presets, {n_ev} events, {n_gen} generated grains ({want} distinct keys)")
    assert n_gen == want
    assert (n_gen < n_ev) if fewer else (n_gen == n_ev)
    # every event its own owner
    plain = _engine({"MSGPU_GEN_SHARE": "0"})
    outs0, metas0, _, n_ev0, n_gen0 = _render(plain, params)
    plain.close()
    assert n_ev0 == n_ev and n_gen0 == n_ev
    for i in range(len(params)):
        assert _same(outs[i], outs0[i]), i
        assert _same(metas[i][0], metas0[i][0]) and _same(metas[i][1], metas0[i][1]), i
    # each preset alone (nothing to share with)
    for i, p in enumerate(params):
        o1, m1, _, ne1, ng1 = _render(shared, [p])
        assert ne1 == ng1 == len(events[i])
        assert _same(outs[i], o1[0]), i
        assert _same(metas[i][0], m1[0][0]) and _same(metas[i][1], m1[0][1]), i
    shared.close()


# n = 480: 48 kHz x unfold 8 (H48); n = 2400: 192 kHz x unfold 10 (C2); micro_ms 1.25
SHORT = {480: ("H48", 0.45), 2400: ("C2", 0.3)}


def _cfg(msgpu, irs, n, seed, **kw):
    name, dur = SHORT[n]
    return msgpu.config_params(name, seed=seed, irs=irs, out_dur_s=dur, **kw)


@pytest.mark.parametrize("n", [480, 2400])
def test_consecutive_seeds(msgpu, irs, n):                                  # (a)
    check_batch([_cfg(msgpu, irs, n, 1000 + s) for s in range(6)], {n}, fewer=True)


@pytest.mark.parametrize("n", [480, 2400])
def test_one_seed_three_stretches(msgpu, irs, n):                           # (b)
    check_batch([_cfg(msgpu, irs, n, 1003, partial_stretch=st) for st in (1.0, 1.5, 2.5)] +
                [_cfg(msgpu, irs, n, 1004, partial_stretch=st) for st in (1.0, 1.5, 2.5)], {n}, fewer=True)


@pytest.mark.parametrize("n", [480, 2400])
def test_one_seed_two_ring_hz(msgpu, irs, n):                               # (c)
    check_batch([_cfg(msgpu, irs, n, 1000, ring_hz=hz) for hz in (4200.0, 3100.0)], {n}, fewer=False)


def test_one_seed_two_unfolds(msgpu, irs):                                  # (d)
    """time_unfold 8 and 40 at 48 kHz: design rates 384 kHz and 1.92 MHz, n = 480 and 2400."""
    check_batch([_cfg(msgpu, irs, 480, 1000, time_unfold=u) for u in (8.0, 40.0)], {480, 2400}, fewer=False)


@pytest.mark.parametrize("n", [480, 2400])
@pytest.mark.parametrize("mode", ["Noise burst", "Skewed transient"])
def test_tilt_path(msgpu, irs, n, mode):                                    # (e)
    """Raw normals shared, tilt, envelope and skew per event: micro_last is written
    beside the pool, never into the shared slot.  Consecutive seeds, each at two stretches."""
    check_batch([_cfg(msgpu, irs, n, 1000 + s, gen_mode=mode, partial_stretch=st)
                 for s in range(3) for st in (1.0, 1.5)], {n}, fewer=True)


@pytest.mark.parametrize("case", ["seeds", "stretches"])
def test_spec3_grains(msgpu, irs, case):
    """n = 37500 (C3: the band-pruned kernel), three presets: (a) and (b)."""
    if case == "seeds":
        params = [msgpu.config_params("C3", seed=1000 + s, irs=irs, out_dur_s=0.3) for s in range(3)]
    else:
        params = [msgpu.config_params("C3", seed=1001, irs=irs, out_dur_s=0.3, partial_stretch=st)
                  for st in (2.0, 1.0, 3.0)]
    check_batch(params, {37500}, fewer=True)


def test_runtime_plan_kernel(msgpu, irs):
    """A length without a compile-time plan (micro_ms 1.0 at 384 kHz: n = 384, k_spectral),
    and one without a spectral stage (band limit off, stretch 1: grain = micro)."""
    check_batch([_cfg(msgpu, irs, 480, 1000 + s, micro_ms=1.0) for s in range(3)], {384}, fewer=True)
    check_batch([_cfg(msgpu, irs, 480, 1000 + s, bandlimit_on=False, partial_stretch=1.0) for s in range(3)],
                {480}, fewer=True)
