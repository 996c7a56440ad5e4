"""Spectral sharing on the device (csrc/gen_share.h specshare): events of a
batch whose spectral keys are equal read one grain, transformed once.

The same kernel on the same micro grain with the same parameters computes the same
grain, so every batch below must give the same bits as with MSGPU_SPEC_SHARE=0 (every
event runs the chain) and as each preset rendered alone -- the output, and micro_last /
grain_last of each preset's last event -- and the count of spectral runs the library
reports must be the one the restated rule gives for the planned events
(tests/spec_share_keys.py: the distinct keys, plus the last events of tilt-mode presets
that are not the first with their key).  Grain lengths 480 (k_spectral_ct, plan 240), 2400
(plan 1200), 384 (k_spectral, runtime plan) and 37500 (k_spec3).
"""
import os

import numpy as np
import pytest

import spec_share_keys as K

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
    """Output, per-preset (micro_last, grain_last), events and the stage counters of one batch."""
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
    return outs, metas, events, [int(round(v)) for v in t[18:22]]


def _expected(params, events):
    from msgpu.pack import Banks, pack_preset
    presets = [pack_preset(p, Banks()) for p in params]
    flat, base, count = [], [], []
    for evs in events:
        base.append(len(flat))
        count.append(len(evs))
        flat.extend(evs)
    own, runs, n_keys, n_gen = K.expected(presets, flat, base, count)
    borrowed_last = [p for p in range(len(params)) if count[p] and own[base[p] + count[p] - 1] != base[p] + count[p] - 1]
    return runs, n_keys, n_gen, borrowed_last


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def check_batch(params, lengths, env=None, ref_env=None):
    """Render with sharing (under env), compare with ref_env (default: env + MSGPU_SPEC_SHARE=0)
    and with each preset alone; returns (events, generated grains, spectral runs, presets
    whose last event borrows its grain, fused overlap-adds)."""
    env = dict(env or {})
    shared = _engine(env)
    outs, metas, events, (n_fused, n_ev, n_gen, n_run) = _render(shared, params)
    assert {e.n for evs in events for e in evs} == set(lengths)     # the kernels this case is about
    assert n_ev == sum(len(evs) for evs in events) > 0
    want_runs, n_keys, want_gen, borrowed_last = _expected(params, events)
    print(f"{len(params)} presets, {n_ev} events, {n_gen} generated grains, {n_run} spectral runs "
          f"({n_keys} distinct keys, {want_runs} runs expected), {len(borrowed_last)} borrowed last events")
    assert n_gen == want_gen and n_run == want_runs
    plain = _engine(ref_env if ref_env is not None else {**env, "MSGPU_SPEC_SHARE": "0"})
    outs0, metas0, _, (_, n_ev0, n_gen0, n_run0) = _render(plain, params)
    plain.close()
    assert n_ev0 == n_ev and n_run0 == n_ev and n_gen0 == n_gen
    for i in range(len(params)):
        assert _same(outs[i], outs0[i]), i
        assert _same(metas[i][0], metas0[i][0]) and _same(metas[i][1], metas0[i][1]), i
    for i, p in enumerate(params):                                  # each preset alone (nothing to share with)
        o1, m1, _, (_, ne1, ng1, nr1) = _render(shared, [p])
        assert ne1 == ng1 == nr1 == len(events[i])
        assert _same(outs[i], o1[0]), i
        assert _same(metas[i][0], m1[0][0]) and _same(metas[i][1], m1[0][1]), i
    shared.close()
    return n_ev, n_gen, n_run, borrowed_last, n_fused


# n = 480: 48 kHz x unfold 8 (H48); n = 2400: 192 kHz x unfold 10 (C2); n = 37500: C3
SHORT = {480: ("H48", 0.45), 2400: ("C2", 0.3), 37500: ("C3", 0.3)}


def _cfg(msgpu, irs, n, seed, **kw):
    name, dur = SHORT[n]
    return msgpu.config_params(name, seed=seed, irs=irs, out_dur_s=dur, **kw)


@pytest.mark.parametrize("n", [480, 2400, 37500])
def test_consecutive_seeds(msgpu, irs, n):                                  # 1
    n_ev, n_gen, n_run, _, _ = check_batch([_cfg(msgpu, irs, n, 1000 + s) for s in range(6 if n < 37500 else 4)], {n})
    assert n_run == n_gen < n_ev


@pytest.mark.parametrize("n", [480, 37500])
def test_stretches_of_two_seeds(msgpu, irs, n):                             # 2
    n_ev, n_gen, n_run, _, _ = check_batch([_cfg(msgpu, irs, n, 1003 + s, partial_stretch=st)
                                            for s in range(2) for st in (1.0, 1.5, 2.5)], {n})
    assert n_gen < n_run < n_ev


@pytest.mark.parametrize("mode", ["Noise burst", "Skewed transient"])
def test_tilt_path(msgpu, irs, mode):                                       # 3
    """micro_last is still written for every preset: the last event of each runs the chain."""
    n_ev, n_gen, n_run, borrowed_last, _ = check_batch(
        [_cfg(msgpu, irs, 480, 1000 + s, gen_mode=mode, partial_stretch=st) for s in range(3) for st in (1.0, 1.5)],
        {480})
    assert n_gen < n_run < n_ev and not borrowed_last


def test_grain_last_through_the_owner(msgpu, irs):                          # 4
    """Equal presets and consecutive seeds: the last events of some presets run no kernel, and
    msg_last_meta reads their grain_last from the owner's slot."""
    params = [_cfg(msgpu, irs, 480, s) for s in (1000, 1000, 1001, 1001)] + [_cfg(msgpu, irs, 2400, 1000)] * 2
    n_ev, n_gen, n_run, borrowed_last, _ = check_batch(params, {480, 2400})
    assert 1 in borrowed_last and 3 in borrowed_last and 5 in borrowed_last and n_run < n_ev


def test_copy_and_runtime_plan(msgpu, irs):                                 # 5
    """Band limit off and stretch 1 (ops == 0: grain = micro, the copy), and micro_ms 1.0 at
    384 kHz (n = 384, no compile-time plan: k_spectral)."""
    n_ev, n_gen, n_run, _, _ = check_batch(
        [_cfg(msgpu, irs, 480, 1000 + s, bandlimit_on=False, partial_stretch=1.0) for s in range(3)], {480})
    assert n_run == n_gen < n_ev
    n_ev, n_gen, n_run, _, _ = check_batch([_cfg(msgpu, irs, 480, 1000 + s, micro_ms=1.0) for s in range(3)], {384})
    assert n_run == n_gen < n_ev


@pytest.mark.parametrize("fir64", ["1", "2"])
def test_fused_overlap_add(msgpu, irs, fir64):                              # 6
    """The overlap-add inside k_fir8p (ola_ev), and with MSGPU_FIR64=2 k_ola_slots, read the
    owners' slots: the bits of the separate overlap-add with sharing off."""
    env = {"MSGPU_OLA_FIR": "1", "MSGPU_OLA_FIR_DENSITY": "1e9", "MSGPU_FIR64": fir64}
    ref = {"MSGPU_OLA_FIR": "0", "MSGPU_SPEC_SHARE": "0", "MSGPU_FIR64": fir64}
    n_ev, n_gen, n_run, _, n_fused = check_batch([_cfg(msgpu, irs, 37500, 1000 + s) for s in range(3)], {37500},
                                                 env=env, ref_env=ref)
    assert n_fused == 3 and n_run == n_gen < n_ev


def test_stretch_lane_beside_flat_ones(msgpu, irs):                         # 7
    """A time-varying bp_stretch lane: per-event keys for that preset, bits unchanged."""
    params = [_cfg(msgpu, irs, 480, 1000), _cfg(msgpu, irs, 480, 1001, bp_stretch="0:1.2, 0.45:2.4"),
              _cfg(msgpu, irs, 480, 1002), _cfg(msgpu, irs, 480, 1003, bp_stretch="0:1.2, 0.45:2.4")]
    n_ev, n_gen, n_run, _, _ = check_batch(params, {480})
    assert n_gen < n_run <= n_ev
