"""The gate on the device (msg_gate_apply; csrc/kernels_gate.h): samples and records to the bit
against the library's host loop (msg_gate_host) at every tile seam, in ragged batches, with the state
carried over hundreds of tiles and across a block of the scan over tiles, alone against in a batch,
with a poisoned neighbour, and in the delivery chain.

profiles/gate_gpu_tests.txt has the values measured on an MI355X, as these tests print them."""
import math
import os

import numpy as np
import pytest

import msgpu
import gate_cases as GC
from msgpu.dynamics import Dynamics, dynamics_host
from msgpu.edges import Edges
from msgpu.gate import GATE_DTYPE, Gate, gate_host, records

pytestmark = pytest.mark.gpu
SR, TILE, N3 = GC.SR, GC.TILE, GC.N3


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def pack(signals, channels, gap=3):
    """The signals back to back with ``gap`` NaN guard frames around and between them (an odd gap:
    mono signals at odd float offsets, stereo signals at odd frames): (buffer, offsets, lens)."""
    shape = (gap, 2) if channels == 2 else (gap,)
    guard = np.full(shape, np.nan, dtype=np.float32)
    offs, lens, parts, at = [], [], [guard], gap
    for s in signals:
        offs.append(at)
        lens.append(len(s))
        parts += [np.asarray(s, dtype=np.float32).reshape((len(s), 2) if channels == 2 else (len(s),)), guard]
        at += len(s) + gap
        if len(offs) % 2:                                           # and every other signal one more frame on
            parts.append(guard[:1])
            at += 1
    return np.concatenate(parts), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)


def run(eng, signals, channels, gate, gap=3, sr=SR):
    """One msg_gate_apply call over the packed signals: (buffer before, buffer after, offsets, lens, records)."""
    buf, offs, lens = pack(signals, channels, gap)
    x = eng.torch.from_numpy(buf).cuda()
    rec = eng.gate_apply(x, offs, lens, channels, sr, gate)
    assert tuple(rec.shape) == (len(signals), 6)
    return buf, x.cpu().numpy(), offs, lens, records(rec)


def raw(rec):
    """The record's own fields as bytes (records() adds derived columns)."""
    return np.array([tuple(r[k] for k in GATE_DTYPE.names) for r in np.atleast_1d(rec)], dtype=GATE_DTYPE).tobytes()


def check_against_host(eng, signals, channels, gate, what, gap=3, sr=SR):
    buf, got, offs, lens, rec = run(eng, signals, channels, gate, gap, sr)
    inside = np.zeros(len(buf), dtype=bool)
    for i, (s, o, n) in enumerate(zip(signals, offs, lens)):
        inside[o:o + n] = True
        want, want_rec = gate_host(s, sr, gate)
        assert np.array_equal(GC.bits(got[o:o + n]), GC.bits(want)), (what, i, int(n))
        assert raw(rec[i]) == want_rec.tobytes(), (what, i, int(n), rec[i], want_rec)
    assert np.array_equal(GC.bits(got[~inside]), GC.bits(buf[~inside])), what      # the NaN guards, bit for bit
    return rec


# ---- device == host to the bit ------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", list(GC.OPTIONS))
def test_device_is_the_host_loop(eng, name, channels):
    """Lengths 0, 1, 2, 4095, 4096, 4097 and 3 x 4096 + 5, the four placements of one opening frame and the
    signal that stays open through three tiles between the thresholds, in one ragged batch; "slow": the
    closing ramp of an opening at frame 0 crosses every later tile and the opening ramp of one at the last
    frame every earlier one."""
    gate = GC.OPTIONS[name]
    rec = check_against_host(eng, GC.seam_signals(channels, gate), channels, gate, name)
    k = len(GC.LENGTHS)
    hold = gate.opts(SR).hold_frames
    assert list(rec["opens"][k:k + 4]) == [1, 1, 1, 1]
    assert list(rec["open_frames"][k:k + 4]) == [min(hold + 1, N3 - at) for at in (0, TILE - 1, TILE, N3 - 1)]
    if float(gate.hysteresis_db) > 0:
        assert rec["opens"][-1] == 1 and rec["open_frames"][-1] == N3 - 110 + min(hold, 100)   # open from 10 to the closer
    if name == "slow":
        print(f"slow, {channels} ch: an opening at frame 0 and at the last frame, mean reduction over {N3} frames "
              f"{rec[k]['mean_reduction_db']:.4f} / {rec[k + 3]['mean_reduction_db']:.4f} dB, max "
              f"{rec[k]['max_reduction_db']:.4f} dB (10 dB take 24000 frames)")
        assert rec[k]["max_e"] == (N3 - 1) * gate.opts(SR).release_step                      # still closing at the far end
        assert rec[k + 3]["max_e"] == (N3 - 1) * gate.opts(SR).attack_step


@pytest.mark.parametrize("hold", [100, 10000])
def test_last_open_frame_before_a_seam_is_held_across_it(eng, hold):
    """The last open frame at 4090: a hold of 100 frames ends 94 frames into the next tile, one of 10 000
    frames crosses two seams and saturates nowhere inside the signal."""
    gate = Gate(threshold_db=-40.0, hysteresis_db=0.0, hold_ms=GC.hold_ms(hold), release_ms=5.0)
    for channels in (1, 2):
        rec = check_against_host(eng, [GC.spike(N3, channels, TILE - 6), GC.spike(TILE - 5, channels, TILE - 6)], channels,
                                 gate, f"hold {hold}")
        assert rec[0]["open_frames"] == min(hold + 1, N3 - (TILE - 6)) and rec[1]["open_frames"] == 1
        assert list(rec["hold_frames"]) == [hold, hold]


def test_even_offsets_and_threshold_under_every_sample(eng):
    for channels in (1, 2):
        gate = GC.OPTIONS["default"]
        sig = GC.seam_signals(channels, gate)
        check_against_host(eng, sig, channels, gate, "even gap", gap=4)
        check_against_host(eng, sig, channels, GC.OPTIONS["local"], "even gap, local", gap=4)
        sig = [np.where(np.abs(s) < 1e-6, np.float32(1e-6), s).astype(np.float32) for s in sig]
        buf, got, offs, lens, rec = run(eng, sig, channels, Gate(threshold_db=-150.0))
        assert np.array_equal(GC.bits(got), GC.bits(buf))                                    # nothing is written
        assert np.all(rec["state"] == 0) and np.all(rec["max_e"] == 0) and np.array_equal(rec["open_frames"], lens)


def test_state_crosses_a_block_of_the_tile_scan(eng):
    """600 tiles: an opener in tile 2, then 300 tiles and more between the thresholds with nothing deciding
    the state, a closer in tile 590.  The scan over tiles takes 256 tiles a block, so the open state enters
    the second and the third block as a carry; the second signal is the same without the opener."""
    n = 600 * TILE + 123
    rng = np.random.default_rng(77)
    gate = Gate(threshold_db=-40.0, hysteresis_db=6.0, hold_ms=GC.hold_ms(300), release_ms=400.0)
    mid = GC.middle(gate)
    x = (mid * rng.uniform(0.8, 1.2, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))).astype(np.float32)   # within +-1.9 dB of -43 dB
    opener, closer = 2 * TILE + 17, 590 * TILE + 4000
    x[:opener] *= np.float32(1e-2)
    x[closer:] *= np.float32(1e-2)
    shut = x.copy()
    x[opener] = 0.5
    rec = check_against_host(eng, [x, shut, x[:TILE + 1]], 2, gate, "600 tiles")
    print(f"600 tiles: {int(rec[0]['open_frames'])} of {n} frames open in {int(rec[0]['opens'])} opening, "
          f"{int(rec[0]['reduced_frames'])} reduced, mean {rec[0]['mean_reduction_db']:.4f} dB; without the opener "
          f"{int(rec[1]['open_frames'])} open, {int(rec[1]['reduced_frames'])} reduced")
    assert rec[0]["opens"] == 1 and rec[0]["open_frames"] == closer - opener + 300
    assert rec[1]["opens"] == 0 and rec[1]["open_frames"] == 0 and rec[1]["reduced_frames"] == n


def test_dense_signal_of_more_tiles_than_are_resident(eng):
    """3000 tiles of grains over a bed with hysteresis and a hold: far more workgroups than the device holds
    at once, so tiles of the apply sweep start while their neighbours have already stored.  Nothing outside
    a tile may be read then: the samples and the record are the host loop's."""
    n = 3000 * TILE + 77
    rng = np.random.default_rng(5)
    env = np.repeat(10.0 ** (rng.uniform(-95.0, -40.0, n // 64 + 1) / 20.0), 64)[:n]
    x = (rng.standard_normal(n, dtype=np.float32) * env.astype(np.float32)).clip(-1, 1)
    gate = Gate(threshold_db=-45.0, hysteresis_db=6.0, attack_ms=1.0, release_ms=10.0, hold_ms=GC.hold_ms(240))
    rec = check_against_host(eng, [x], 1, gate, "3000 tiles")
    print(f"3000 tiles: {int(rec[0]['open_frames'])} of {n} frames open in {int(rec[0]['opens'])} openings, "
          f"{int(rec[0]['reduced_frames'])} reduced, mean {rec[0]['mean_reduction_db']:.4f} dB")
    assert rec[0]["opens"] > 3000 and 0 < rec[0]["reduced_frames"] < n


def test_nan_neighbour_and_batch_against_solo(eng):
    for channels in (1, 2):
        sig = [GC.texture(n, channels, 60 + i) for i, n in enumerate((N3, 2 * TILE, TILE + 1, 777, 1))]
        bad = sig[1].copy()
        bad.reshape(-1)[5000] = np.nan
        worse = sig[3].copy()
        worse.reshape(-1)[-1] = np.inf
        batch = [sig[0], bad, sig[2], worse, sig[4]]
        gate = GC.OPTIONS["default"]
        buf, got, offs, lens, rec = run(eng, batch, channels, gate)
        for i in (1, 3):                                                                      # as they were, state 2
            assert np.array_equal(GC.bits(got[offs[i]:offs[i] + lens[i]]), GC.bits(batch[i]))
            assert rec[i]["state"] == 2 and rec[i]["max_e"] == 0 and rec[i]["reduced_frames"] == 0 and rec[i]["open_frames"] == 0
        for i in (0, 2, 4):                                                                   # the neighbours: their solo runs
            for gap in (3, 4):
                _, solo, o, k, solo_rec = run(eng, [batch[i]], channels, gate, gap)
                assert np.array_equal(GC.bits(solo[o[0]:o[0] + k[0]]), GC.bits(got[offs[i]:offs[i] + lens[i]])), (i, gap)
                assert raw(solo_rec[0]) == raw(rec[i])
        order = [4, 2, 0]                                                                     # another batch: the same bits
        _, again, o2, k2, rec2 = run(eng, [batch[i] for i in order], channels, gate, 5)
        for j, i in enumerate(order):
            assert np.array_equal(GC.bits(again[o2[j]:o2[j] + k2[j]]), GC.bits(got[offs[i]:offs[i] + lens[i]]))
            assert raw(rec2[j]) == raw(rec[i])


def test_public_function_and_refusals(eng):
    x = GC.texture(TILE + 9, 2, 5)
    gate = Gate(threshold_db=-44.0, ratio=3.0, range_db=30.0)
    want, want_rec = gate_host(x, SR, gate)
    y, rec = msgpu.gate(x, SR, gate)                                                          # NumPy in: a copy and its record
    assert np.array_equal(GC.bits(y), GC.bits(want)) and raw(rec) == want_rec.tobytes() and rec["max_reduction_db"] > 0
    t = eng.torch.from_numpy(x).cuda()
    dev = msgpu.gate(t, SR, gate)                                                             # a tensor in: in place, the device record
    assert np.array_equal(GC.bits(t.cpu().numpy()), GC.bits(want)) and raw(records(dev)[0]) == want_rec.tobytes()
    mono = msgpu.gate(x[:, 0].copy(), SR, gate)[0]
    assert np.array_equal(GC.bits(mono), GC.bits(gate_host(x[:, 0].copy(), SR, gate)[0]))
    before = t.clone()
    with pytest.raises(ValueError, match="overlap"):                                          # it writes where it reads
        eng.gate_apply(t, [0, 100], [200, 200], 2, SR, gate)
    with pytest.raises(ValueError):
        eng.gate_apply(t, [0], [len(x) + 1], 2, SR, gate)
    with pytest.raises(ValueError):
        eng.gate_apply(t, [-1], [10], 2, SR, gate)
    with pytest.raises(ValueError, match="range_db"):
        eng.gate_apply(t, [0], [100], 2, SR, Gate(range_db=0.0))
    with pytest.raises(ValueError, match="ratio"):
        msgpu.gate(x, SR, Gate(ratio=0.5))
    assert eng.torch.equal(before, t)                                                         # the refused calls wrote nothing
    assert tuple(eng.gate_apply(t, [], [], 2, SR, gate).shape) == (0, 6)


# ---- the delivery chain -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(irs):
    return msgpu.config_params("C2", irs=irs, out_dur_s=0.75)


# The 0.75 s render (192 kHz) ends in a strike whose tail falls from -20 dB to -60 dB within 4000 frames.  This gate closes
# under -32 dB, holds 960 frames and then falls 10 dB in every 960 more, so its silence begins before the tail's own -60 dB.
G = Gate(threshold_db=-26.0, hysteresis_db=6.0, range_db=math.inf, attack_ms=0.5, release_ms=5.0, hold_ms=5.0)
D = Dynamics(threshold_db=-30.0, ratio=4.0, knee_db=6.0, attack_ms=2.0, release_ms=60.0, hold_ms=5.0, makeup_db=3.0)


def test_chain_equals_the_rules_by_hand(eng, c2):
    from msgpu.export import edges_packed, loudness_packed, quantize_packed, unpack_all
    sr = int(c2["base_sr"])
    trim = Edges(trim_db=-60)
    kw = dict(out_edges=trim, out_lufs=-23, out_true_peak=-1, out_bits=16)
    out = msgpu.render_batch([c2], out_gate=G, out_dynamics=D, **kw)
    ungated = msgpu.render_batch([c2], out_dynamics=D, **kw)
    plain = msgpu.render_batch([c2])[0]
    n = plain.shape[0]
    t = eng.torch.from_numpy(plain).cuda()
    rec = records(msgpu.gate(t, sr, G))[0]                                                    # the public function, in place
    gated = gate_host(plain, sr, G)[0]
    assert np.array_equal(GC.bits(t.cpu().numpy()), GC.bits(gated))
    msgpu.dynamics(t, sr, D)
    assert np.array_equal(GC.bits(t.cpu().numpy()), GC.bits(dynamics_host(gated, sr, D)[0]))
    off, cnt, _ = edges_packed(eng, t, [0], [n], [sr], trim)
    loudness_packed(eng, t, off, cnt, [sr], -23, None, -1)
    q, qoff, nbytes, _ = quantize_packed(eng, t, off, cnt, 16, keys=[0])
    by_hand = unpack_all(q.cpu().numpy(), qoff, nbytes, 16)[0]
    assert len(out) == 1 and out[0].dtype == np.int16 and np.array_equal(by_hand, out[0])
    print(f"chain: {int(rec['open_frames'])} of {n} frames open in {int(rec['opens'])} openings, "
          f"{int(rec['reduced_frames'])} reduced, max {rec['max_reduction_db']:.3f} dB; trimmed at -60 dB the gated render "
          f"has {out[0].shape[0]} frames, the ungated {ungated[0].shape[0]}")
    assert rec["state"] == 1 and 0 < rec["open_frames"] < n
    assert out[0].shape[0] < ungated[0].shape[0]                                              # the trim sees the gated tail: shorter
    only = msgpu.render_batch([c2], out_gate=G)[0]                                            # float32, no other rule
    assert only.dtype == np.float32 and np.array_equal(GC.bits(only), GC.bits(gated))
    dev = msgpu.render_batch([c2], results="device", out_gate=G)
    assert np.array_equal(GC.bits(dev[0].cpu().numpy()), GC.bits(only))
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([c2], devices=[0, 1], out_gate=G)


def test_mixed_rates_through_per_rate(eng):
    from msgpu.export import gate_packed
    rates = [48000, 8000, 48000]
    sig = [GC.texture(n, 2, 90 + i) for i, n in enumerate((TILE + 77, 2 * TILE + 1, 999))]
    buf, offs, lens = pack(sig, 2)
    y = eng.torch.from_numpy(buf).cuda()
    gate = GC.OPTIONS["default"]                                                              # 10 ms: 480 frames, or 80
    rec = records(gate_packed(eng, y, offs, lens, rates, gate))
    got = y.cpu().numpy()
    for i, (s, r, o, n) in enumerate(zip(sig, rates, offs, lens)):
        want, want_rec = gate_host(s, r, gate)
        assert np.array_equal(GC.bits(got[o:o + n]), GC.bits(want)) and raw(rec[i]) == want_rec.tobytes()
    assert list(rec["hold_frames"]) == [480, 80, 480]


def test_render_variations_writes_gated_files(c2, tmp_path):
    from msgpu.batch import read_wav_float32
    args = (c2, [1000], [c2["time_unfold"]], [c2["partial_stretch"]])
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_gate=G)
    plain = msgpu.render_batch([msgpu.merged(c2, seed=1000)])[0]
    name, y, rate = got[0]
    want = gate_host(plain, rate, G)[0]
    assert y.shape == plain.shape and np.array_equal(GC.bits(y), GC.bits(want)) and not np.array_equal(y, plain)
    back, sr = read_wav_float32(os.path.join(str(tmp_path), name))
    assert sr == rate and np.array_equal(GC.bits(back), GC.bits(want))
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(*args, devices=[0, 1], export_gate=G)
