"""The compressor on the device (msg_dynamics; csrc/kernels_dynamics.h): samples and records to the
bit against the library's host loop (msg_dynamics_host) at every tile seam, in ragged batches, alone
against in a batch, over 300 tiles, with a poisoned neighbour, and in the delivery chain.

profiles/dynamics_gpu_tests.txt has the values measured on an MI355X, as these tests print them."""
import os

import numpy as np
import pytest

import msgpu
import dynamics_cases as DC
from msgpu.dynamics import DYNAMICS_DTYPE, UNIT, Dynamics, dynamics_host, records
from msgpu.stereo import Stereo

pytestmark = pytest.mark.gpu
SR, TILE = DC.SR, DC.TILE
N3 = 3 * TILE + 5


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


def run(eng, signals, channels, dyn, gap=3, sr=SR):
    """One msg_dynamics call over the packed signals: (buffer before, buffer after, offsets, lens, records)."""
    buf, offs, lens = pack(signals, channels, gap)
    x = eng.torch.from_numpy(buf).cuda()
    rec = eng.dynamics(x, offs, lens, channels, sr, dyn)
    assert tuple(rec.shape) == (len(signals), 4)
    return buf, x.cpu().numpy(), offs, lens, records(rec)


def raw(rec):
    """The record's own fields as bytes (records() adds derived columns)."""
    return np.array([tuple(r[k] for k in DYNAMICS_DTYPE.names) for r in np.atleast_1d(rec)], dtype=DYNAMICS_DTYPE).tobytes()


def check_against_host(eng, signals, channels, dyn, what, gap=3, sr=SR):
    buf, got, offs, lens, rec = run(eng, signals, channels, dyn, gap, sr)
    inside = np.zeros(len(buf), dtype=bool)
    for i, (s, o, n) in enumerate(zip(signals, offs, lens)):
        inside[o:o + n] = True
        want, want_rec = dynamics_host(s, sr, dyn)
        assert np.array_equal(DC.bits(got[o:o + n]), DC.bits(want)), (what, i, int(n))
        assert raw(rec[i]) == want_rec.tobytes(), (what, i, int(n), rec[i], want_rec)
    assert np.array_equal(DC.bits(got[~inside]), DC.bits(buf[~inside])), what      # the NaN guards, bit for bit
    return rec


def seam_signals(channels):
    """Every length at a tile's edges as texture, and a single full-scale frame at frame 0, at both
    sides of the first seam and at the last frame of a signal of three tiles and five frames."""
    sig = [DC.texture(n, channels, 40 + i) for i, n in enumerate(DC.LENGTHS)]
    return sig + [DC.spike(N3, channels, at) for at in (0, TILE - 1, TILE, N3 - 1)]


# ---- device == host to the bit ------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", list(DC.OPTIONS))
def test_device_is_the_host_loop(eng, name, channels):
    """Lengths 0, 1, 2, 4095, 4096, 4097 and 3 x 4096 + 5 and the four peak placements in one ragged
    batch; "slow": the release of a peak at frame 0 crosses every later tile and the attack of a peak at
    the last frame every earlier one; the holds: a peak at 4095 is held across the seam."""
    dyn = DC.OPTIONS[name]
    rec = check_against_host(eng, seam_signals(channels), channels, dyn, name)
    if name == "slow":
        first, last = rec[len(DC.LENGTHS)], rec[-1]
        assert first["reduced_frames"] == N3 and last["reduced_frames"] == N3                # the ramps reach the far end
        assert first["max_e"] == 12 * int(UNIT)                                               # 2/3 of 18 dB over the threshold
        print(f"slow, {channels} ch: a peak at frame 0 and at the last frame reduce all {N3} frames, "
              f"mean {first['mean_reduction_db']:.4f} / {last['mean_reduction_db']:.4f} dB")
    if name == "makeup alone":
        assert np.all(rec["state"][1:] == 1) and np.all(rec["reduced_frames"] == 0) and rec["state"][0] == 0


def test_even_offsets_and_threshold_above_every_sample(eng):
    for channels in (1, 2):
        sig = seam_signals(channels)
        check_against_host(eng, sig, channels, DC.OPTIONS["default"], "even gap", gap=4)
        buf, got, offs, lens, rec = run(eng, sig, channels, Dynamics(threshold_db=0.5, knee_db=0.0))
        assert np.array_equal(DC.bits(got), DC.bits(buf))                                    # nothing is written
        assert np.all(rec["state"] == 0) and np.all(rec["max_e"] == 0)


def test_long_signal_through_the_parallel_tile_scan(eng):
    """300 tiles (two blocks of the scan over tiles), three bursts, a release that takes 100 tiles to
    let go of 12 dB; the attack is as slow."""
    n = 300 * TILE + 123
    x = np.full((n, 2), 1e-4, dtype=np.float32)
    rng = np.random.default_rng(77)
    for at in (5 * TILE + 17, 140 * TILE - 3, 298 * TILE + 4000):
        x[at:at + 300] = (rng.standard_normal((300, 2)) * 0.5).clip(-1, 1)
        x[at + 150] = 1.0
    ms = 1000.0 * (100 * TILE) / SR * 10.0 / 12.0                                             # 12 dB in 100 tiles
    dyn = Dynamics(attack_ms=ms, release_ms=ms)
    rec = check_against_host(eng, [x, x[:TILE + 1]], 2, dyn, "300 tiles")
    print(f"300 tiles: {int(rec[0]['reduced_frames'])} of {n} frames reduced, mean {rec[0]['mean_reduction_db']:.4f} dB, "
          f"max {rec[0]['max_reduction_db']:.4f} dB")
    assert rec[0]["reduced_frames"] > 250 * TILE


@pytest.mark.parametrize("hold", [240, 4096])
def test_held_signal_of_more_tiles_than_are_resident(eng, hold):
    """3000 tiles of dense material with a hold: far more workgroups than the device holds at once (at
    most four a CU at 240 frames, two at 4096), so tiles of sweep 2 start while their neighbours have
    already stored.  The demands of the frames before a tile must be those of the input, not of a
    neighbour's output: the samples and the record are the host loop's."""
    n = 3000 * TILE + 77
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(n, dtype=np.float32) * np.float32(0.3)).clip(-1, 1)
    dyn = Dynamics(threshold_db=-30.0, ratio=8.0, knee_db=6.0, attack_ms=1.0, release_ms=10.0, hold_ms=DC.hold_ms(hold))
    rec = check_against_host(eng, [x], 1, dyn, f"3000 tiles, hold {hold}")
    print(f"3000 tiles, hold {hold}: {int(rec[0]['reduced_frames'])} of {n} frames reduced, mean "
          f"{rec[0]['mean_reduction_db']:.4f} dB")
    assert rec[0]["reduced_frames"] == n


def test_nan_neighbour_and_batch_against_solo(eng):
    for channels in (1, 2):
        sig = [DC.texture(n, channels, 60 + i) for i, n in enumerate((N3, 2 * TILE, TILE + 1, 777, 1))]
        bad = sig[1].copy()
        bad.reshape(-1)[5000] = np.nan
        worse = sig[3].copy()
        worse.reshape(-1)[-1] = np.inf
        batch = [sig[0], bad, sig[2], worse, sig[4]]
        dyn = DC.OPTIONS["hold 100"]
        buf, got, offs, lens, rec = run(eng, batch, channels, dyn)
        for i in (1, 3):                                                                      # as they were, state 2
            assert np.array_equal(DC.bits(got[offs[i]:offs[i] + lens[i]]), DC.bits(batch[i]))
            assert rec[i]["state"] == 2 and rec[i]["max_e"] == 0 and rec[i]["reduced_frames"] == 0
        for i in (0, 2, 4):                                                                   # the neighbours: their solo runs
            for gap in (3, 4):
                _, solo, o, k, solo_rec = run(eng, [batch[i]], channels, dyn, gap)
                assert np.array_equal(DC.bits(solo[o[0]:o[0] + k[0]]), DC.bits(got[offs[i]:offs[i] + lens[i]])), (i, gap)
                assert raw(solo_rec[0]) == raw(rec[i])
        order = [4, 2, 0]                                                                     # another batch: the same bits
        _, again, o2, k2, rec2 = run(eng, [batch[i] for i in order], channels, dyn, 5)
        for j, i in enumerate(order):
            assert np.array_equal(DC.bits(again[o2[j]:o2[j] + k2[j]]), DC.bits(got[offs[i]:offs[i] + lens[i]]))
            assert raw(rec2[j]) == raw(rec[i])


def test_public_function_and_refusals(eng):
    x = DC.texture(TILE + 9, 2, 5)
    dyn = Dynamics(ratio=6.0, makeup_db=2.0)
    want, want_rec = dynamics_host(x, SR, dyn)
    y, rec = msgpu.dynamics(x, SR, dyn)                                                       # NumPy in: a copy and its record
    assert np.array_equal(DC.bits(y), DC.bits(want)) and raw(rec) == want_rec.tobytes() and rec["max_reduction_db"] > 0
    t = eng.torch.from_numpy(x).cuda()
    dev = msgpu.dynamics(t, SR, dyn)                                                          # a tensor in: in place, the device record
    assert np.array_equal(DC.bits(t.cpu().numpy()), DC.bits(want)) and raw(records(dev)[0]) == want_rec.tobytes()
    mono = msgpu.dynamics(x[:, 0].copy(), SR, dyn)[0]
    assert np.array_equal(DC.bits(mono), DC.bits(dynamics_host(x[:, 0].copy(), SR, dyn)[0]))
    before = t.clone()
    with pytest.raises(ValueError, match="overlap"):                                          # it writes where it reads
        eng.dynamics(t, [0, 100], [200, 200], 2, SR, dyn)
    with pytest.raises(ValueError):
        eng.dynamics(t, [0], [len(x) + 1], 2, SR, dyn)
    with pytest.raises(ValueError, match="hold_ms"):
        eng.dynamics(t, [0], [100], 2, SR, Dynamics(hold_ms=DC.hold_ms(4097)))
    with pytest.raises(ValueError, match="ratio"):
        msgpu.dynamics(x, SR, Dynamics(ratio=0.5))
    assert eng.torch.equal(before, t)                                                         # the refused calls wrote nothing
    assert tuple(eng.dynamics(t, [], [], 2, SR, dyn).shape) == (0, 4)


# ---- the delivery chain -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(irs):
    return msgpu.config_params("C2", irs=irs, out_dur_s=0.75)


D = Dynamics(threshold_db=-30.0, ratio=4.0, knee_db=6.0, attack_ms=2.0, release_ms=60.0, hold_ms=5.0, makeup_db=3.0)


def test_chain_equals_the_rules_by_hand(eng, c2):
    from msgpu.export import loudness_packed, quantize_packed, unpack_all
    sr = int(c2["base_sr"])
    rows, plain_rows = [], []
    out = msgpu.render_batch([c2], out_dynamics=D, out_lufs=-23, out_true_peak=-1, out_bits=16, out_report=rows)
    msgpu.render_batch([c2], out_lufs=-23, out_true_peak=-1, out_bits=16, out_report=plain_rows)
    plain = msgpu.render_batch([c2])[0]
    n = plain.shape[0]
    assert len(out) == 1 and out[0].shape == (n, 2) and out[0].dtype == np.int16
    t = eng.torch.from_numpy(plain).cuda()
    rec = records(msgpu.dynamics(t, sr, D))[0]                                                # the public function, in place
    assert np.array_equal(DC.bits(t.cpu().numpy()), DC.bits(dynamics_host(plain, sr, D)[0]))
    loudness_packed(eng, t, [0], [n], [sr], -23, None, -1)
    q, off, nbytes, _ = quantize_packed(eng, t, [0], [n], 16, keys=[0])
    assert np.array_equal(unpack_all(q.cpu().numpy(), off, nbytes, 16)[0], out[0])
    print(f"chain: {int(rec['reduced_frames'])} of {n} frames reduced, max {rec['max_reduction_db']:.3f} dB, report "
          f"{float(rows[0]['lufs']):.4f} LUFS {float(rows[0]['dbtp']):+.4f} dBTP, LRA {float(rows[0]['lra']):.4f} LU "
          f"against {float(plain_rows[0]['lra']):.4f} LU without the rule")
    assert rec["state"] == 1 and rec["reduced_frames"] > 0
    assert float(rows[0]["lra"]) <= float(plain_rows[0]["lra"])      # 0.75 s have no short-term window: both are 0, and
    #                                                                   test_report_shows_the_loudness_range_come_down has the range
    only = msgpu.render_batch([c2], out_dynamics=D)[0]                                        # float32, no other rule
    assert only.dtype == np.float32 and np.array_equal(DC.bits(only), DC.bits(dynamics_host(plain, sr, D)[0]))
    dev = msgpu.render_batch([c2], results="device", out_dynamics=D)
    assert np.array_equal(DC.bits(dev[0].cpu().numpy()), DC.bits(only))
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([c2], devices=[0, 1], out_dynamics=D)


def test_report_shows_the_loudness_range_come_down(eng):
    """The chain on 24 s of noise whose level steps between -14 and -29 dBFS rms every 6 s: both levels
    pass the meter's relative gate, so the report without the rule reads an LRA near the step; with a 4:1
    compressor from -40 dB the envelope rides the peaks of either level, 20 dB and more above the threshold,
    so the step shrinks to about a quarter and the reported LRA with it."""
    from msgpu.export import Delivery, deliver
    sr, n = 48000, 24 * 48000
    rng = np.random.default_rng(9)
    level = np.where((np.arange(n) // (6 * sr)) % 2 == 0, 10.0 ** (-14.0 / 20.0), 10.0 ** (-29.0 / 20.0))
    x = (rng.standard_normal((n, 2)) * level[:, None]).clip(-1, 1).astype(np.float32)
    dyn = Dynamics(threshold_db=-40.0, ratio=4.0, knee_db=0.0, attack_ms=5.0, release_ms=150.0, makeup_db=6.0)
    lra = {}
    for name, rule in (("plain", None), ("compressed", dyn)):
        d = Delivery(lufs=-23.0, true_peak=-1.0, report=[], dynamics=rule)
        deliver(eng, eng.torch.from_numpy(x).cuda(), [0], [n], [sr], d)
        eng.torch.cuda.synchronize()
        d.flush_report()
        lra[name] = float(d.report[0]["lra"])
    print(f"report: LRA {lra['plain']:.3f} LU without the rule, {lra['compressed']:.3f} LU with it")
    assert lra["plain"] > 10.0                                                                # the step is 15 dB
    assert lra["compressed"] < 0.5 * lra["plain"]                                             # and a quarter of it is left


def test_mono_fold_is_compressed_as_delivered(eng, c2):
    from msgpu.export import loudness_packed
    sr = int(c2["base_sr"])
    out = msgpu.render_batch([c2], out_stereo=Stereo(channels=1), out_dynamics=D, out_lufs=-23, out_true_peak=-1)[0]
    plain = msgpu.render_batch([c2])[0]
    n = plain.shape[0]
    fold = msgpu.stereo(plain, sr, Stereo(channels=1))
    assert out.shape == (n, 1) and out.dtype == np.float32 and fold.shape == (n, 1)
    t = eng.torch.from_numpy(fold).cuda()
    msgpu.dynamics(t, sr, D)
    assert np.array_equal(DC.bits(t.cpu().numpy()[:, 0]), DC.bits(dynamics_host(fold[:, 0].copy(), sr, D)[0]))
    loudness_packed(eng, t, [0], [n], [sr], -23, None, -1, channels=1)
    assert np.array_equal(DC.bits(t.cpu().numpy()), DC.bits(out))


def test_mixed_rates_through_per_rate(eng):
    from msgpu.export import dynamics_packed
    rates = [48000, 8000, 48000]
    sig = [DC.texture(n, 2, 90 + i) for i, n in enumerate((TILE + 77, 2 * TILE + 1, 999))]
    buf, offs, lens = pack(sig, 2)
    y = eng.torch.from_numpy(buf).cuda()
    dyn = Dynamics(hold_ms=10.0)                                                              # 480 frames, or 80
    rec = records(dynamics_packed(eng, y, offs, lens, rates, dyn))
    got = y.cpu().numpy()
    for i, (s, r, o, n) in enumerate(zip(sig, rates, offs, lens)):
        want, want_rec = dynamics_host(s, r, dyn)
        assert np.array_equal(DC.bits(got[o:o + n]), DC.bits(want)) and raw(rec[i]) == want_rec.tobytes()
    assert list(rec["hold_frames"]) == [480, 80, 480]


def test_render_variations_writes_compressed_files(c2, tmp_path):
    from msgpu.batch import read_wav_float32
    args = (c2, [1000], [c2["time_unfold"]], [c2["partial_stretch"]])
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_dynamics=D)
    plain = msgpu.render_batch([msgpu.merged(c2, seed=1000)])[0]
    name, y, rate = got[0]
    want = dynamics_host(plain, rate, D)[0]
    assert y.shape == plain.shape and np.array_equal(DC.bits(y), DC.bits(want)) and not np.array_equal(y, plain)
    back, sr = read_wav_float32(os.path.join(str(tmp_path), name))
    assert sr == rate and np.array_equal(DC.bits(back), DC.bits(want))
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(*args, devices=[0, 1], export_dynamics=D)
