"""The stereo rule on the device (msg_stereo_meter, msg_stereo; csrc/kernels_image.h): the meter against the
library's host loop at the tolerances of tests/stereo_cases.py and to the bit alone against in a batch, the
image to the bit against msg_stereo_host in place and folded, the polarity taken from the record on the
device, and the delivery chain with the rule.

profiles/stereo_gpu_tests.txt has the values measured on an MI355X, as these tests print them."""
import math
import os
import struct

import numpy as np
import pytest

import msgpu
import stereo_cases as SC
from msgpu import _lib as L
from msgpu.stereo import STEREO_DTYPE, Stereo, meter_reference, records, stereo_host, stereo_meter_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def lengths(sr):
    hop = sr // 10
    if sr == 4000:
        return [0, 1, hop - 1, 4 * hop - 1, 4 * hop, 4 * hop + 1, 10 * hop + 137]
    return [4096, 4097, 4 * hop, 6 * hop + 1]                      # 48 kHz: a hop is two tiles


def pack(signals, gap=3):
    """The signals back to back with `gap` NaN guard frames around and between them (an odd gap: signals at
    odd frame offsets, 16-byte pieces cut inside a frame pair): (buffer, offsets, lens)."""
    guard = np.full((gap, 2), np.nan, dtype=np.float32)
    offs, lens, parts, at = [], [], [guard], gap
    for s in signals:
        offs.append(at)
        lens.append(len(s))
        parts += [np.asarray(s, dtype=np.float32), guard]
        at += len(s) + gap
    return np.concatenate(parts), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)


def meter(eng, signals, sr, gap=3):
    buf, offs, lens = pack(signals, gap)
    return records(eng.stereo_meter(eng.torch.from_numpy(buf).cuda(), offs, lens, sr))


def record_bits(a):
    """The eight float64 of each record as uint64, (records, 8)."""
    a = np.atleast_1d(a)
    return np.stack([np.asarray(a[k], dtype=np.float64) for k in STEREO_DTYPE.names], axis=-1).view(np.uint64)


def same_records(a, b):
    return np.array_equal(record_bits(a), record_bits(b))


# ---- the meter ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [4000, 48000])
def test_meter_against_host_alone_and_in_a_batch(eng, sr):
    hop = sr // 10
    sig = [SC.hop_noise(n, hop, 100 + i) for i, n in enumerate(lengths(sr))]
    got = meter(eng, sig, sr)
    assert same_records(got, meter(eng, sig, sr))                   # from run to run
    for i, x in enumerate(sig):
        assert SC.separated(meter_reference(x, sr)), i              # the input's own blocks: no tie for the minimum
        host = stereo_meter_host(x, sr)
        SC.check_meter(f"device against host, {sr} Hz, {len(x)} frames", got[i], host)
        assert int(got[i]["blocks"]) == (0 if len(x) < 4 * hop else (len(x) - 4 * hop) // hop + 1)
        for gap in (4, 1):                                          # alone, at another alignment: the same bits
            assert same_records(meter(eng, [x], sr, gap), got[i:i + 1]), (i, gap)
    order = [3, 0, 2, 1] + list(range(4, len(sig)))                 # in another batch: the same bits
    assert same_records(meter(eng, [sig[i] for i in order], sr, 5), got[order])


def test_meter_special_signals_and_refusals(eng):
    sr, hop = 4000, 400
    a = SC.hop_noise(7 * hop + 3, hop, 7)
    same, anti, silent = a.copy(), a.copy(), a.copy()
    same[:, 1] = same[:, 0]
    anti[:, 1] = -anti[:, 0]
    silent[:, 1] = 0.0
    got = meter(eng, [same, anti, silent], sr)
    assert got["corr"][0] == pytest.approx(1.0, abs=1e-12) and got["corr"][1] == pytest.approx(-1.0, abs=1e-12)
    assert got["mono_db"][0] == pytest.approx(0.0, abs=1e-9) and got["mono_db"][1] == -math.inf
    assert got["corr"][2] == 0.0 and got["blocks_kept"][2] == 0 and got["corr_min_block"][2] == -1
    assert got["blocks_kept"][0] == got["blocks"][0] == 4
    x = eng.torch.from_numpy(a).cuda()
    rec = eng.torch.empty((1, 8), dtype=eng.torch.float64, device=x.device)
    off, cnt = np.array([0], dtype=np.int64), np.array([100], dtype=np.int64)
    import ctypes as C
    with pytest.raises(ValueError, match="channels must be 2"):     # a mono signal has no image
        eng._signal_call(L.lib().msg_stereo_meter, x, 1, off, cnt, sr, C.c_void_p(rec.data_ptr()))
    with pytest.raises(ValueError):
        eng.stereo_meter(x, [0], [100], 44101)
    with pytest.raises(ValueError):
        eng.stereo_meter(x, [0], [len(a) + 1], sr)
    assert eng.stereo_meter(x, [], [], sr).shape == (0, 8)
    one = msgpu.stereo_meter(a, sr)                                 # the public function: a host array, a device tensor
    assert same_records(one, meter(eng, [a], sr))
    assert np.array_equal(msgpu.stereo_meter(x, sr).cpu().numpy().view(np.uint64), record_bits(one))


# ---- the image ------------------------------------------------------------------------------------
IMAGES = [Stereo(width=1.3, balance_db=-2.5, swap=True, invert="left"), Stereo(width=0), Stereo(matrix=[[0.3, -1.7], [1e-3, 2.5]])]


def image_signals():
    sig = [SC.hop_noise(n, 400, 200 + i) for i, n in enumerate(lengths(4000) + lengths(48000) + [2 * 4096, 3 * 4096 + 2])]
    return sig + [SC.samples()]                                     # +-0, subnormals, 1e30


@pytest.mark.parametrize("gap", [3, 4], ids=["odd frame offsets", "even frame offsets"])
@pytest.mark.parametrize("stereo", IMAGES, ids=repr)
def test_image_in_place_is_the_host_loop(eng, stereo, gap):
    sig = image_signals()
    buf, offs, lens = pack(sig, gap)
    x = eng.torch.from_numpy(buf).cuda()
    back, off = eng.stereo(x, offs, lens, stereo)
    assert back is x and np.array_equal(off, offs)
    got = x.cpu().numpy()
    inside = np.zeros(len(buf), dtype=bool)
    for s, o, n in zip(sig, offs, lens):
        inside[o:o + n] = True
        assert np.array_equal(SC.bits(got[o:o + n]), SC.bits(stereo_host(s, stereo))), (n, gap)
    assert np.array_equal(SC.bits(got[~inside]), SC.bits(buf[~inside]))           # the NaN guards, bit for bit
    if stereo.width == 0:
        assert np.array_equal(SC.bits(got[inside][:, 0]), SC.bits(got[inside][:, 1]))


@pytest.mark.parametrize("gap", [3, 4], ids=["odd frame offsets", "even frame offsets"])
@pytest.mark.parametrize("shift", [0, 1], ids=["even float offset", "odd float offset"])
def test_fold_is_the_host_loop(eng, gap, shift):
    torch = eng.torch
    sig = image_signals()
    buf, offs, lens = pack(sig, gap)
    x = torch.from_numpy(buf).cuda()
    total = int(lens.sum())
    for stereo in (Stereo(channels=1), Stereo(width=1.3, balance_db=-2.5, swap=True, invert="left", channels=1)):
        room = torch.full((total + shift + 3,), float("nan"), dtype=torch.float32, device=x.device)
        y, y_off = eng.stereo(x, offs, lens, stereo, out=room[shift:])
        assert np.array_equal(y_off, np.cumsum(lens) - lens)
        got = room.cpu().numpy()
        for s, o, n in zip(sig, y_off, lens):
            want = stereo_host(s, stereo)
            assert want.shape == (n, 1)
            assert np.array_equal(SC.bits(got[shift + o:shift + o + n]), SC.bits(want[:, 0])), (n, gap, shift)
        assert np.isnan(got[:shift]).all() and np.isnan(got[shift + total:]).all()     # nothing outside the outputs
        assert np.array_equal(SC.bits(x.cpu().numpy()), SC.bits(buf))                  # the input as it was
    y, y_off = eng.stereo(x, offs, lens, Stereo(channels=1))                           # a tensor of its own
    assert tuple(y.shape) == (total, 1)
    assert np.array_equal(SC.bits(y.cpu().numpy()[:, 0]), SC.bits(np.concatenate([stereo_host(s, Stereo(channels=1))[:, 0]
                                                                                  for s in sig])))


def test_identity_launches_nothing_and_refusals(eng):
    torch = eng.torch
    sig = image_signals()
    buf, offs, lens = pack(sig)
    x = torch.from_numpy(buf).cuda()
    eng.stereo(x, offs, lens, Stereo())
    eng.stereo(x, offs, lens, Stereo(matrix=np.eye(2)))
    assert np.array_equal(SC.bits(x.cpu().numpy()), SC.bits(buf))                      # -0, subnormals and NaN guards as they were
    with pytest.raises(ValueError, match="overlap"):                                   # in place: it writes where it reads
        eng.stereo(x, [0, 100], [200, 200], Stereo(width=0))
    flat = x.view(-1)
    with pytest.raises(ValueError, match="overlap"):                                   # a fold onto its own input
        eng.stereo(x, [0], [200], Stereo(channels=1), out=flat[100:])
    with pytest.raises(ValueError, match="auto"):
        eng.stereo(x, offs, lens, Stereo(invert="auto"))
    with pytest.raises(ValueError):
        eng.stereo(x, [0], [len(buf) + 1], Stereo(width=0))
    with pytest.raises(ValueError):
        eng.stereo(x, offs, lens, Stereo(width=0), rec=torch.zeros((2, 8), dtype=torch.float64, device=x.device))
    assert np.array_equal(SC.bits(x.cpu().numpy()), SC.bits(buf))                      # the refused calls wrote nothing
    eng.stereo(x, [], [], Stereo(width=0))
    import ctypes as C
    m = np.eye(2, dtype=np.float32).reshape(4) * 2
    with pytest.raises(ValueError, match="channels must be 2"):
        eng._signal_call(L.lib().msg_stereo, flat, 1, offs, lens, m.ctypes.data_as(C.c_void_p), None, None, None, None)


# ---- auto polarity --------------------------------------------------------------------------------
def test_auto_polarity_from_the_device_record(eng):
    sr, n = 4000, 6 * 400 + 77
    a = np.random.default_rng(31).standard_normal((3, n, 2)) * 0.2
    sig = [np.stack([v[:, 0], c * v[:, 0] + math.sqrt(1 - c * c) * v[:, 1]], axis=1).astype(np.float32)
           for v, c in zip(a, (0.9, -0.9, -0.2))]
    host = [stereo_meter_host(s, sr) for s in sig]
    print("auto polarity: host corr", [float(h["corr"]) for h in host])
    assert all(abs(h["corr"]) > 1e-3 for h in host) and [h["corr"] < 0 for h in host] == [False, True, True]
    buf, offs, lens = pack(sig)
    for stereo in (Stereo(invert="auto"), Stereo(invert="auto", width=1.5, balance_db=3), Stereo(invert="auto", channels=1)):
        x = eng.torch.from_numpy(buf).cuda()
        rec = eng.stereo_meter(x, offs, lens, sr)
        y, y_off = eng.stereo(x, offs, lens, stereo, rec=rec)                          # nothing returns to the host in between
        got = y.cpu().numpy()
        for s, h, o, k in zip(sig, host, y_off, lens):
            want = stereo_host(s, stereo, rec=h)
            assert np.array_equal(SC.bits(got[o:o + k]), SC.bits(want)), (stereo, float(h["corr"]))
        if stereo == Stereo(invert="auto"):                                            # only the two negative ones, only R
            assert np.array_equal(got[offs[0]:offs[0] + n], sig[0])
            for i in (1, 2):
                seg = got[offs[i]:offs[i] + n]
                assert np.array_equal(seg[:, 0], sig[i][:, 0]) and np.array_equal(seg[:, 1], -sig[i][:, 1])
    repaired = msgpu.stereo(sig[1], sr, Stereo(invert="auto"))                         # the public function measures first
    assert np.array_equal(repaired[:, 1], -sig[1][:, 1]) and msgpu.stereo_meter(repaired, sr)["corr"] > 0.8


# ---- the delivery chain ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(irs):
    return msgpu.config_params("C2", irs=irs, out_dur_s=0.75)


def test_mono_delivery(eng, c2):
    """A mono export is levelled, held, reported and quantised as delivered.  The report is metered on the
    float32 mono render in front of the quantiser; the dequantised words differ from it by at most 1.5 steps
    a sample (TPDF dither of +-1 step and the rounding), and the K-weighting's gain is at most the shelf's
    4 dB (a factor 1.585), so the K-weighted rms moves by at most e = 1.585 x 1.5 x 2^-15 and the level by at
    most 20 log10(1 + e / sqrt(z)), z the report's own mean square 10^((lufs + 0.691) / 10)."""
    sr = int(c2["base_sr"])
    rows = []
    out = msgpu.render_batch([c2], out_stereo=Stereo(channels=1), out_lufs=-23, out_true_peak=-1, out_bits=16, out_report=rows)
    plain = msgpu.render_batch([c2])[0]
    n = plain.shape[0]
    assert len(out) == 1 and out[0].shape == (n, 1) and out[0].dtype == np.int16
    row = rows[0]
    assert float(row["dbtp"]) <= -1.0 + 1e-6 and int(row["frames"]) == n and int(row["rate"]) == sr   # test_gpu_lrange's bar
    back = msgpu.loudness(out[0].astype(np.float32) / np.float32(32768.0), sr)
    z = 10.0 ** ((float(row["lufs"]) + 0.691) / 10.0)
    bar = 20.0 * math.log10(1.0 + 1.585 * 1.5 * 2.0 ** -15 / math.sqrt(z))
    print(f"mono delivery: report {float(row['lufs']):.7f} LUFS {float(row['dbtp']):+.5f} dBTP, dequantised words "
          f"{back:.7f} LUFS, difference {abs(back - float(row['lufs'])):.3e} LU, bar {bar:.3e} LU")
    assert abs(back - float(row["lufs"])) <= bar
    assert abs(float(row["lufs"]) + 23.0) <= 1e-5 or float(row["dbtp"]) >= -1.0 - 1e-3            # at the target or at the ceiling
    # float32, no other rule: the public function on the plain render, to the bit
    mono = msgpu.render_batch([c2], out_stereo=Stereo(channels=1))[0]
    want = msgpu.stereo(plain, sr, Stereo(channels=1))
    assert mono.shape == (n, 1) and mono.dtype == np.float32 and np.array_equal(SC.bits(mono), SC.bits(want))
    assert np.array_equal(SC.bits(want), SC.bits(stereo_host(plain, Stereo(channels=1))))
    dev = msgpu.render_batch([c2], results="device", out_stereo=Stereo(channels=1))
    assert tuple(dev[0].shape) == (n, 1) and np.array_equal(SC.bits(dev[0].cpu().numpy()), SC.bits(want))
    wide = msgpu.render_batch([c2], out_stereo=Stereo(width=1.5))[0]                                # two channels stay two
    assert wide.shape == (n, 2) and np.array_equal(SC.bits(wide), SC.bits(stereo_host(plain, Stereo(width=1.5))))
    # the mono chain step by step: the level rules and the quantiser on the folded render, the same words
    from msgpu.export import loudness_packed, quantize_packed, unpack_all
    t = eng.torch.from_numpy(want).cuda()
    loudness_packed(eng, t, [0], [n], [sr], -23, None, -1, channels=1)
    q, off, nbytes, _ = quantize_packed(eng, t, [0], [n], 16, keys=[0], channels=1)
    assert int(nbytes[0]) == 2 * n                                                                  # half the bytes cross
    assert np.array_equal(unpack_all(q.cpu().numpy(), off, nbytes, 16, channels=1)[0], out[0])
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([c2], devices=[0, 1], out_stereo=Stereo(channels=1))


def test_meter_rows(c2, irs):
    ps = [c2, msgpu.config_params("C2", seed=1001, irs=irs, out_dur_s=0.75)]
    sr = int(c2["base_sr"])
    rows = []
    out = msgpu.render_batch(ps, out_stereo=Stereo(meter=rows))
    plain = msgpu.render_batch(ps)
    assert len(rows) == 2 and all(np.array_equal(SC.bits(a), SC.bits(b)) for a, b in zip(out, plain))   # metering changes no sample
    for row, y in zip(rows, plain):
        want = msgpu.stereo_meter(y, sr)
        print(f"meter row: corr {float(row['corr']):+.6f}, worst 400 ms {float(row['corr_min']):+.6f} at block "
              f"{int(row['corr_min_block'])}, mono {float(row['mono_db']):+.3f} dB, balance {float(row['balance_db']):+.3f} dB")
        assert row.dtype == want.dtype and row.tobytes() == want.tobytes()
    both, rep = [], []
    msgpu.render_batch(ps, out_stereo=Stereo(meter=both, channels=1), out_lufs=-23, out_report=rep)    # read with the report's rows
    assert len(both) == len(rep) == 2 and all(a.tobytes() == b.tobytes() for a, b in zip(both, rows))


def test_mixed_rates_through_per_rate(eng):
    from msgpu.export import stereo_packed
    rates = [48000, 4000, 48000]
    sig = [SC.hop_noise(n, r // 10, 300 + i) for i, (n, r) in enumerate(zip((6 * 4800 + 1, 10 * 400 + 137, 4097), rates))]
    sig[1][:, 1] = -np.abs(sig[1][:, 1]) * np.sign(sig[1][:, 0])                       # one that needs the repair
    buf, offs, lens = pack(sig)
    rows = []
    stereo = Stereo(invert="auto", width=0.5, channels=1, meter=rows)
    y, y_off, ch = stereo_packed(eng, eng.torch.from_numpy(buf).cuda(), offs, lens, rates, stereo)
    got = y.cpu().numpy()
    assert ch == 1 and tuple(y.shape) == (int(lens.sum()), 1) and len(rows) == 3
    for s, r, row, o, n in zip(sig, rates, rows, y_off, lens):
        alone_rows = []
        alone = msgpu.stereo(s, r, Stereo(invert="auto", width=0.5, channels=1, meter=alone_rows))
        assert np.array_equal(SC.bits(got[o:o + n]), SC.bits(alone)) and row.tobytes() == alone_rows[0].tobytes()
    assert rows[1]["corr"] < 0


def test_render_variations_writes_mono_files(c2, tmp_path):
    from msgpu.pcm import read_wav_pcm
    args = (c2, [1000], [c2["time_unfold"]], [c2["partial_stretch"]])
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_stereo=Stereo(channels=1), export_bits=24)
    n = msgpu.render_batch([msgpu.merged(c2, seed=1000)])[0].shape[0]
    name, y, rate = got[0]
    assert y.shape == (n, 1) and y.dtype == np.int32
    with open(os.path.join(str(tmp_path), name), "rb") as fh:
        head = fh.read(44)
    tag, ch, sr, _, align, width = struct.unpack("<HHIIHH", head[20:36])
    assert (tag, ch, sr, align, width) == (1, 1, rate, 3, 24) and head[36:40] == b"data"
    assert struct.unpack("<I", head[40:44])[0] == 3 * n
    q, sr, b = read_wav_pcm(os.path.join(str(tmp_path), name))
    assert q.shape == (n, 1) and b == 24 and np.array_equal(q, y)
    flt = msgpu.render_variations(*args, folder=str(tmp_path), export_stereo=Stereo(channels=1))
    from msgpu.batch import read_wav_float32
    back, sr = read_wav_float32(os.path.join(str(tmp_path), flt[0][0]))
    assert back.shape == (n, 1) and np.array_equal(back, flt[0][1])
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(*args, devices=[0, 1], export_stereo=Stereo(channels=1))
