"""The delivery filter on the device (msg_filter, csrc/kernels_filter.h) against scipy.signal.sosfilt in
float64 on the same float32 input, over ragged batches of the signals and cascades of
tests/filter_cases.py: one call per option set, mono signals at odd float offsets, NaN guard frames
between the signals that must come back as they were.  The bar is filter_cases.check_against: with
e32 = rms(float32(ref) - ref), rms(out - ref) <= 2 e32 per signal.  Then determinism, NaN isolation,
zero phase and the delivery chain with the new rule.

profiles/filter_gpu_tests.txt has the values measured on an MI355X, as these tests print them."""
import numpy as np
import pytest

import filter_cases as FC
import msgpu
from msgpu.filter import Filter, filter_host, sos_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def pack(signals, channels, gap=3):
    """The signals back to back with `gap` NaN guard frames around and between them (an odd gap: mono
    signals start at odd floats): (buffer, offsets, lens)."""
    guard = np.full((gap, 2) if channels == 2 else gap, np.nan, dtype=np.float32)
    offs, lens, parts, at = [], [], [guard], gap
    for s in signals:
        offs.append(at)
        lens.append(len(s))
        parts += [np.asarray(s, dtype=np.float32), guard]
        at += len(s) + gap
    return np.concatenate(parts), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)


def run(eng, buf, offs, lens, channels, sr, flt, reverse=False):
    x = eng.torch.from_numpy(buf).cuda()
    eng.filter(x, offs, lens, channels, sr, flt, reverse=reverse)
    return x.cpu().numpy()


_BATCH = {}


def batch(eng, name, channels, reverse):
    """One ragged call of an option set, computed once: (named signals, buffer, offsets, lens, output)."""
    key = (name, channels, reverse)
    if key not in _BATCH:
        flt, sr = FC.FILTERS[name]
        named = FC.signals(channels)
        buf, offs, lens = pack([x for _, x in named], channels)
        _BATCH[key] = (named, buf, offs, lens, run(eng, buf, offs, lens, channels, sr, flt, reverse))
    return _BATCH[key]


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", FC.DEVICE_SETS)
def test_ragged_batch_against_sosfilt(eng, name, channels, reverse):
    """Every length (0, 1, 2, 15, 16, 17, T - 1, T, T + 1, 3 T + 5), the impulses at the chunk, wave and
    tile seams and the conditioning case in one call; the guards keep their bits."""
    flt, sr = FC.FILTERS[name]
    sos = flt.design(sr)
    named, buf, offs, lens, got = batch(eng, name, channels, reverse)
    inside = np.zeros(len(buf), dtype=bool)
    for (label, x), o, n in zip(named, offs, lens):
        out = got[o:o + n]
        inside[o:o + n] = True
        err, bar = FC.check_against(f"{name} / {label} ch={channels} rev={reverse}", out, sos_reference(x, sos, reverse))
        host = FC.rms(filter_host(x, sr, flt, reverse).astype(np.float64) - sos_reference(x, sos, reverse))
        line = (f"{name:24s} {label:18s} ch={channels} {'reverse' if reverse else 'forward'}: rms error {err:.4e}  "
                f"e32 {bar:.4e}  ratio {err / bar if bar else 0.0:.4f}  host loop {host:.4e}")
        print(line)
    assert np.array_equal(FC.bits(got[~inside]), FC.bits(buf[~inside]))           # the NaN guards, bit for bit


@pytest.mark.parametrize("channels", [1, 2])
def test_alone_is_in_the_batch_and_runs_repeat(eng, channels):
    """Each signal filtered alone gives the bits it gives in the batch, and two runs give the same bits."""
    for name in ("hp4 20 Hz @ 384k", "eight sections @ 48k"):
        flt, sr = FC.FILTERS[name]
        for reverse in (False, True):
            named, buf, offs, lens, got = batch(eng, name, channels, reverse)
            again = run(eng, buf, offs, lens, channels, sr, flt, reverse)
            assert np.array_equal(FC.bits(again), FC.bits(got))
            for (label, x), o, n in zip(named, offs, lens):
                if n in (0, 2, 16) or label.startswith("impulse") and "at 16" not in label:
                    continue                                                      # a few of each kind are enough
                one, o1, n1 = pack([x], channels, gap=4)                          # another alignment, too
                alone = run(eng, one, o1, n1, channels, sr, flt, reverse)[o1[0]:o1[0] + n]
                assert np.array_equal(FC.bits(alone), FC.bits(got[o:o + n])), (name, label, reverse)


def test_nan_poisons_its_own_channel_from_its_frame_on(eng):
    flt, sr = FC.FILTERS["eight sections @ 48k"]
    x = FC.noise(FC.N_LONG, 2, 41)
    bad = x.copy()
    bad[FC.T, 0] = np.nan
    inf = x.copy()
    inf[FC.T + 17, 1] = np.inf
    buf, offs, lens = pack([x, bad, inf, x], 2)
    got = run(eng, buf, offs, lens, 2, sr, flt)
    clean, b, i, last = (got[o:o + n] for o, n in zip(offs, lens))
    assert np.isfinite(clean).all() and np.array_equal(FC.bits(clean), FC.bits(last))
    assert np.array_equal(FC.bits(b[:, 1]), FC.bits(clean[:, 1]))                 # R: untouched
    assert np.array_equal(FC.bits(b[:FC.T, 0]), FC.bits(clean[:FC.T, 0]))         # L before the NaN
    assert np.isnan(b[FC.T:, 0]).all()
    assert np.array_equal(FC.bits(i[:, 0]), FC.bits(clean[:, 0]))
    assert np.array_equal(FC.bits(i[:FC.T + 17, 1]), FC.bits(clean[:FC.T + 17, 1]))
    assert not np.isfinite(i[FC.T + 17:, 1]).any()
    # the reverse run: from its frame on is towards the first frame
    rev = run(eng, buf, offs, lens, 2, sr, flt, reverse=True)
    clean, b = rev[offs[0]:offs[0] + lens[0]], rev[offs[1]:offs[1] + lens[1]]
    assert np.array_equal(FC.bits(b[:, 1]), FC.bits(clean[:, 1]))
    assert np.array_equal(FC.bits(b[FC.T + 1:, 0]), FC.bits(clean[FC.T + 1:, 0])) and np.isnan(b[:FC.T + 1, 0]).all()


@pytest.mark.parametrize("channels", [1, 2])
def test_zero_phase_is_forward_then_reverse(eng, channels):
    hp = Filter(highpass=(20, 4))
    zp = Filter(highpass=(20, 4), zero_phase=True)
    buf, offs, lens = pack([x for _, x in FC.signals(channels)], channels)
    x = eng.torch.from_numpy(buf).cuda()
    eng.filter(x, offs, lens, channels, 48000, hp)
    eng.filter(x, offs, lens, channels, 48000, hp, reverse=True)
    two = x.cpu().numpy()
    assert np.array_equal(FC.bits(run(eng, buf, offs, lens, channels, 48000, zp)), FC.bits(two))
    s = FC.noise(FC.N_LONG, channels, 9)
    y = msgpu.filter(s, 48000, zp)                                                # the public function, a host array
    assert y.dtype == np.float32 and y.shape == s.shape
    assert np.array_equal(FC.bits(y), FC.bits(msgpu.filter(msgpu.filter(s, 48000, hp), 48000, hp, reverse=True)))
    # each run against its own reference: the second one's input is the first one's float32 output
    first = msgpu.filter(s, 48000, hp)
    FC.check_against("zero phase, second run", y, sos_reference(first, hp.design(48000), True))


def test_public_function_and_refusals(eng):
    flt, sr = FC.FILTERS["hp2 20 Hz @ 48k"]
    s = FC.noise(FC.T + 1, 2, 11)
    t = eng.torch.from_numpy(s).cuda()
    back = msgpu.filter(t, sr, flt)                                               # a device tensor: in place
    assert back is t
    assert np.array_equal(FC.bits(t.cpu().numpy()), FC.bits(msgpu.filter(s, sr, flt)))
    with pytest.raises(ValueError):
        eng.filter(t, [0], [FC.T + 2], 2, sr, flt)
    with pytest.raises(ValueError, match="overlap"):                              # it writes where it reads
        eng.filter(t, [0, 100], [200, 200], 2, sr, flt)
    with pytest.raises(ValueError):
        eng.filter(t, [0], [100], 2, sr, Filter(sos=[[1, 0, 0, 1, 0, 1.0]]))
    assert np.array_equal(FC.bits(t.cpu().numpy()), FC.bits(msgpu.filter(s, sr, flt)))   # the refused calls wrote nothing
    eng.filter(t, [], [], 2, sr, flt)


# ---- the delivery chain -------------------------------------------------------------------------
def test_render_batch_with_a_filter(eng, irs):
    """The chain with the rule equals, to the bit, the same chain run step by step: msgpu.resample,
    msgpu.filter and the existing passes; its report reads -23 LUFS."""
    from msgpu.export import Delivery, deliver, unpack_all
    hp = Filter(highpass=(20, 4))
    ps = [msgpu.config_params("C2", seed=1000, irs=irs)]
    rep = []
    out = msgpu.render_batch(ps, out_sr=48000, out_filter=hp, out_lufs=-23, out_true_peak=-1, out_bits=16,
                             out_report=rep)
    plain = msgpu.render_batch(ps)[0]
    sr_in = int(msgpu.merged(ps[0])["base_sr"])
    y = msgpu.filter(msgpu.resample(plain, sr_in, 48000), 48000, hp)
    assert not np.array_equal(y, msgpu.resample(plain, sr_in, 48000))
    t = eng.torch.from_numpy(y).cuda()
    q, off, nbytes, _ = deliver(eng, t, [0], [len(y)], [48000], Delivery(lufs=-23, true_peak=-1, bits=16), None, [0])
    eng.torch.cuda.synchronize(eng.device)
    steps = unpack_all(q.cpu().numpy(), off, nbytes, 16)[0]
    assert out[0].dtype == np.int16 and out[0].shape == steps.shape and np.array_equal(out[0], steps)
    line = (f"chain: C2 at 48 kHz, hp4 20 Hz, -23 LUFS / -1 dBTP / 16 bits: report {float(rep[0]['lufs']):.7f} LUFS, "
            f"{float(rep[0]['dbtp']):+.4f} dBTP, {int(rep[0]['frames'])} frames")
    print(line)
    assert abs(float(rep[0]["lufs"]) + 23.0) <= 1e-5                              # test_gpu_loudness.GAIN_TOL
    with pytest.raises(NotImplementedError):
        msgpu.render_batch(ps, devices=[0, 1], out_filter=hp)


def test_render_variations_with_a_filter(irs):
    hp = Filter(highpass=(20, 4))
    c2 = msgpu.config_params("C2", irs=irs)
    args = (c2, [1000], [c2["time_unfold"]], [c2["partial_stretch"]])
    got = msgpu.render_variations(*args, export_sr=48000, export_lufs=-23, export_true_peak=-1, export_bits=16,
                                  export_filter=hp)
    want = msgpu.render_batch([msgpu.config_params("C2", seed=1000, irs=irs)], out_sr=48000, out_lufs=-23,
                              out_true_peak=-1, out_bits=16, out_filter=hp)
    assert np.array_equal(got[0][1], want[0])
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(*args, devices=[0, 1], export_filter=hp)
