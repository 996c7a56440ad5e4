"""Device true peak (msg_truepeak / msg_truepeak_gain, csrc/kernels_truepeak.h): to the
bit against the library's host loop (msg_truepeak_host), within E x peak of the float64
reference (msgpu.truepeak.true_peak_reference); the dBTP ceiling of the exports on top
of it.  Signals and bounds: tests/truepeak_cases.py (E = 3.35e-6 from the taps; after a
gain E_GAIN adds the rounding of g and of the scaled samples).  NaN frames lie around
and between the signals of every packed call, so an over-read shows as a NaN record."""
import gc
import math
import os

import numpy as np
import pytest

import loudness_cases as LC
import truepeak_cases as TC
import msgpu
from msgpu.loudness import loudness_reference
from msgpu.loudness import records as loud_records
from msgpu.truepeak import TILE, records, true_peak_host, true_peak_reference

pytestmark = pytest.mark.gpu
GAIN_TOL = 1e-5     # LU after a gain, tests/test_gpu_loudness.py


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def pack(signals, channels, gap=3):
    """The signals back to back with `gap` frames of NaN around and between them (an
    odd gap: mono signals start at odd floats): (buffer, offsets, lens)."""
    offs, lens, parts = [], [], []
    at = gap
    nan = lambda k: np.full((k, 2) if channels == 2 else k, np.nan, dtype=np.float32)
    parts.append(nan(gap))
    for s in signals:
        offs.append(at)
        lens.append(len(s))
        parts += [np.asarray(s, dtype=np.float32), nan(gap)]
        at += len(s) + gap
    return np.concatenate(parts), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)


def measure(eng, signals, channels, sr):
    """(host records, device buffer, offsets, lens, device records) of one msg_truepeak call."""
    buf, offs, lens = pack(signals, channels)
    x = eng.torch.from_numpy(buf).cuda()
    rec = eng.true_peak(x, offs, lens, channels, sr)
    return records(rec), x, offs, lens, rec


def check_all(got, signals, sr, what):
    for r, s in zip(got, signals):
        host = true_peak_host(s, sr)
        assert math.isfinite(r["true_peak"]) and math.isfinite(r["peak"]) and not math.isnan(r["dbtp"])
        ref = TC.check_record(r, s, sr, host=host)
        print(f"{what} n={len(s)} {sr} Hz: device {r['true_peak']:.9f} host {host['true_peak']:.9f} "
              f"reference {ref:.9f} dbtp {r['dbtp']:.6f} os {r['os']}")


# ---- device equals host to the bit --------------------------------------------------------
@pytest.mark.parametrize("sr", [48000, 96000, 384000])
@pytest.mark.parametrize("channels", [1, 2])
def test_device_equals_host(eng, channels, sr):
    sig = [TC.case(n, channels, sr)[0] for n in TC.LENGTHS]
    got = measure(eng, sig, channels, sr)[0]
    check_all(got, sig, sr, f"ragged ch={channels}")


@pytest.mark.parametrize("sr", [48000, 96000])
@pytest.mark.parametrize("channels", [1, 2])
def test_pairs_at_tile_edges(eng, channels, sr):
    """[1, 1] straddling frame 0, a tile boundary and the last frame: the peak between the
    two lies in the halo of one tile or the other."""
    n = 3 * TILE
    sig = [TC.pair_signal(n, at, channels) for at in (0, TILE - 1, 2 * TILE - 1, n - 2)]
    got = measure(eng, sig, channels, sr)[0]
    check_all(got, sig, sr, f"pair ch={channels}")
    assert all(1.26 < r["true_peak"] < 1.28 for r in got)


@pytest.mark.parametrize("channels", [1, 2])
def test_batch_independence(eng, channels):
    sr = 48000
    sig = [TC.case(n, channels, sr)[0] for n in (1, TILE + 1, 13, 0, 20011, 2 * TILE + 1)]
    got, x, offs, lens, _ = measure(eng, sig, channels, sr)
    again = records(eng.true_peak(x, offs, lens, channels, sr))
    assert np.array_equal(got.view(np.uint8), again.view(np.uint8))       # the call repeated: the same bytes
    for i, s in enumerate(sig):                                         # each signal alone: the same bytes
        alone = measure(eng, [s], channels, sr)[0]
        assert np.array_equal(alone.view(np.uint8), got[i:i + 1].view(np.uint8)), i


@pytest.mark.parametrize("sr", [48000, 384000])
def test_nan_is_sticky_on_the_device(eng, sr):
    x = np.array(TC.case(TILE + 1, 2, sr)[0])
    x[TILE - 5, 0] = np.nan
    clean = TC.case(TILE, 2, sr)[0]
    got = measure(eng, [x, clean], 2, sr)[0]
    assert math.isnan(got["peak"][0]) and math.isnan(got["true_peak"][0])
    assert math.isfinite(got["true_peak"][1])


# ---- msgpu.true_peak ---------------------------------------------------------------------------
def test_public_true_peak(eng):
    x = TC.faded_sine()
    host = true_peak_host(x, 48000)
    got = msgpu.true_peak(x, 48000)
    got_db = msgpu.true_peak(x, 48000, db=True)
    print(f"msgpu.true_peak: {got:.9f} ({got_db:+.6f} dBTP), sample peak {host['peak']:.6f}")
    assert isinstance(got, float) and got == host["true_peak"]
    assert isinstance(got_db, float) and got_db == TC.db_exact(got)
    t = eng.torch.from_numpy(np.stack([x, x], axis=1)).cuda()
    y = msgpu.true_peak(t, 48000)
    assert isinstance(y, eng.torch.Tensor) and y.is_cuda and tuple(y.shape) == (1,) and y.dtype == eng.torch.float64
    assert float(y.cpu()[0]) == got
    yd = msgpu.true_peak(t, 48000, db=True)
    assert tuple(yd.shape) == (1,) and float(yd.cpu()[0]) == got_db
    with pytest.raises(ValueError):
        msgpu.true_peak(t, 0)


# ---- gain -------------------------------------------------------------------------------------
def exact_scale(y, plain):
    """The float32 g with y == plain * g sample for sample, or None."""
    k = int(np.argmax(np.abs(plain)))
    q = np.float32(np.float64(y.flat[k]) / np.float64(plain.flat[k]))
    for g in (q, np.nextafter(q, np.float32(0)), np.nextafter(q, np.float32(np.inf))):
        if np.array_equal(plain * g, y):
            return float(g)
    return None


def held_at(y, sr, ceiling, what):
    """The reference true peak of y lies at the ceiling within E_GAIN."""
    tp = true_peak_reference(y, sr)
    rel = tp / ceiling - 1.0
    print(f"{what}: reference true peak {tp:.9f} = {20 * math.log10(tp):+.5f} dBTP, ceiling {ceiling:.9f}, "
          f"off by {rel:+.2e} (bound {TC.E_GAIN:.2e})")
    assert abs(rel) <= TC.E_GAIN


def held(y, ceiling, what):
    held_at(y, 48000, ceiling, what)


def outside_is_nan(y, offs, lens):
    inside = np.zeros(len(y), dtype=bool)
    for o, n in zip(offs, lens):
        inside[o:o + n] = True
    return np.isnan(y[~inside]).all() and not np.isnan(y[inside]).any()


@pytest.mark.parametrize("channels", [1, 2])
def test_gain_ceiling_only(eng, channels):
    s = LC.programme(48000, 2.0, channels, 11)
    ceiling = true_peak_reference(s, 48000) * LC.db(-3.0)
    got, x, offs, lens, rec = measure(eng, [s, s[:5000]], channels, 48000)
    eng.true_peak_gain(x, offs[:1], lens[:1], channels, rec, ceiling_tp=ceiling)
    eng.torch.cuda.synchronize()
    y = x.cpu().numpy()
    after = records(rec)
    out = y[offs[0]:offs[0] + lens[0]]
    g = exact_scale(out, s)
    assert g is not None and g == float(np.float32(after["gain"][0]))      # x (float)g exactly
    assert abs(after["gain"][0] / (ceiling / got["true_peak"][0]) - 1.0) <= 1e-12
    assert after["true_peak"][0] == got["true_peak"][0] and after["peak"][0] == got["peak"][0]
    held(out, ceiling, f"ceiling only ch={channels}")
    assert np.array_equal(y[offs[1]:offs[1] + lens[1]], s[:5000])           # a signal not in the call
    assert outside_is_nan(y, offs, lens)


@pytest.mark.parametrize("channels", [1, 2])
def test_gain_without_a_binding_ceiling_is_loudness_gain(eng, channels):
    s = LC.programme(48000, 2.0, channels, 12)
    ref = LC.check_rule2(s, 48000, -23.0)
    assert LC.db(-23.0 - ref) * true_peak_reference(s, 48000) < 0.9         # the ceiling of 1.0 does not bind
    got, x, offs, lens, rec = measure(eng, [s], channels, 48000)
    x2 = x.clone()
    lrec = eng.loudness(x, offs, lens, channels, 48000)
    lrec2 = lrec.clone()
    eng.true_peak_gain(x, offs, lens, channels, rec, lrec, -23.0, ceiling_tp=1.0)
    eng.loudness_gain(x2, offs, lens, channels, lrec2, -23.0)
    eng.torch.cuda.synchronize()
    a, b = x.cpu().numpy(), x2.cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert records(rec)["gain"][0] == loud_records(lrec2)["gain"][0] == loud_records(lrec)["gain"][0]


@pytest.mark.parametrize("channels", [1, 2])
def test_gain_with_loudness_and_binding_true_peak(eng, channels):
    s = LC.programme(48000, 2.0, channels, 13)
    ref = LC.check_rule2(s, 48000, -14.0)
    ceiling = 0.7 * LC.db(-14.0 - ref) * true_peak_reference(s, 48000)      # under g x true peak: it binds
    got, x, offs, lens, rec = measure(eng, [s], channels, 48000)
    lrec = eng.loudness(x, offs, lens, channels, 48000)
    eng.true_peak_gain(x, offs, lens, channels, rec, lrec, -14.0, ceiling_tp=ceiling)
    eng.torch.cuda.synchronize()
    y = x.cpu().numpy()[offs[0]:offs[0] + lens[0]]
    g = records(rec)["gain"][0]
    lr = loud_records(lrec)
    assert lr["gain"][0] == g and abs(g / (ceiling / got["true_peak"][0]) - 1.0) <= 1e-12
    assert exact_scale(y, s) == float(np.float32(g))
    held(y, ceiling, f"loudness + true-peak ceiling ch={channels}")
    lu = loudness_reference(y, 48000)
    want = float(lr["lufs"][0]) + 20 * math.log10(g)
    print(f"  loudness {lu:.9f} LUFS, expected {want:.9f}")
    assert abs(lu - want) <= GAIN_TOL


@pytest.mark.parametrize("channels", [1, 2])
def test_gain_sample_peak_ceiling_binds_harder(eng, channels):
    s = LC.programme(48000, 2.0, channels, 14)
    ref = LC.check_rule2(s, 48000, -14.0)
    g0 = LC.db(-14.0 - ref)
    peak = float(np.max(np.abs(s)))
    c_tp, c_pk = 0.9 * g0 * true_peak_reference(s, 48000), 0.5 * g0 * peak
    got, x, offs, lens, rec = measure(eng, [s], channels, 48000)
    lrec = eng.loudness(x, offs, lens, channels, 48000)
    eng.true_peak_gain(x, offs, lens, channels, rec, lrec, -14.0, ceiling_tp=c_tp, ceiling_peak=c_pk)
    eng.torch.cuda.synchronize()
    y = x.cpu().numpy()[offs[0]:offs[0] + lens[0]]
    c32 = np.float32(c_pk)
    top = np.float32(np.max(np.abs(y)))
    print(f"sample-peak ceiling {c_pk:.6f} ch={channels}: max|y| {top:.9f}, g {records(rec)['gain'][0]:.9f}")
    assert abs(float(top) - float(c32)) <= float(np.spacing(c32))
    assert abs(records(rec)["gain"][0] / (c_pk / peak) - 1.0) <= 1e-12
    assert true_peak_reference(y, 48000) < c_tp


@pytest.mark.parametrize("channels", [1, 2])
def test_gain_leaves_silence(eng, channels):
    zero = np.zeros((30000, 2) if channels == 2 else 30000, dtype=np.float32)
    quiet = (np.random.default_rng(7).standard_normal(zero.shape) * LC.db(-130.0)).astype(np.float32)
    got, x, offs, lens, rec = measure(eng, [zero, quiet], channels, 48000)
    lrec = eng.loudness(x, offs, lens, channels, 48000)
    eng.true_peak_gain(x, offs, lens, channels, rec, lrec, -23.0, ceiling_tp=0.5, ceiling_peak=0.4)
    eng.torch.cuda.synchronize()
    y = x.cpu().numpy()
    assert got["true_peak"][0] == 0.0 and got["dbtp"][0] == -math.inf
    for i, s in enumerate((zero, quiet)):
        assert np.array_equal(y[offs[i]:offs[i] + lens[i]].view(np.uint32), s.view(np.uint32))
    assert (records(rec)["gain"] == 1.0).all() and (loud_records(lrec)["gain"] == 1.0).all()
    assert outside_is_nan(y, offs, lens)


def test_gain_argument_errors(eng):
    got, x, offs, lens, rec = measure(eng, [TC.case(25, 2, 48000)[0]], 2, 48000)
    with pytest.raises(ValueError):
        eng.true_peak_gain(x, offs, lens, 2, rec, ceiling_tp=0.0)
    with pytest.raises(ValueError):
        eng.true_peak_gain(x, offs, lens, 2, rec, None, -23.0)
    with pytest.raises(ValueError):
        eng.true_peak_gain(x, offs, lens, 2, rec.float(), ceiling_tp=0.5)
    with pytest.raises(ValueError):
        eng.true_peak(x, offs, lens, 2, 0)


# ---- exports ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(irs):
    return msgpu.config_params("C2", irs=irs, out_dur_s=0.75)


def binding_ceiling_db(plains, sr):
    """-1 dBTP where it binds on every render (reference true peak above it by 1e-4 and
    more), else 3 dB under the lowest reference true peak."""
    tps = [true_peak_reference(p, sr) for p in plains]
    c = -1.0 if min(tps) > LC.db(-1.0) * (1 + 1e-4) else 20 * math.log10(min(tps)) - 3.0
    assert all(tp > LC.db(c) * (1 + 1e-4) for tp in tps)
    return c, tps


@pytest.mark.parametrize("export_sr", [None, 48000])
def test_export_true_peak(c2, tmp_path, export_sr):
    from msgpu.batch import read_wav_float32
    args = (c2, [1000, 1001], [c2["time_unfold"]], [c2["partial_stretch"]])
    kw = {} if export_sr is None else {"export_sr": export_sr}
    plain = msgpu.render_variations(*args, **kw)
    sr = export_sr or int(c2["base_sr"])
    c, tps = binding_ceiling_db([p for _, p, _ in plain], sr)
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_true_peak=c, **kw)
    assert len(got) == len(plain) == 2
    for (name, y, rate), (pname, p, _), tp in zip(got, plain, tps):
        assert name == pname and rate == sr and y.shape == p.shape and y.dtype == np.float32
        g = exact_scale(y, p)
        print(f"{name}: plain {20 * math.log10(tp):+.4f} dBTP (sample peak {np.max(np.abs(p)):.4f}), "
              f"ceiling {c:+.2f} dBTP, g {g}")
        assert g is not None and g < 1.0               # one scalar per variant: y = plain * (float)g exactly
        held_at(y, sr, LC.db(c), name)
        wav, wsr = read_wav_float32(os.path.join(str(tmp_path), name))
        assert wsr == sr and np.array_equal(wav, y)
    # with a loudness target under which the ceiling does not bind: the bytes of export_lufs alone
    lufs = msgpu.render_variations(*args, export_lufs=-23.0, **kw)
    both = msgpu.render_variations(*args, export_lufs=-23.0, export_true_peak=-1.0, **kw)
    for (_, a, _), (_, b, _) in zip(lufs, both):
        assert true_peak_reference(a, sr) < LC.db(-1.0) * (1 - 1e-4)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    same = msgpu.render_variations(*args, export_lufs=None, export_ceiling=None, export_true_peak=None, **kw)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for (_, a, _), (_, b, _) in zip(plain, same))


def test_render_batch_out_true_peak(c2, irs):
    torch = __import__("torch")
    ps = [c2, msgpu.config_params("C2", seed=1001, irs=irs, out_dur_s=0.75)]
    sr = int(c2["base_sr"])
    plain = msgpu.render_batch(ps)
    c, _ = binding_ceiling_db(plain, sr)
    dev = msgpu.render_batch(ps, results="device", out_true_peak=c)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev)
    for i, (t, p) in enumerate(zip(dev, plain)):
        y = t.cpu().numpy()
        assert exact_scale(y, p) is not None
        held_at(y, sr, LC.db(c), f"render_batch device {i}")
    p48 = msgpu.render_batch(ps, out_sr=48000)
    c48, _ = binding_ceiling_db(p48, 48000)
    for i, (y, p) in enumerate(zip(msgpu.render_batch(ps, out_sr=48000, out_true_peak=c48), p48)):
        assert exact_scale(y, p) is not None
        held_at(y, 48000, LC.db(c48), f"render_batch out_sr=48000 {i}")
    low = msgpu.render_batch(ps, out_true_peak=c, out_ceiling=0.05)          # the sample-peak ceiling binds harder
    assert all(float(np.max(np.abs(a))) <= 0.05 * (1 + 2.0 ** -23) for a in low)
    same = msgpu.render_batch(ps, out_lufs=None, out_ceiling=None, out_true_peak=None)
    assert all(np.array_equal(a, b) for a, b in zip(plain, same))           # the new argument left None: bit-identical


def test_export_argument_errors(c2):
    with pytest.raises(ValueError):
        msgpu.render_batch([c2], out_sr=48000, out_peak=0.5, out_true_peak=-1.0)
    with pytest.raises(ValueError):
        msgpu.render_batch([c2], results="stats", out_true_peak=-1.0)
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([c2], devices=[0, 1], out_true_peak=-1.0)
    with pytest.raises(ValueError):
        msgpu.render_batch([c2], out_ceiling=0.5)                            # still needs a level rule
    args = (c2, [1000], [1.0], [1.0])
    with pytest.raises(ValueError):
        msgpu.render_variations(*args, export_sr=48000, export_peak="preset", export_true_peak=-1.0)
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(*args, devices=[0, 1], export_true_peak=-1.0)
    with pytest.raises(ValueError):
        msgpu.render_variations(*args, export_ceiling=0.5)


# ---- life cycle ---------------------------------------------------------------------------------
def test_destroy_releases_truepeak_buffers():
    import ctypes as C
    import torch
    from msgpu import _lib as L
    from msgpu.engine import Engine

    def live():
        fn = L.lib().msg_debug_live
        fn.argtypes = [C.POINTER(C.c_int64)]
        fn.restype = C.c_int
        out = (C.c_int64 * 4)()
        assert fn(out) == 0
        return tuple(out)

    gc.collect()
    base = live()
    e = Engine(0)
    x = torch.from_numpy(LC.programme(48000, 1.0, 2, 4)).cuda()
    rec = e.true_peak(x, [0], [x.shape[0]], 2, 48000)
    e.true_peak_gain(x, [0], [x.shape[0]], 2, rec, ceiling_tp=0.2)
    torch.cuda.synchronize()
    assert live()[0] > base[0] and live()[1] > base[1]
    e.close()
    assert live() == base

