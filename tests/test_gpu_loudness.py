"""Device loudness (msg_loudness / msg_loudness_gain, csrc/kernels_loudness.h) against
the float64 reference (msgpu.loudness.loudness_reference) at 1e-6 LU and against the
library's host loop (msg_loudness_host); the LUFS-normalised exports on top of it.
Signals and input rules: tests/loudness_cases.py.

Bars.  1e-6 LU against the reference: float64 on both sides over the same float32
samples (tests/test_loudness_host.py).  1e-5 LU after a gain: rounding g to float32
moves the level by at most 20 log10(1 + 2^-24) = 5.2e-7 dB and the rounding of the
scaled samples averages out."""
import gc
import math
import os

import numpy as np
import pytest

import loudness_cases as LC
import msgpu
from msgpu.loudness import TILE, loudness_host, loudness_reference, records

pytestmark = pytest.mark.gpu
GAIN_TOL = 1e-5
HOP = 4800          # 48 kHz


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
    """(host records, device buffer, offsets, lens, device records) of one msg_loudness call."""
    buf, offs, lens = pack(signals, channels)
    x = eng.torch.from_numpy(buf).cuda()
    rec = eng.loudness(x, offs, lens, channels, sr)
    return records(rec), x, offs, lens, rec


def noise(n, channels, seed, level_db=-20.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 2) if channels == 2 else n) * LC.db(level_db)).astype(np.float32)


def check_against_reference(r, x, sr):
    ref = loudness_reference(x, sr)
    host = loudness_host(x, sr)
    assert LC.close_lu(float(r["lufs"]), ref), (float(r["lufs"]), ref)
    assert LC.close_lu(float(r["lufs"]), float(host["lufs"]))
    assert r["n_blocks"] == host["n_blocks"] and r["n_kept"] == host["n_kept"]
    assert r["peak"] == host["peak"] and r["gain"] == 0.0
    if math.isinf(ref):
        assert r["mean_sq"] == 0.0
    else:
        assert abs(r["mean_sq"] / host["mean_sq"] - 1.0) <= 2.3e-7
    return ref


# ---- the CPU signals again, through msgpu.loudness ------------------------------------
DEVICE_CASES = [(f"sine:{d}", sr) for d in (-23.0, -33.0) for sr in LC.RATES] + \
               [(n, sr) for n, rates in LC.CPU_CASES for sr in rates] + [("dc", 384000)]


@pytest.mark.parametrize("name,sr", DEVICE_CASES)
def test_cpu_signals_on_device(name, sr):
    x, ref = LC.case(name, sr)
    got = msgpu.loudness(np.asarray(x), sr)
    host = float(loudness_host(x, sr)["lufs"])
    print(f"{name} at {sr} Hz: device {got:.9f} reference {ref:.9f} host {host:.9f} diff {got - ref:.2e}")
    assert isinstance(got, float)
    assert LC.close_lu(got, ref)
    assert LC.close_lu(got, host)
    if name.startswith("sine"):
        assert abs(got - float(name.split(":")[1])) <= 0.1


def test_device_tensor_in_device_tensor_out(eng):
    x, ref = LC.case("noise:2", 48000)
    t = eng.torch.from_numpy(np.array(x)).cuda()
    y = msgpu.loudness(t, 48000)
    assert isinstance(y, eng.torch.Tensor) and y.is_cuda and tuple(y.shape) == (1,) and y.dtype == eng.torch.float64
    assert LC.close_lu(float(y.cpu()[0]), ref)
    with pytest.raises(ValueError):
        msgpu.loudness(t, 11025)


# ---- tile and hop edges -----------------------------------------------------------------
def edge_lengths():
    return [k * TILE + d for k in (1, 2) for d in (-1, 0, 1)] + [m * HOP + d for m in (4, 5, 9) for d in (-1, 1)]


@pytest.mark.parametrize("channels", [1, 2])
def test_tile_and_hop_edges(eng, channels):
    """Lengths either side of one and two tiles (shorter than four hops: no block, the
    peak alone) and of 4, 5 and 9 hops, one signal each of a ragged call."""
    sig = [noise(n, channels, 100 + i) for i, n in enumerate(edge_lengths())]
    for s in sig:
        LC.check_rule1(s, 48000)
    got = measure(eng, sig, channels, 48000)[0]
    for r, s in zip(got, sig):
        ref = check_against_reference(r, s, 48000)
        print(f"n={len(s)} ch={channels}: device {r['lufs']:.9f} reference {ref:.9f} blocks {r['n_blocks']}")
        assert r["n_blocks"] == (0 if len(s) < 4 * HOP else (len(s) - 4 * HOP) // HOP + 1)


def impulse_signals(channels):
    """Unit impulses one frame either side of a tile boundary inside a hop (frame TILE of
    hop 0 and of hop 2) and of the hop boundary: the tail that crosses the boundary
    carries the block's energy, so a wrong state hand-over shows at once."""
    n = 6 * HOP
    out = []
    for at in (TILE - 1, TILE, 2 * HOP + TILE - 1, 2 * HOP + TILE, HOP - 1, HOP):
        x = np.zeros((n, 2) if channels == 2 else n, dtype=np.float32)
        if channels == 2:
            x[at] = (1.0, -0.5)
        else:
            x[at] = 1.0
        out.append(x)
    return out


@pytest.mark.parametrize("channels", [1, 2])
def test_impulses_at_tile_boundaries(eng, channels):
    sig = impulse_signals(channels)
    for s in sig:
        LC.check_rule1(s, 48000)
    got = measure(eng, sig, channels, 48000)[0]
    for r, s in zip(got, sig):
        ref = check_against_reference(r, s, 48000)
        assert math.isfinite(ref)
        print(f"impulse ch={channels}: device {r['lufs']:.9f} reference {ref:.9f}")


# ---- ragged batch -----------------------------------------------------------------------
RAGGED = [1, 4097, 30001, 8, 52345, 0, 240000]


@pytest.mark.parametrize("channels", [1, 2])
def test_ragged_batch(eng, channels):
    sig = [noise(n, channels, 200 + i, -18.0 - i) for i, n in enumerate(RAGGED)]
    for s in sig:
        LC.check_rule1(s, 48000)
    got, x, offs, lens, _ = measure(eng, sig, channels, 48000)
    for r, s in zip(got, sig):
        ref = check_against_reference(r, s, 48000)        # NaN around the signals: an over-read poisons a record
        assert math.isfinite(r["lufs"]) or r["lufs"] == -math.inf
        assert math.isfinite(r["mean_sq"]) and math.isfinite(r["peak"])
        assert r["peak"] == (float(np.max(np.abs(s))) if len(s) else 0.0)
        print(f"ragged n={len(s)} ch={channels}: {r['lufs']:.9f} reference {ref:.9f}")
    again = records(eng.loudness(x, offs, lens, channels, 48000))
    assert np.array_equal(got.view(np.uint8), again.view(np.uint8))       # the call repeated: the same bytes
    for i, s in enumerate(sig):                                         # each signal alone: the same bytes
        alone = measure(eng, [s], channels, 48000)[0]
        assert np.array_equal(alone.view(np.uint8), got[i:i + 1].view(np.uint8)), i


# ---- gain -------------------------------------------------------------------------------
def gain_signals(channels):
    silent = noise(30000, channels, 7, -130.0)
    return [LC.programme(48000, 2.0, channels, 1), silent, LC.programme(48000, 1.3, channels, 2)]


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("target", [-23.0, -14.0])
def test_gain_to_target(eng, channels, target):
    sig = gain_signals(channels)
    assert loudness_reference(sig[1], 48000) == -math.inf
    refs = [LC.check_rule2(s, 48000, target) for s in (sig[0], sig[2])]
    got, x, offs, lens, rec = measure(eng, sig, channels, 48000)
    eng.loudness_gain(x, offs, lens, channels, rec, target)
    eng.torch.cuda.synchronize()
    y = x.cpu().numpy()
    after = records(rec)
    for i, ref in zip((0, 2), refs):
        out = y[offs[i]:offs[i] + lens[i]]
        lu = loudness_reference(out, 48000)
        print(f"gain to {target} ch={channels}: was {ref:.6f}, now {lu:.9f}, g {after['gain'][i]:.9f}")
        assert abs(lu - target) <= GAIN_TOL
        assert abs(after["gain"][i] / LC.db(target - got["lufs"][i]) - 1.0) <= 1e-12
        assert after["lufs"][i] == got["lufs"][i] and after["peak"][i] == got["peak"][i]
    quiet = y[offs[1]:offs[1] + lens[1]]
    assert after["gain"][1] == 1.0
    assert np.array_equal(quiet.view(np.uint32), sig[1].view(np.uint32))     # a silent signal: bit for bit
    assert np.isnan(y[:offs[0]]).all() and np.isnan(y[offs[0] + lens[0]:offs[1]]).all()   # nothing outside


@pytest.mark.parametrize("channels", [1, 2])
def test_gain_ceiling_binds(eng, channels):
    s = LC.programme(48000, 2.0, channels, 3)
    ref = LC.check_rule2(s, 48000, -14.0)
    peak = float(np.max(np.abs(s)))
    ceiling = 0.8 * peak * LC.db(-14.0 - ref)                   # under g * peak: the ceiling binds
    assert ceiling > 0 and abs(20 * math.log10(ceiling / peak)) <= 15.0
    got, x, offs, lens, rec = measure(eng, [s], channels, 48000)
    eng.loudness_gain(x, offs, lens, channels, rec, -14.0, ceiling)
    eng.torch.cuda.synchronize()
    y = x.cpu().numpy()[offs[0]:offs[0] + lens[0]]
    c32 = np.float32(ceiling)
    top = np.float32(np.max(np.abs(y)))
    lu = loudness_reference(y, 48000)
    want = ref + 20 * math.log10(ceiling / peak)
    print(f"ceiling {ceiling:.6f} ch={channels}: max|y| {top:.9f}, {lu:.9f} LUFS, expected {want:.9f}")
    assert abs(float(top) - float(c32)) <= float(np.spacing(c32))
    assert abs(lu - want) <= GAIN_TOL
    assert abs(records(rec)["gain"][0] / (ceiling / peak) - 1.0) <= 1e-12


# ---- exports ----------------------------------------------------------------------------
def exact_scale(y, plain):
    """The float32 g with y == plain * g sample for sample, or None."""
    k = int(np.argmax(np.abs(plain)))
    q = np.float32(np.float64(y.flat[k]) / np.float64(plain.flat[k]))
    for g in (q, np.nextafter(q, np.float32(0)), np.nextafter(q, np.float32(np.inf))):
        if np.array_equal(plain * g, y):
            return float(g)
    return None


@pytest.fixture(scope="module")
def c2(irs):
    return msgpu.config_params("C2", irs=irs, out_dur_s=0.75)


@pytest.mark.parametrize("export_sr", [None, 48000])
def test_export_lufs(c2, tmp_path, export_sr):
    from msgpu.batch import read_wav_float32
    args = (c2, [1000, 1001], [c2["time_unfold"]], [c2["partial_stretch"]])
    kw = {} if export_sr is None else {"export_sr": export_sr}
    plain = msgpu.render_variations(*args, **kw)
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_lufs=-23.0, **kw)
    sr = export_sr or int(c2["base_sr"])
    assert len(got) == len(plain) == 2
    for (name, y, rate), (pname, p, _) in zip(got, plain):
        assert name == pname and rate == sr and y.shape == p.shape and y.dtype == np.float32
        LC.check_export_shift(p, sr, -23.0)
        lu = loudness_reference(y, sr)
        g = exact_scale(y, p)
        print(f"{name}: {lu:.9f} LUFS, g {g}")
        assert abs(lu + 23.0) <= GAIN_TOL
        assert g is not None                       # one scalar per variant: y = plain * (float)g exactly
        wav, wsr = read_wav_float32(os.path.join(str(tmp_path), name))
        assert wsr == sr and np.array_equal(wav, y)


def test_render_batch_out_lufs(c2, irs):
    torch = __import__("torch")
    ps = [c2, msgpu.config_params("C2", seed=1001, irs=irs, out_dur_s=0.75)]
    dev = msgpu.render_batch(ps, results="device", out_lufs=-16.0)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in dev)
    plain = msgpu.render_batch(ps)
    for t, p in zip(dev, plain):
        LC.check_rule2(p, int(c2["base_sr"]), -16.0)
        assert abs(loudness_reference(t.cpu().numpy(), int(c2["base_sr"])) + 16.0) <= GAIN_TOL
    held = msgpu.render_batch(ps, out_sr=48000, out_lufs=-16.0, out_ceiling=0.05)
    assert all(float(np.max(np.abs(a))) <= 0.05 * (1 + 2.0 ** -23) for a in held)
    same = msgpu.render_batch(ps, out_lufs=None, out_ceiling=None)
    assert all(np.array_equal(a, b) for a, b in zip(plain, same))     # the new arguments left None: bit-identical


def test_export_argument_errors(c2):
    with pytest.raises(ValueError):
        msgpu.render_batch([c2], out_sr=48000, out_peak=0.5, out_lufs=-23.0)
    with pytest.raises(ValueError):
        msgpu.render_batch([c2], results="stats", out_lufs=-23.0)
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([c2], devices=[0, 1], out_lufs=-23.0)
    args = (c2, [1000], [1.0], [1.0])
    with pytest.raises(ValueError):
        msgpu.render_variations(*args, export_sr=48000, export_peak="preset", export_lufs=-23.0)
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(*args, devices=[0, 1], export_lufs=-23.0)


# ---- life cycle ---------------------------------------------------------------------------
def test_destroy_releases_loudness_buffers():
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
    rec = e.loudness(x, [0], [x.shape[0]], 2, 48000)
    e.loudness_gain(x, [0], [x.shape[0]], 2, rec, -23.0, 0.9)
    torch.cuda.synchronize()
    assert live()[0] > base[0] and live()[1] > base[1]
    e.close()
    assert live() == base
