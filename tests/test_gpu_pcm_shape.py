"""Noise-shaped dither on the device: msg_quantize_shaped (csrc/kernels_pcm_shape.h) against
msg_quantize_shaped_host for equal bytes and records on ragged batches whose lanes end at
different steps, batch independence, the exports (render_variations(export_shape=),
render_batch(out_shape=)) and the context's life cycle.  Signals: tests/pcm_shape_cases.py;
every comparison is for equal bits."""
import gc
import os

import numpy as np
import pytest

import pcm_shape_cases as SC
import msgpu
from msgpu.pcm import (PCM_DTYPE, pack, quantize_host, quantize_shaped_host, read_wav_pcm, records, unpack)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def layout(signals, channels, gap=3):
    """The signals in one buffer with `gap` frames of NaN in front of and between them (an
    odd gap: mono signals start at odd floats) and none behind: the last signal ends at
    the buffer's last float.  (buffer, offsets, lens)."""
    offs, lens, parts = [], [], []
    at = 0
    nan = lambda k: np.full((k, 2) if channels == 2 else k, np.nan, dtype=np.float32)
    for s in signals:
        parts += [nan(gap), np.asarray(s, dtype=np.float32)]
        at += gap
        offs.append(at)
        lens.append(len(s))
        at += len(s)
    return np.concatenate(parts), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)


def device_quantize(eng, signals, channels, bits, mode, shape, keys, fill=0xA5):
    """One msg_quantize_shaped call over the ragged batch into a byte tensor pre-filled with
    `fill`, 64 spare bytes behind: (host bytes, byte offsets, records)."""
    torch = eng.torch
    buf, offs, lens = layout(signals, channels)
    x = torch.from_numpy(buf).cuda()
    total = sum((len(s) * channels * (bits // 8) + 15) // 16 * 16 for s in signals) + 64
    out = torch.full((total,), fill, dtype=torch.uint8, device=x.device)
    got, byte_off, rec = eng.quantize(x, offs, lens, channels, bits, mode, SC.SEED, keys, out=out, shape=shape)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy(), byte_off, records(rec)


@pytest.fixture(scope="module")
def host():
    """msg_quantize_shaped_host of a signal of tests/pcm_shape_cases.py, computed once per
    (signal, bits, mode, shape, key) and shared: do not write to it."""
    memo = {}

    def get(s, bits, mode, shape, key):
        k = (id(s), bits, mode, shape, key)
        if k not in memo:
            memo[k] = (s, *quantize_shaped_host(s, bits, mode, shape, SC.SEED, key))
        return memo[k][1:]
    return get


def check_against_host(host, host_bytes, byte_off, recs, signals, channels, bits, mode, shape, keys, fill=0xA5):
    untouched = np.ones(host_bytes.size, dtype=bool)
    for i, (s, o, r) in enumerate(zip(signals, byte_off, recs)):
        key = i if keys is None else keys[i]
        q, hrec = host(s, bits, mode, shape, key)
        nb = s.size * (bits // 8)
        assert o % 16 == 0
        dev = host_bytes[o:o + nb]
        assert np.array_equal(dev, pack(q, bits)), f"signal {i}: W={s.size} ch={channels} {bits} bits {mode} {shape}"
        assert r.tobytes() == np.asarray(hrec, dtype=PCM_DTYPE).tobytes(), (i, s.size, r, hrec)
        assert r["nan"] == 0                                # no NaN of the gaps reached the record
        untouched[o:o + nb] = False
    assert np.all(host_bytes[untouched] == fill)            # not a byte outside the signals' ranges


def ragged(channels, count):
    """`count` signals of mixed lengths: the lanes of a wave end at different steps, a long
    signal now and then, empty ones between."""
    pool = SC.runs(channels)
    order = np.random.default_rng(count + channels).permutation(len(pool))
    return [pool[order[i % len(pool)]] for i in range(count)]


# ---- device equals host to the bit --------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_ragged_batch_equals_host(eng, host, channels):
    sig = ragged(channels, 130)
    assert len({s.size for s in sig}) >= 10 and max(s.size for s in sig) > 20000 and sig[-1].size > 0
    keys = [1000 + 7 * (i % 29) for i in range(len(sig))]
    host_bytes, byte_off, recs = device_quantize(eng, sig, channels, 16, "tpdf", "f9", keys)
    check_against_host(host, host_bytes, byte_off, recs, sig, channels, 16, "tpdf", "f9", keys)
    assert sum(int(r["clipped"]) for r in recs) > 0         # the 1.2 signals clip on the device too


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_signal_counts(eng, host, count):
    sig = ragged(2, 130)[-count:]
    keys = [1000 + 7 * (i % 29) for i in range(130)][-count:]
    host_bytes, byte_off, recs = device_quantize(eng, sig, 2, 16, "tpdf", "f9", keys)
    check_against_host(host, host_bytes, byte_off, recs, sig, 2, 16, "tpdf", "f9", keys)


@pytest.mark.parametrize("shape", SC.NAMES)
@pytest.mark.parametrize("mode", SC.DITHERS)
@pytest.mark.parametrize("bits", SC.BITS)
@pytest.mark.parametrize("channels", [1, 2])
def test_every_variant_on_the_short_lengths(eng, host, channels, bits, mode, shape):
    sig = SC.runs(channels, SC.SHORT)
    keys = [50 + i for i in range(len(sig))]
    host_bytes, byte_off, recs = device_quantize(eng, sig, channels, bits, mode, shape, keys)
    check_against_host(host, host_bytes, byte_off, recs, sig, channels, bits, mode, shape, keys)


@pytest.mark.parametrize("shape", ["f9", "e3"])
@pytest.mark.parametrize("bits", SC.BITS)
@pytest.mark.parametrize("channels", [1, 2])
def test_long_signals(eng, host, channels, bits, shape):
    sig = SC.runs(channels, SC.LONG + (2 * SC.CHUNK + 3, 12)) + [SC.signal(20010, channels, 1.2)]
    host_bytes, byte_off, recs = device_quantize(eng, sig, channels, bits, "tpdf", shape, None)
    check_against_host(host, host_bytes, byte_off, recs, sig, channels, bits, "tpdf", shape, None)


@pytest.mark.parametrize("channels", [1, 2])
def test_batch_independence(eng, channels):
    sig = ragged(channels, 70)
    keys = list(range(50, 50 + len(sig)))
    together, byte_off, recs = device_quantize(eng, sig, channels, 24, "tpdf", "lipshitz5", keys)
    big = max(range(len(sig)), key=lambda i: sig[i].size)
    for i in (1, 5, big, 64, len(sig) - 1):                 # alone, with the same key
        alone, off1, rec1 = device_quantize(eng, [sig[i]], channels, 24, "tpdf", "lipshitz5", [keys[i]])
        nb = sig[i].size * 3
        assert np.array_equal(alone[:nb], together[byte_off[i]:byte_off[i] + nb])
        assert rec1[0].tobytes() == recs[i].tobytes()


def test_nan_and_infinities_on_the_device(eng):
    for channels in (1, 2):
        x = np.array(SC.signal(4098, channels, 0.3))
        flat = x.reshape(-1)
        flat[[0, 77, 4097]] = np.nan
        flat[[5, 4095]] = [np.inf, -np.inf]
        for bits in SC.BITS:
            host_bytes, byte_off, recs = device_quantize(eng, [x], channels, bits, "tpdf", "f9", [9])
            q, hrec = quantize_shaped_host(x, bits, "tpdf", "f9", SC.SEED, 9)
            assert np.array_equal(host_bytes[:x.size * (bits // 8)], pack(q, bits))
            assert recs[0].tobytes() == np.asarray(hrec, dtype=PCM_DTYPE).tobytes()
            assert recs[0]["nan"] == 3 and recs[0]["clipped"] >= 2


def test_public_quantize(eng):
    torch = eng.torch
    for x, bits, shape in ((SC.signal(2 * SC.CHUNK + 3, 1, 0.3), 16, "f9"), (SC.signal(20010, 2, 1.2), 24, "e3")):
        q = msgpu.quantize(x, bits=bits, seed=5, key=11, shape=shape)
        want, _ = quantize_shaped_host(x, bits, "tpdf", shape, 5, 11)
        assert q.dtype == want.dtype and q.shape == x.shape and np.array_equal(q, want)
        t = msgpu.quantize(torch.from_numpy(np.array(x)).cuda(), bits=bits, seed=5, key=11, shape=shape)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8
        assert np.array_equal(t.cpu().numpy(), pack(want, bits))
        # shape=None runs what it ran before: msg_quantize's bytes
        assert np.array_equal(msgpu.quantize(x, bits=bits, seed=5, key=11, shape=None),
                              quantize_host(x, bits, "tpdf", 5, 11)[0])
    x = SC.signal(SC.CHUNK + 1, 1, 0.3)
    assert np.array_equal(msgpu.quantize(x, dither="none", shape="lipshitz5"),
                          quantize_shaped_host(x, 16, "none", "lipshitz5")[0])


def test_argument_errors(eng):
    torch = eng.torch
    x = torch.zeros((64, 2), dtype=torch.float32, device="cuda")
    for bad in ("shaped", 0, 4, True):
        with pytest.raises(ValueError):
            eng.quantize(x, [0], [64], 2, 16, shape=bad)
    with pytest.raises(ValueError):
        eng.quantize(x, [0], [64], 2, 20, shape="f9")
    with pytest.raises(ValueError):
        eng.quantize(x, [0], [65], 2, 16, shape="f9")       # past the input tensor
    with pytest.raises(ValueError):
        msgpu.quantize(np.zeros(8, dtype=np.float32), shape="shaped")
    # the C ABI's own checks: the shape code, offsets off 16 bytes, overlapping ranges
    import ctypes as C
    from msgpu import _lib as L
    out = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    rec = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    off = (C.c_int64 * 2)(0, 32)
    cnt = (C.c_int64 * 2)(32, 32)
    stream = torch.cuda.current_stream()
    for shape, byte_off in ((0, (0, 128)), (4, (0, 128)), (3, (0, 136)), (3, (0, 64))):   # 32 stereo frames: 128 bytes
        bo = (C.c_int64 * 2)(*byte_off)
        rc = L.lib().msg_quantize_shaped(eng._ctx, C.c_void_p(x.data_ptr()), 2, off, cnt, 2, 16, 1, shape, 0, None,
                                         C.c_void_p(out.data_ptr()), bo, C.c_void_p(rec.data_ptr()),
                                         C.c_void_p(stream.cuda_stream))
        assert rc == L.MSG_E_VALUE
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                      # a refused call writes nothing


# ---- exports ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(irs):
    return msgpu.config_params("C2", irs=irs, out_dur_s=0.25)


SEEDS = [1000, 1001, 1002, 1003, 1004]
R128 = {"export_sr": 48000, "export_lufs": -23.0, "export_true_peak": -1.0}


@pytest.fixture(scope="module")
def plain(c2):
    """The float32 R 128 export of five variants, shared by the export tests: do not write to it."""
    return msgpu.render_variations(c2, SEEDS, [c2["time_unfold"]], [c2["partial_stretch"]], **R128)


def test_export_shape(c2, plain, tmp_path, monkeypatch):
    from msgpu import batch
    args = (c2, SEEDS, [c2["time_unfold"]], [c2["partial_stretch"]])
    recs = []
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_bits=16, export_shape="f9", export_dither_seed=21,
                                  export_records=recs, **R128)
    assert len(got) == len(plain) == len(recs) == 5
    for i, ((name, q, rate), (pname, p, _), r) in enumerate(zip(got, plain, recs)):
        want, hrec = quantize_shaped_host(p, 16, "tpdf", "f9", 21, i)   # the variant's index is the key
        assert name == pname and rate == 48000
        SC.same(q, r, want, hrec, 16, name)
        assert r["clipped"] == 0 and r["nan"] == 0          # -1 dBTP leaves headroom over f9's 33.6 LSB
        wav, wsr, wbits = read_wav_pcm(os.path.join(str(tmp_path), name))
        assert wsr == 48000 and wbits == 16 and np.array_equal(wav, q)
    # the same bits however the batch is cut
    monkeypatch.setattr(batch, "MAX_BATCH_PRESETS", 2)
    cut = msgpu.render_variations(*args, export_bits=16, export_shape="f9", export_dither_seed=21, **R128)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for (_, a, _), (_, b, _) in zip(got, cut))
    monkeypatch.undo()
    # export_shape=None is the TPDF export
    unshaped = msgpu.render_variations(*args, export_bits=16, export_shape=None, export_dither_seed=21, **R128)
    for i, ((_, q, _), (_, p, _)) in enumerate(zip(unshaped, plain)):
        assert np.array_equal(q, quantize_host(p, 16, "tpdf", 21, i)[0])


def test_render_batch_out_shape(c2, irs):
    torch = __import__("torch")
    ps = [c2, msgpu.config_params("C2", seed=1001, irs=irs, out_dur_s=0.25)]
    floats = msgpu.render_batch(ps)
    audio = msgpu.render_batch(ps, out_bits=16, out_dither_seed=4, out_shape="f9")
    dev = msgpu.render_batch(ps, results="device", out_bits=16, out_dither_seed=4, out_shape="f9")
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 for t in dev)
    for i, (a, t, f) in enumerate(zip(audio, dev, floats)):
        want, _ = quantize_shaped_host(f, 16, "tpdf", "f9", 4, i)
        assert a.dtype == np.int16 and a.shape == f.shape and np.array_equal(a, want)
        assert np.array_equal(unpack(t.cpu().numpy(), 16, f.shape), want)
    a24 = msgpu.render_batch(ps, out_bits=24, out_dither="none", out_shape="e3")
    for a, f in zip(a24, floats):
        assert a.dtype == np.int32 and np.array_equal(a, quantize_shaped_host(f, 24, "none", "e3")[0])
    same = msgpu.render_batch(ps, out_bits=16, out_dither_seed=4, out_shape=None)
    for i, (a, f) in enumerate(zip(same, floats)):
        assert np.array_equal(a, quantize_host(f, 16, "tpdf", 4, i)[0])


# ---- life cycle ---------------------------------------------------------------------------------
def test_destroy_releases_shaper_buffers():
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
    x = torch.from_numpy(np.array(SC.signal(20010, 2, 0.3))).cuda()
    e.quantize(x, [0, 4000], [4000, 6005], 2, 24, shape="f9")
    torch.cuda.synchronize()
    assert live()[0] > base[0] and live()[1] > base[1]
    e.close()
    assert live() == base
