"""16/24-bit PCM with TPDF dither on the device: msg_quantize (csrc/kernels_pcm.h) against
msg_quantize_host for equal bytes and records on a ragged batch, batch independence, the
exports (render_variations(export_bits=), render_batch(out_bits=)) and the context's
life cycle.  Signals: tests/pcm_cases.py; every comparison is for equal bits."""
import gc
import os

import numpy as np
import pytest

import pcm_cases as PC
import msgpu
from msgpu.pcm import PCM_DTYPE, pack, quantize_host, read_wav_pcm, records, unpack

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


def device_quantize(eng, signals, channels, bits, mode, keys, fill=0xA5):
    """One msg_quantize call over the ragged batch into a byte tensor pre-filled with
    `fill`, 64 spare bytes behind: (host bytes, byte offsets, records)."""
    torch = eng.torch
    buf, offs, lens = layout(signals, channels)
    x = torch.from_numpy(buf).cuda()
    total = sum((len(s) * channels * (bits // 8) + 15) // 16 * 16 for s in signals) + 64
    out = torch.full((total,), fill, dtype=torch.uint8, device=x.device)
    got, byte_off, rec = eng.quantize(x, offs, lens, channels, bits, mode, PC.SEED, keys, out=out)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy(), byte_off, records(rec)


def check_against_host(host_bytes, byte_off, recs, signals, channels, bits, mode, keys, fill=0xA5):
    untouched = np.ones(host_bytes.size, dtype=bool)
    for i, (s, o, r) in enumerate(zip(signals, byte_off, recs)):
        key = i if keys is None else keys[i]
        q, hrec = quantize_host(s, bits, mode, PC.SEED, key)
        nb = s.size * (bits // 8)
        assert o % 16 == 0
        dev = host_bytes[o:o + nb]
        assert np.array_equal(dev, pack(q, bits)), f"signal {i}: W={s.size} ch={channels} {bits} bits {mode}"
        assert r.tobytes() == np.asarray(hrec, dtype=PCM_DTYPE).tobytes(), (i, s.size, r, hrec)
        assert r["nan"] == 0                                # no NaN of the gaps reached the record
        untouched[o:o + nb] = False
    assert np.all(host_bytes[untouched] == fill)            # not a byte outside the signals' ranges


# ---- device equals host to the bit --------------------------------------------------------
@pytest.mark.parametrize("mode", PC.DITHERS)
@pytest.mark.parametrize("bits", PC.BITS)
@pytest.mark.parametrize("channels", [1, 2])
def test_device_equals_host(eng, channels, bits, mode):
    tile = 4096 // channels                                 # frames of one tile; empty signals between, last too
    sig = PC.signals(channels) + [PC.signal(n * channels, channels, 0.3) for n in (0, 1, tile, 0, tile + 1, 0)]
    keys = [1000 + 7 * i for i in range(len(sig))]
    host_bytes, byte_off, recs = device_quantize(eng, sig, channels, bits, mode, keys)
    check_against_host(host_bytes, byte_off, recs, sig, channels, bits, mode, keys)
    assert sum(int(r["clipped"]) for r in recs) > 0         # the 1.2 signals clip on the device too


def test_default_keys_are_the_indices(eng):
    sig = PC.signals(2)[:6]
    host_bytes, byte_off, recs = device_quantize(eng, sig, 2, 16, "tpdf", None)
    check_against_host(host_bytes, byte_off, recs, sig, 2, 16, "tpdf", None)


@pytest.mark.parametrize("bits", PC.BITS)
@pytest.mark.parametrize("channels", [1, 2])
def test_batch_independence(eng, channels, bits):
    sig = PC.signals(channels)
    keys = list(range(50, 50 + len(sig)))
    together, byte_off, recs = device_quantize(eng, sig, channels, bits, "tpdf", keys)
    for i in (1, 5, len(sig) // 2, len(sig) - 3, len(sig) - 1):        # alone, with the same key
        alone, off1, rec1 = device_quantize(eng, [sig[i]], channels, bits, "tpdf", [keys[i]])
        nb = sig[i].size * (bits // 8)
        assert np.array_equal(alone[:nb], together[byte_off[i]:byte_off[i] + nb])
        assert rec1[0].tobytes() == recs[i].tobytes()


def test_nan_and_infinities_on_the_device(eng):
    x = np.array(PC.signal(4097, 1, 0.3))
    x[[0, 77, 4096]] = np.nan
    x[[5, 4095]] = [np.inf, -np.inf]
    for bits in PC.BITS:
        host_bytes, byte_off, recs = device_quantize(eng, [x], 1, bits, "tpdf", [9])
        q, hrec = quantize_host(x, bits, "tpdf", PC.SEED, 9)
        assert np.array_equal(host_bytes[:x.size * (bits // 8)], pack(q, bits))
        assert recs[0].tobytes() == np.asarray(hrec, dtype=PCM_DTYPE).tobytes()
        assert recs[0]["nan"] == 3 and recs[0]["clipped"] >= 2


def test_public_quantize(eng):
    torch = eng.torch
    for x, bits in ((PC.signal(8195, 1, 0.3), 16), (PC.signal(4096, 2, 1.2), 24)):
        q = msgpu.quantize(x, bits=bits, seed=5, key=11)
        want, _ = quantize_host(x, bits, "tpdf", 5, 11)
        assert q.dtype == want.dtype and q.shape == x.shape and np.array_equal(q, want)
        t = msgpu.quantize(torch.from_numpy(np.array(x)).cuda(), bits=bits, seed=5, key=11)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8
        assert np.array_equal(t.cpu().numpy(), pack(want, bits))
    assert np.array_equal(msgpu.quantize(PC.signal(17, 1, 0.3), dither="none"),
                          quantize_host(PC.signal(17, 1, 0.3), 16, "none")[0])


def test_argument_errors(eng):
    torch = eng.torch
    x = torch.zeros((64, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        eng.quantize(x, [0], [64], 2, 20)
    with pytest.raises(ValueError):
        eng.quantize(x, [0], [64], 2, 16, "shaped")
    with pytest.raises(ValueError):
        eng.quantize(x, [0], [64], 3, 16)
    with pytest.raises(ValueError):
        eng.quantize(x, [0], [65], 2, 16)                   # past the input tensor
    with pytest.raises(ValueError):
        eng.quantize(x, [0], [64], 2, 16, out=torch.zeros(100, dtype=torch.uint8, device="cuda"))   # too small
    with pytest.raises(ValueError):
        eng.quantize(x, [0, 32], [32, 32], 2, 16, keys=[1])
    # the C ABI's own checks: offsets off 16 bytes, overlapping ranges
    import ctypes as C
    from msgpu import _lib as L
    out = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    rec = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    off = (C.c_int64 * 2)(0, 32)
    cnt = (C.c_int64 * 2)(32, 32)
    stream = torch.cuda.current_stream()
    for byte_off in ((0, 136), (0, 64)):                    # 32 stereo frames at 16 bits are 128 bytes
        bo = (C.c_int64 * 2)(*byte_off)
        rc = L.lib().msg_quantize(eng._ctx, C.c_void_p(x.data_ptr()), 2, off, cnt, 2, 16, 1, 0, None,
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


@pytest.mark.parametrize("bits", PC.BITS)
def test_export_bits(c2, plain, tmp_path, monkeypatch, bits):
    from msgpu import batch
    args = (c2, SEEDS, [c2["time_unfold"]], [c2["partial_stretch"]])
    recs = []
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_bits=bits, export_dither_seed=21,
                                  export_records=recs, **R128)
    assert len(got) == len(plain) == len(recs) == 5
    for i, ((name, q, rate), (pname, p, _), r) in enumerate(zip(got, plain, recs)):
        want, hrec = quantize_host(p, bits, "tpdf", 21, i)  # the variant's index is the key
        assert name == pname and rate == 48000
        PC.same(q, r, want, hrec, bits, name)
        assert r["clipped"] == 0 and r["nan"] == 0          # -1 dBTP leaves headroom over one LSB of dither
        wav, wsr, wbits = read_wav_pcm(os.path.join(str(tmp_path), name))
        assert wsr == 48000 and wbits == bits and np.array_equal(wav, q)
    # the same bits however the batch is cut
    monkeypatch.setattr(batch, "MAX_BATCH_PRESETS", 2)
    cut = msgpu.render_variations(*args, export_bits=bits, export_dither_seed=21, **R128)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for (_, a, _), (_, b, _) in zip(got, cut))
    monkeypatch.undo()
    undithered = msgpu.render_variations(*args, export_bits=bits, export_dither="none", **R128)
    for (_, q, _), (_, p, _) in zip(undithered, plain):
        assert np.array_equal(q, quantize_host(p, bits, "none")[0])


def test_export_bits_none_is_the_float32_export(c2, plain):
    args = (c2, SEEDS, [c2["time_unfold"]], [c2["partial_stretch"]])
    same = msgpu.render_variations(*args, export_bits=None, **R128)
    assert all(a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
               for (_, a, _), (_, b, _) in zip(plain, same))


def test_render_batch_out_bits(c2, irs):
    torch = __import__("torch")
    ps = [c2, msgpu.config_params("C2", seed=1001, irs=irs, out_dur_s=0.25)]
    floats = msgpu.render_batch(ps)
    audio = msgpu.render_batch(ps, out_bits=16, out_dither_seed=4)
    dev = msgpu.render_batch(ps, results="device", out_bits=16, out_dither_seed=4)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 for t in dev)
    for i, (a, t, f) in enumerate(zip(audio, dev, floats)):
        want, _ = quantize_host(f, 16, "tpdf", 4, i)
        assert a.dtype == np.int16 and a.shape == f.shape and np.array_equal(a, want)
        assert np.array_equal(unpack(t.cpu().numpy(), 16, f.shape), want)
    f48 = msgpu.render_batch(ps, out_sr=48000, out_true_peak=-1.0)
    a48 = msgpu.render_batch(ps, out_sr=48000, out_true_peak=-1.0, out_bits=24, out_dither="none")
    for a, f in zip(a48, f48):
        assert a.dtype == np.int32 and np.array_equal(a, quantize_host(f, 24, "none")[0])
    same = msgpu.render_batch(ps, out_bits=None)
    assert all(np.array_equal(a, b) for a, b in zip(floats, same))


def test_export_argument_errors(c2):
    with pytest.raises(ValueError):
        msgpu.render_batch([c2], results="stats", out_bits=16)
    with pytest.raises(ValueError):
        msgpu.render_batch([c2], out_bits=20)
    with pytest.raises(ValueError):
        msgpu.render_batch([c2], out_bits=16, out_dither="shaped")
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([c2], devices=[0, 1], out_bits=16)
    args = (c2, [1000], [1.0], [1.0])
    with pytest.raises(ValueError):
        msgpu.render_variations(*args, export_bits=8)
    with pytest.raises(ValueError):
        msgpu.render_variations(*args, export_bits=16, export_dither="shaped")
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(*args, devices=[0, 1], export_bits=24)


# ---- life cycle ---------------------------------------------------------------------------------
def test_destroy_releases_quantiser_buffers():
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
    x = torch.from_numpy(np.array(PC.signal(20011 - 1, 2, 0.3))).cuda()
    e.quantize(x, [0, 4000], [4000, 6005], 2, 24)
    torch.cuda.synchronize()
    assert live()[0] > base[0] and live()[1] > base[1]
    e.close()
    assert live() == base
