"""FLAC delivery on the device (msg_flac; csrc/kernels_flac.h): frames and records equal to the
library's host loop (msg_flac_host) to the byte, read back by the independent reader, at every
block form, frame-number width, content, rate and in ragged batches, and through the delivery chain."""
import hashlib
import os

import numpy as np
import pytest

import msgpu
import flac_cases as FC
from msgpu import pcm
from msgpu.flac import FLAC_DTYPE, Flac, bound, frames_host, read_flac, read_frame, records, stream_header

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def pack_batch(signals, bits):
    """The signals' packed PCM at 16-byte-rounded offsets, as Engine.quantize lays them: (bytes, offsets, lens)."""
    parts, offs, at = [], [], 0
    for q in signals:
        b = pcm.pack(q, bits)
        offs.append(at)
        pad = -len(b) % 16
        parts += [b, np.full(pad, 0xA5, dtype=np.uint8)]
        at += len(b) + pad
    buf = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return buf, np.array(offs, dtype=np.int64), np.array([len(q) for q in signals], dtype=np.int64)


def encode(eng, signals, channels, bits, sr, flac):
    buf, offs, lens = pack_batch(signals, bits)
    t = eng.torch.from_numpy(buf.copy()).cuda()
    out, rec = eng.flac(t, offs, lens, channels, bits, sr, flac.block, flac.md5)
    assert tuple(rec.shape) == (len(signals), 11)
    assert out.numel() == sum((bound(len(q), channels, bits, flac.block) + 15) // 16 * 16 for q in signals)
    return out.cpu().numpy(), records(rec)


def check(eng, signals, channels, bits, sr=FC.SR, flac=None, decode=True, what=""):
    """Device bytes and records equal msg_flac_host's; the output is compact; the reader gives the input back."""
    flac = flac or Flac()
    out, rec = encode(eng, signals, channels, bits, sr, flac)
    at = 0
    for i, q in enumerate(signals):
        body, want = frames_host(q, sr, bits, flac)
        want = want.copy()
        want["byte_off"] = at
        got = out[at:at + len(body)]
        assert rec[i].tobytes() == want.tobytes(), (what, i, len(q), rec[i], want)
        assert np.array_equal(got, body), (what, i, len(q), int(np.flatnonzero(got != body)[0]))
        assert bytes(rec[i]["md5"]) == (hashlib.md5(pcm.pack(q, bits).tobytes()).digest() if flac.md5 else bytes(16))
        if decode:
            y = read_flac(np.concatenate([stream_header(rec[i], sr, channels, bits, flac.block), got]))[0]
            assert np.array_equal(y, q.reshape(y.shape)), (what, i)
        at += (len(body) + 15) // 16 * 16
    return out, rec


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("channels", [1, 2])
def test_lengths(eng, channels, bits):
    """0, 1, 4, 5 (constant or verbatim only), 255, 256, 257 (the 8- and 16-bit last-block forms), 4095, 4096 (a full
    last block), 4097 and 8192 + 17 frames at block 4096, in one ragged batch and with md5 off."""
    sig = [FC.signal("sine", n, channels, bits) for n in FC.LENGTHS]
    out, rec = check(eng, sig, channels, bits)
    out2, rec2 = check(eng, sig, channels, bits, flac=Flac(md5=False), decode=False)
    total = int(rec[-1]["byte_off"] + rec[-1]["bytes"])
    assert np.array_equal(out[:total], out2[:total]) and not rec2["md5"].any() and not rec2["flags"].any()


def test_frame_numbers(eng):
    """129 and 2049 blocks of 256: two- and three-byte frame numbers; the reader on the first and last three frames."""
    f = Flac(block=256)
    for blocks, channels, bits in ((129, 2, 16), (2049, 1, 24)):
        q = FC.signal("sine", blocks * 256 - 100, channels, bits)
        out, rec = check(eng, [q], channels, bits, flac=f, decode=blocks < 1000, what=f"{blocks} blocks")
        assert int(rec[0]["frames"]) == blocks
    data = bytes(out[:int(rec[0]["bytes"])])
    pos = 0
    for j in range(3):
        x, pos, info = read_frame(data, pos, channels, bits)
        assert info["number"] == j and np.array_equal(x, q[j * 256:(j + 1) * 256].reshape(x.shape))
    # the last frames: walk to the end from each sync pattern near it; a false sync fails a CRC
    tail = []
    for s in (i for i in range(len(data) - 4000, len(data) - 1) if data[i] == 0xFF and data[i + 1] == 0xF8):
        try:
            at, tail = s, []
            while at < len(data):
                x, at, info = read_frame(data, at, channels, bits)
                tail.append((info["number"], x))
        except ValueError:
            continue
        if len(tail) >= 3:
            break
    assert len(tail) >= 3 and tail[-1][0] == blocks - 1 and len(tail[-1][1]) == 256 - 100
    for number, x in tail[-3:]:
        assert np.array_equal(x, q[number * 256:number * 256 + len(x)].reshape(x.shape))


@pytest.mark.parametrize("bits", [16, 24])
def test_content(eng, bits):
    """Every content case, mono and stereo, 4096 + 300 frames: all subframe kinds, both Rice methods, the four
    assignments; at 24 bits the +- full-scale alternation with L = -R gives the largest residuals."""
    seen = np.zeros(4, dtype=np.int64)
    kinds = np.zeros(3, dtype=np.int64)
    for channels in (1, 2):
        sig = [FC.signal(name, 4096 + 300, channels, bits) for name in FC.CONTENT]
        _, rec = check(eng, sig, channels, bits, what=f"content {channels}")
        seen += rec["assign"].sum(axis=0)
        kinds += [rec["constant"].sum(), rec["verbatim"].sum(), rec["fixed"].sum()]
    assert kinds.all() and seen[0] and seen[3] and (seen[1] or seen[2])


def test_quantised_render(eng):
    """A real render quantised by msg_quantize_shaped: the encoder reads the device bytes where the quantiser left them."""
    rng = np.random.default_rng(3)
    n = 3 * 4096 + 501
    t = np.arange(n) / FC.SR
    x = (0.3 * np.sin(2 * np.pi * 220 * t) * np.exp(-3 * t))[:, None] * np.array([1.0, 0.6]) + 1e-3 * rng.standard_normal((n, 2))
    xt = eng.torch.from_numpy(x.astype(np.float32)).cuda()
    for bits in (16, 24):
        q, byte_off, _ = eng.quantize(xt, [0, 4096], [n, n - 4096], 2, bits, "tpdf", 5, [0, 1], shape="f9")
        out, rec = eng.flac(q, byte_off, [n, n - 4096], 2, bits, FC.SR)
        host = q.cpu().numpy()
        rec, out = records(rec), out.cpu().numpy()
        for i, m in enumerate((n, n - 4096)):
            ints = pcm.unpack(host[int(byte_off[i]):int(byte_off[i]) + m * 2 * (bits // 8)], bits, (m, 2))
            body, want = frames_host(ints, FC.SR, bits)
            o = int(rec[i]["byte_off"])
            assert np.array_equal(out[o:o + len(body)], body) and int(rec[i]["bytes"]) == len(body)
            assert bytes(rec[i]["md5"]) == bytes(want["md5"])
            assert int(rec[i]["bytes"]) < 0.8 * m * 2 * (bits // 8)


@pytest.mark.parametrize("sr", [44100, 48000, 96000, 384000, 44101])
def test_rates(eng, sr):
    check(eng, [FC.signal("sine", 700, 2, 16), FC.signal("gauss", 300, 2, 16)], 2, 16, sr=sr, flac=Flac(block=256))


def test_batch_equals_alone(eng):
    """A dozen signals of mixed lengths and contents in one call: each signal's bytes and record are those of the
    signal encoded alone, and the output is compact (check: offsets are the 16-byte-rounded prefix of the lengths)."""
    lens = (5000, 0, 1, 4096, 777, 8192 + 17, 256, 4097, 3, 12000, 255, 2048)
    for channels, bits, block in ((2, 16, 4096), (1, 24, 1024)):
        f = Flac(block=block)
        sig = [FC.signal(FC.CONTENT[i % len(FC.CONTENT)], n, channels, bits) for i, n in enumerate(lens)]
        out, rec = check(eng, sig, channels, bits, flac=f, decode=False, what="batch")
        for i in (0, 5, 9, 11):
            o1, r1 = encode(eng, [sig[i]], channels, bits, FC.SR, f)
            a, b = int(rec[i]["byte_off"]), int(rec[i]["bytes"])
            assert np.array_equal(o1[:b], out[a:a + b]) and int(r1[0]["byte_off"]) == 0
            r = rec[i].copy()
            r["byte_off"] = 0
            assert r.tobytes() == r1[0].tobytes()


def test_public_function_and_refusals(eng):
    q = FC.signal("sine", 5000, 2, 16)
    data = msgpu.flac(q, 48000, 16)
    assert data.dtype == np.uint8 and np.array_equal(read_flac(data)[0], q)
    t = eng.torch.from_numpy(pcm.pack(q, 16).copy()).cuda()
    assert np.array_equal(msgpu.flac(t, 48000, 16, Flac(block=512), channels=2), msgpu.flac(q, 48000, 16, Flac(block=512)))
    assert len(msgpu.flac(q[:0], 48000, 16)) == 42
    with pytest.raises(ValueError):
        eng.flac(t, [0], [5000], 2, 16, 655351)
    with pytest.raises(ValueError):
        eng.flac(t, [8], [100], 2, 16, 48000)
    with pytest.raises(ValueError):
        eng.flac(t, [0], [5001], 2, 16, 48000)
    with pytest.raises(ValueError):
        eng.flac(t, [0], [5000], 2, 16, 48000, block=300)


@pytest.fixture(scope="module")
def c2(irs):
    return msgpu.config_params("C2", irs=irs, out_dur_s=0.75)


def test_chain_returns_files(eng, c2):
    from msgpu.stereo import Stereo
    presets = [c2, msgpu.merged(c2, seed=77)]
    kw = dict(out_sr=48000, out_lufs=-23, out_true_peak=-1, out_bits=16)
    files = msgpu.render_batch(presets, out_flac=Flac(), **kw)
    ints = msgpu.render_batch(presets, **kw)
    for f, q in zip(files, ints):
        y, sr, bits, info = read_flac(f)
        assert f.dtype == np.uint8 and sr == 48000 and bits == 16 and info["channels"] == 2 and np.array_equal(y, q)
        assert info["md5"] == hashlib.md5(pcm.pack(q, 16).tobytes()).digest()
        assert len(f) < q.size * 2
    mono = msgpu.render_batch(presets, out_flac=Flac(), out_stereo=Stereo(channels=1), **kw)
    want = msgpu.render_batch(presets, out_stereo=Stereo(channels=1), **kw)
    for f, q in zip(mono, want):
        y, _, _, info = read_flac(f)
        assert info["channels"] == 1 and np.array_equal(y, q)


def test_render_variations_writes_flac_files(c2, tmp_path):
    args = (c2, [1000, 1001], [c2["time_unfold"]], [c2["partial_stretch"]])
    pcm_rec, flac_rec, pcm_rec2 = [], [], []
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_bits=24, export_flac=Flac(), export_records=pcm_rec,
                                  export_flac_records=flac_rec)
    want = msgpu.render_variations(*args, export_bits=24, export_records=pcm_rec2)
    assert len(got) == 2 and len(flac_rec) == 2 and [r.tobytes() for r in pcm_rec] == [r.tobytes() for r in pcm_rec2]
    for (name, data, rate), (_, q, _), r in zip(got, want, flac_rec):
        assert name.endswith(".flac") and sorted(os.listdir(str(tmp_path))) == sorted(n for n, _, _ in got)
        y, sr, bits, info = read_flac(os.path.join(str(tmp_path), name))
        assert sr == rate and bits == 24 and np.array_equal(y, q) and np.array_equal(read_flac(data)[0], q)
        assert r.dtype == FLAC_DTYPE and int(r["bytes"]) == len(data) - 42 and int(r["frames"]) == info["frames"]
