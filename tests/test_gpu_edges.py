"""The edges pass on the device (msg_edges, csrc/kernels_edges.h) against the library's host loop
(msg_edges_host), records and samples to the bit, over ragged batches of the signals and options
of tests/edges_cases.py; then the delivery chain with the new rule."""
import os

import numpy as np
import pytest

import edges_cases as EC
import truepeak_cases as TC
import msgpu
from msgpu.edges import EDGES_DTYPE, Edges, edges_host, edges_reference, records

pytestmark = pytest.mark.gpu

GUARD = 0.75          # between the signals: sound at every threshold, so a frame read past an end shows in the record


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def pack(signals, channels, gap=3):
    """The signals back to back with `gap` guard frames around and between them (an odd gap: mono
    signals start at odd floats): (buffer, offsets, lens)."""
    guard = np.full((gap, 2) if channels == 2 else gap, GUARD, dtype=np.float32)
    offs, lens, parts, at = [], [], [guard], gap
    for s in signals:
        offs.append(at)
        lens.append(len(s))
        parts += [np.asarray(s, dtype=np.float32), guard]
        at += len(s) + gap
    return np.concatenate(parts), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)


def run_and_compare(eng, named, channels, config, gap=3):
    """One msg_edges call over the signals between guards; every record and every word against
    msg_edges_host, the guards against what they were.  Returns the device records."""
    e = EC.CONFIGS[config] if isinstance(config, str) else config
    buf, offs, lens = pack([x for _, x in named], channels, gap)
    x = eng.torch.from_numpy(buf).cuda()
    rec = records(eng.edges(x, offs, lens, channels, EC.SR, e))
    got = x.cpu().numpy()
    assert rec.dtype == EDGES_DTYPE and len(rec) == len(named)
    want = buf.copy()
    for i, (name, s) in enumerate(named):
        y, r = edges_host(s, EC.SR, e)
        o = int(offs[i])
        want[o:o + len(s)] = y
        EC.assert_same(f"{config} / #{i} {name} ch={channels}", got[o:o + len(s)], rec[i], y, r)
    assert np.array_equal(EC.bits(got), EC.bits(want))              # the guard frames too
    return rec


@pytest.mark.parametrize("config", list(EC.CONFIGS))
@pytest.mark.parametrize("channels", [1, 2])
def test_ragged_batch_equals_the_host(eng, channels, config):
    run_and_compare(eng, EC.signals(channels), channels, config)


def test_seventy_signals(eng):
    """More signals than one step of the tile lookup's bisection resolves, empty ones among them."""
    sig = EC.signals(1)
    named = [sig[(7 * i) % len(sig)] for i in range(70)]
    for config in ("both", "loop", "fades longer than the signal"):
        run_and_compare(eng, named, 1, config)


@pytest.mark.parametrize("channels", [1, 2])
def test_wave_boundary(eng, channels):
    """A frame at the threshold in the last lane of a wave, one in the first lane of the next, and
    both: with the tile's first float 16-byte aligned (a gap of four frames) and at odd offsets."""
    sig = dict(EC.signals(channels))
    a, b = EC.wave_edge(channels)
    names = ("last lane of a wave", "first lane of the next wave", "both sides of a wave")
    for gap in (4, 3):
        rec = run_and_compare(eng, [(n, sig[n]) for n in names], channels, Edges(trim_db=EC.TRIM_DB), gap)
        assert [(int(r["first"]), int(r["last"])) for r in rec] == [(a, a), (b, b), (a, b)]
        assert [(int(r["start"]), int(r["end"])) for r in rec] == [(a, a + 1), (b, b + 1), (a, b + 1)]


@pytest.mark.parametrize("channels", [1, 2])
def test_loop(eng, channels):
    sig = dict(EC.signals(channels))
    x = sig["odd span"]
    for config in ("loop", "loop longer than half", "loop only"):
        e = EC.CONFIGS[config]
        rec = run_and_compare(eng, [("odd span", x)], channels, config)[0]
        y, r = msgpu.edges(x, EC.SR, e)                                   # the public function: the span, copied out
        y_def, r_def = edges_reference(x, EC.SR, e)
        assert r.tobytes() == rec.tobytes() == r_def.tobytes()
        s, end = int(r["start"]), int(r["end"])
        assert y.shape[0] == end - s and r["loop"] > 0
        # within the crossfade's own arithmetic of the float64 definition: two gains, each within 2^-24, |x| <= 1
        assert np.abs(y.astype(np.float64) - y_def[s:end].astype(np.float64)).max() <= 2.0 ** -23
        # the seam: the span's first frame is the frame that followed its last one, to within the first gains
        t0 = 1.0 / (2.0 * int(r["loop"]))
        assert np.abs(y[0].astype(np.float64) - x[end].astype(np.float64)).max() <= 2.0 * t0 + 2.0 ** -23


def test_public_function_on_a_device_tensor(eng):
    x = dict(EC.signals(2))[f"burst n={EC.N}"]
    e = EC.CONFIGS["both"]
    y_host, r_host = edges_host(x, EC.SR, e)
    t = eng.torch.from_numpy(x).cuda()
    rec = msgpu.edges(t, EC.SR, e)                                        # in place, the device records back
    assert rec.is_cuda and tuple(rec.shape) == (1, 8)
    assert records(rec)[0].tobytes() == r_host.tobytes()
    assert np.array_equal(EC.bits(t.cpu().numpy()), EC.bits(y_host))
    y, r = msgpu.edges(x, EC.SR, e)
    assert np.array_equal(EC.bits(y), EC.bits(y_host[int(r["start"]):int(r["end"])]))
    with pytest.raises(ValueError):
        eng.edges(t, [0], [EC.N + 1], 2, EC.SR, e)


# ---- the delivery chain -------------------------------------------------------------------------
CHAIN = Edges(trim_db=-60, pad_ms=5, fade_ms=(2, 20))


@pytest.fixture(scope="module")
def sparse():
    """Two short sparse presets: one event in half a second at 44.1 kHz, three Hawkes events in
    0.75 s at 48 kHz whose first comes after a quarter of a second (seed 1000: five events from 52 ms).
    Mono-compatible stereo: the spectral diffusion of stereo_on spreads every event over the whole render."""
    return [msgpu.config_params("C1", base_sr=44100, out_dur_s=0.5, stereo_on=False),
            msgpu.config_params("C1", seed=1001, out_dur_s=0.75, event_process="Hawkes", grains_per_sec=4.0,
                                bp_density="", stereo_on=False)]


def host_spans(renders, sr=48000):
    recs = [edges_host(y, sr, CHAIN)[1] for y in renders]
    return [int(r["end"] - r["start"]) for r in recs], recs


def test_render_batch_with_edges(eng, sparse):
    from msgpu.export import Delivery, deliver, unpack_all
    from msgpu.pack import PackedBatch
    from msgpu.params import merged
    rep = []
    out = msgpu.render_batch(sparse, out_sr=48000, out_lufs=-23, out_true_peak=-1, out_bits=16, out_edges=CHAIN,
                             out_report=rep)
    plain = msgpu.render_batch(sparse, out_sr=48000)                   # the undelivered renders, resampled alone
    lens, recs = host_spans(plain)
    print("edges chain: full", [len(y) for y in plain], "delivered", lens, [tuple(r) for r in recs])
    assert [a.shape for a in out] == [(n, 2) for n in lens] and all(a.dtype == np.int16 for a in out)
    assert all(0 < n < len(y) for n, y in zip(lens, plain))           # sparse renders: each is trimmed
    assert [int(r["frames"]) for r in rep] == lens
    # the ceiling holds on what is delivered, faded ends included: a render too short for a loudness block
    # (the first, 51 ms) is scaled to the ceiling itself, and lies there within the bound of a gain's roundings
    for r in rep:
        print(f"edges chain report: {float(r['lufs']):.6f} LUFS, true peak {float(r['true_peak']):.9f}, "
              f"{float(r['dbtp']):+.7f} dBTP, {int(r['frames'])} frames")
        assert float(r["true_peak"]) <= 10.0 ** (-1.0 / 20.0) * (1.0 + TC.E_GAIN)
    # float32 delivery with the edges alone: the host function's samples
    shaped = msgpu.render_batch(sparse, out_sr=48000, out_edges=CHAIN)
    for y, x, r in zip(shaped, plain, recs):
        want = edges_host(x, 48000, CHAIN)[0][int(r["start"]):int(r["end"])]
        assert np.array_equal(EC.bits(y), EC.bits(want))
    # batch independence: each render delivered alone, with its dither key, gives the same words
    for i, p in enumerate(sparse):
        d = Delivery(48000, None, -23, None, -1, 16, edges=CHAIN)
        packed = PackedBatch([p])
        y, off, nbytes, _ = deliver(eng, eng.render_packed(packed), packed.offsets, packed.out_n, [merged(p)["base_sr"]], d,
                                    None, [i])
        eng.torch.cuda.synchronize(eng.device)
        alone = unpack_all(y.cpu().numpy(), off, nbytes, 16)[0]
        assert np.array_equal(alone, out[i]), i
    dev = msgpu.render_batch(sparse, results="device", out_sr=48000, out_edges=CHAIN)
    assert [int(t.shape[0]) for t in dev] == lens
    with pytest.raises(NotImplementedError):
        msgpu.render_batch(sparse, devices=[0, 1], out_edges=CHAIN)


def test_render_variations_with_edges(sparse, tmp_path):
    from msgpu.pcm import read_wav_pcm
    base = sparse[1]
    args = (base, [1000, 1001], [base["time_unfold"]], [base["partial_stretch"]])
    plain = msgpu.render_variations(*args, export_sr=48000)
    lens, _ = host_spans([y for _, y, _ in plain])
    rep = []
    got = msgpu.render_variations(*args, folder=str(tmp_path), export_sr=48000, export_lufs=-23, export_true_peak=-1,
                                  export_bits=16, export_edges=CHAIN, export_report=rep)
    assert [y.shape[0] for _, y, _ in got] == lens and [int(r["frames"]) for r in rep] == lens
    for (name, y, rate), n in zip(got, lens):
        q, sr, bits = read_wav_pcm(os.path.join(str(tmp_path), name))
        assert (q.shape, sr, bits) == ((n, 2), 48000, 16) and np.array_equal(q, y)
    with open(os.path.join(str(tmp_path), "loudness_report.csv")) as fh:
        lines = fh.read().splitlines()
    col = lines[0].split(",").index("frames")
    assert [int(l.split(",")[col]) for l in lines[1:]] == lens
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(*args, devices=[0, 1], export_edges=CHAIN)
