"""The delivery chain (msgpu/export.py) on the device: render_batch(out_...) and
render_variations(export_...) deliver the same integers through it, and the passes' one
per-rate driver gives every render the records, the extents and the samples of a call of its own."""
import numpy as np
import pytest

import msgpu
from msgpu.export import edges_packed, limiter_packed, loudness_packed, report_packed, truepeak_packed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def test_both_front_ends_deliver_the_same_integers(irs):
    """C2 at its own length (1 s: seven gating blocks at the delivered rate), resampled,
    levelled to R 128 under -1 dBTP and quantised to 24 bits with TPDF dither: render_batch keys
    the dither by the preset's index, render_variations by the variant's, and both get the same
    order here.  The loudness rule has to have acted: the delivery measures -23 LUFS (or less,
    where the ceiling holds it) and differs from the one without the rule."""
    seeds = [1000, 1001]
    c2 = msgpu.config_params("C2", irs=irs)
    ps = [msgpu.config_params("C2", seed=s, irs=irs) for s in seeds]
    rules = dict(out_sr=48000, out_true_peak=-1, out_bits=24, out_dither_seed=21)
    batch = msgpu.render_batch(ps, out_lufs=-23, **rules)
    unlevelled = msgpu.render_batch(ps, **rules)
    for a, u in zip(batch, unlevelled):
        lufs = msgpu.loudness(a.astype(np.float32) / np.float32(1 << 23), 48000)
        print(f"delivered at {lufs:.3f} LUFS, {int((a != u).sum())} of {a.size} words differ from the unlevelled delivery")
        assert np.isfinite(lufs) and lufs <= -23.0 + 0.01 and not np.array_equal(a, u)
    variations = msgpu.render_variations(c2, seeds, [c2["time_unfold"]], [c2["partial_stretch"]], export_sr=48000,
                                         export_lufs=-23, export_true_peak=-1, export_bits=24, export_dither_seed=21)
    assert len(batch) == len(variations) == len(seeds)
    for a, (name, b, rate) in zip(batch, variations):
        assert rate == 48000 and a.dtype == b.dtype == np.int32 and a.shape == b.shape and a.shape[1] == 2
        assert a.any() and np.array_equal(a, b), name


RATES = [44100, 48000, 48000, 44100]          # the zero-length signal goes in front of the second, at its rate


@pytest.fixture(scope="module")
def bursts():
    """Three noise bursts of 4 hops + 1 frame (exactly one gating block each) and an empty
    signal, back to back in one buffer: (buffer, offsets, lens).  Do not write to it."""
    rng = np.random.default_rng(20011)
    lens = [4 * (sr // 10) + 1 for sr in RATES]
    lens[1] = 0
    sig = [(0.1 * (i + 1) * rng.standard_normal((n, 2))).astype(np.float32) for i, n in enumerate(lens)]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return np.concatenate(sig), offs, np.array(lens, dtype=np.int64)


def _burst_batch(frames, pad_ms=(0, 0)):
    """Noise bursts of frames[i] frames at RATES[i], 0.1 (i + 1) loud, each non-empty one between
    pad_ms of zeros, back to back in one buffer: (buffer, offsets, lens)."""
    rng = np.random.default_rng(20011)
    sig = []
    for i, (n, sr) in enumerate(zip(frames, RATES)):
        head, tail = ((sr * ms) // 1000 if n else 0 for ms in pad_ms)
        noise = (0.1 * (i + 1) * rng.standard_normal((n, 2))).astype(np.float32)
        sig.append(np.concatenate([np.zeros((head, 2), np.float32), noise, np.zeros((tail, 2), np.float32)]))
    lens = np.array([len(x) for x in sig], dtype=np.int64)
    return np.concatenate(sig), np.cumsum(lens) - lens, lens


@pytest.fixture(scope="module")
def padded_bursts():
    """``bursts`` with 10 ms of zeros in front of, and 20 ms behind, each non-empty signal.  Do not write to it."""
    return _burst_batch([0 if i == 1 else 4 * (sr // 10) + 1 for i, sr in enumerate(RATES)], (10, 20))


@pytest.fixture(scope="module")
def meter_bursts():
    """33 hops + 1 frame, nothing, 4 hops + 1 frame and exactly 30 hops: a signal with several
    short-term windows, an empty one, one with none and one with exactly one.  Do not write to it."""
    hops = [sr // 10 for sr in RATES]
    return _burst_batch([33 * hops[0] + 1, 0, 4 * hops[2] + 1, 30 * hops[3]])


EDGES = msgpu.Edges(trim_db=-60, pad_ms=(1, 1), fade_ms=(2, 5))


def _level(eng, rule, y, o, n, rates):
    """One pass of the chain over the signals given, through the per-rate driver: what it returns per
    signal, {name: rows in signal order} (device tensors or host arrays)."""
    if rule == "lufs":
        return {"rec": loudness_packed(eng, y, o, n, rates, -23.0)}
    if rule == "lufs+true_peak":
        return {"rec": loudness_packed(eng, y, o, n, rates, -23.0, None, -20.0)}      # the ceiling binds: noise has a crest
    if rule == "true_peak":
        return {"rec": truepeak_packed(eng, y, o, n, rates, -20.0)}
    if rule in ("limiter", "lufs+limiter"):
        return {"rec": limiter_packed(eng, y, o, n, rates, -20.0, 5.0, -23.0 if rule == "lufs+limiter" else None)}
    if rule == "edges":
        off, cnt, rec = edges_packed(eng, y, o, n, rates, EDGES)
        return {"rec": rec, "offsets": off, "lens": cnt}
    rows = report_packed(eng, y, o, n, rates).rows()
    return {k: rows[k] for k in rows.dtype.names}


def _bits(v):
    """v (a device tensor or a host array) on the host, floats as the unsigned words they are."""
    a = np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


COLUMNS = {"lufs": 5, "lufs+true_peak": 5, "true_peak": 5, "limiter": 4, "lufs+limiter": 4, "edges": 8}
FIXTURE = {"edges": "padded_bursts", "report": "meter_bursts"}


@pytest.mark.parametrize("rule", ["lufs", "lufs+true_peak", "true_peak", "limiter", "lufs+limiter", "edges", "report"])
def test_per_rate_loop_equals_one_call_per_signal(eng, request, rule):
    """Every pass that goes through export.per_rate, over the mixed-rate batch and over each signal
    alone: the records, extents and samples of a render are those of a call of its own, in render
    order, to the bit (one rate's renders are [0, 3]: the scatter is not the identity).
    resample_packed, which shares only the grouping, has no case here: alone, the empty signal
    makes an empty output tensor, whose null pointer msg_resample refuses ("bad arguments")."""
    torch = eng.torch
    buf, offs, lens = request.getfixturevalue(FIXTURE.get(rule, "bursts"))
    y = torch.from_numpy(buf).cuda()
    batch = _level(eng, rule, y, offs, lens, RATES)
    if rule in COLUMNS:
        assert tuple(batch["rec"].shape) == (len(RATES), COLUMNS[rule])
    alone_y = torch.from_numpy(buf).cuda()
    alone = [_level(eng, rule, alone_y, offs[i:i + 1], lens[i:i + 1], RATES[i:i + 1]) for i in range(len(RATES))]
    torch.cuda.synchronize()
    for name, rows in batch.items():
        assert len(rows) == len(RATES), name
        for i, r in enumerate(alone):                                            # render order, to the bit
            assert np.array_equal(_bits(rows[i]), _bits(r[name][0])), (rule, name, i)
    got = y.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), alone_y.cpu().numpy().view(np.uint32))
    changed = not np.array_equal(got.view(np.uint32), buf.view(np.uint32))
    if rule in ("lufs", "lufs+true_peak", "true_peak"):
        gains = np.abs(got).max(axis=0).max() / np.abs(buf).max(axis=0).max()
        assert gains != 1.0                                                      # and it was scaled at all
    elif rule in ("limiter", "lufs+limiter"):
        from msgpu.limit import records
        limited = records(batch["rec"])["limited_frames"]
        print(f"{rule}: limited frames per render {limited.tolist()}")
        assert changed and (limited > 0).any()                                   # and the limiter had frames to hold
    elif rule == "edges":
        print(f"edges: spans {batch['lens'].tolist()} of {lens.tolist()} frames")
        assert changed and (batch["lens"][lens > 0] < lens[lens > 0]).all()      # trimmed, and faded
    else:
        assert not changed                                                       # the meters change no sample
