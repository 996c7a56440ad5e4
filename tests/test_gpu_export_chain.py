"""The delivery chain (msgpu/export.py) on the device: render_batch(out_...) and
render_variations(export_...) deliver the same integers through it, and the level passes'
shared per-rate loop gives every render the record and the samples of a call of its own."""
import numpy as np
import pytest

import msgpu
from msgpu.export import loudness_packed, truepeak_packed

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


@pytest.mark.parametrize("rule", ["lufs", "lufs+true_peak", "true_peak"])
def test_per_rate_loop_equals_one_call_per_signal(eng, bursts, rule):
    torch = eng.torch
    buf, offs, lens = bursts

    def level(y, o, n, rates):
        if rule == "lufs":
            return loudness_packed(eng, y, o, n, rates, -23.0)
        if rule == "lufs+true_peak":
            return loudness_packed(eng, y, o, n, rates, -23.0, None, -20.0)      # the ceiling binds: noise has a crest
        return truepeak_packed(eng, y, o, n, rates, -20.0)

    y = torch.from_numpy(buf).cuda()
    rec = level(y, offs, lens, RATES)
    assert tuple(rec.shape) == (len(RATES), 5)
    alone_y = torch.from_numpy(buf).cuda()
    alone = [level(alone_y, offs[i:i + 1], lens[i:i + 1], RATES[i:i + 1]) for i in range(len(RATES))]
    torch.cuda.synchronize()
    rec = rec.cpu().numpy().view(np.uint64)
    for i, r in enumerate(alone):                                                # render order, to the bit
        assert np.array_equal(rec[i], r.cpu().numpy().view(np.uint64)[0]), (rule, i)
    got = y.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), alone_y.cpu().numpy().view(np.uint32))
    gains = np.abs(got).max(axis=0).max() / np.abs(buf).max(axis=0).max()
    assert gains != 1.0                                                          # and it was scaled at all
