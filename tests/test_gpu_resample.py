"""Device resampler (msg_resample, csrc/kernels_resample.h) against the float64
reference: scipy.signal.resample_poly with the same taps (msgpu.resample's float64
restatement where scipy is missing; tests/test_resample_host.py holds the two to
1e-12 of each other).  Bar: the project's float32 bar, REL = 1e-5 relative RMS per
channel."""
import math
import os

import numpy as np
import pytest

import msgpu
from msgpu.resample import design, ratio, resample_len, resample_reference, tile_frames

pytestmark = pytest.mark.gpu
REL = 1e-5


def reference(x, up, down, h):
    x = np.asarray(x, dtype=np.float64)
    try:
        from scipy.signal import resample_poly
    except ImportError:
        return resample_reference(x, up, down, h)
    if up == down:
        return x.copy()
    return resample_poly(x, up, down, axis=0, window=h)


def rel_rms(got, want):
    got = np.asarray(got, dtype=np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2)) / max(np.sqrt(np.mean(want ** 2)), 1e-300))


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(20011).standard_normal((20011, 2)).astype(np.float32)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("sr_in,sr_out", [(384000, 48000), (384000, 44100), (48000, 44100), (44100, 48000),
                                          (48000, 96000), (96000, 48000)])
def test_ratios(noise, sr_in, sr_out, channels):
    x = noise[:, 0].copy() if channels == 1 else noise
    up, down = ratio(sr_in, sr_out)
    y = msgpu.resample(x, sr_in, sr_out)
    assert y.dtype == np.float32
    assert y.shape == (resample_len(len(x), up, down),) + x.shape[1:]
    assert np.isfinite(y).all()
    want = reference(x, up, down, design(up, down))
    for c in range(channels):
        err = rel_rms(y[:, c] if channels == 2 else y, want[:, c] if channels == 2 else want)
        print(f"resample {sr_in}->{sr_out} ch {c + 1}/{channels}: rel rms {err:.2e}")
        assert err <= REL


@pytest.mark.parametrize("up,down,lengths", [(1, 8, (1, 2, 7, 8, 9, 255, 256, 257, 513)),
                                             (147, 160, (1, 159, 160, 161))])
def test_short_and_edge_lengths(up, down, lengths):
    h = design(up, down)
    rng = np.random.default_rng(7)
    for n in lengths:
        for channels in (1, 2):
            x = rng.standard_normal((n, 2) if channels == 2 else n).astype(np.float32)
            y = msgpu.resample(x, down, up)          # the rates only set the ratio
            want = reference(x, up, down, h)
            assert y.shape == want.shape
            err = float(np.max(np.abs(y - want)))
            bound = 1e-5 * float(np.max(np.abs(want)))
            print(f"resample {up}/{down} n={n} ch={channels}: max err {err:.2e} (bound {bound:.2e})")
            assert err <= bound


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("up,down", [(1, 8), (147, 160)])
def test_impulses(eng, up, down, channels):
    """A unit impulse at input frame m gives y[k] = up h[k down + half - m up]: the ends
    and the input frames either side of every output-tile boundary, one signal each
    in a ragged batch.  Pins the index arithmetic."""
    torch = eng.torch
    h = design(up, down)
    K, half = h.size, (h.size - 1) // 2
    tile = tile_frames(up, down, K, channels)
    n = -(-(3 * tile + 5) * down // up)              # the output spans three tiles and five frames
    n_out = resample_len(n, up, down)
    assert 3 * tile + 5 <= n_out < 4 * tile
    at = {0, n - 1}
    for b in (tile, 2 * tile, 3 * tile):
        m = b * down // up
        at |= {m - 1, m, m + 1}
    at = sorted(at)
    shape = (len(at), n, 2) if channels == 2 else (len(at), n)
    x = np.zeros(shape, dtype=np.float32)
    for i, m in enumerate(at):
        if channels == 2:
            x[i, m] = (1.0, -0.5)
        else:
            x[i, m] = 1.0
    y, off, cnt = eng.resample(torch.from_numpy(x).cuda().reshape((-1, 2) if channels == 2 else -1),
                               np.arange(len(at)) * n, [n] * len(at), channels, up, down, h)
    torch.cuda.synchronize()
    y = y.cpu().numpy().astype(np.float64)
    t_all = np.arange(n_out) * down + half
    worst = 0.0
    for i, m in enumerate(at):
        t = t_all - m * up
        want = np.where((t >= 0) & (t < K), up * h[np.clip(t, 0, K - 1)], 0.0)
        got = y[off[i]:off[i] + cnt[i]]
        assert cnt[i] == n_out
        if channels == 2:
            worst = max(worst, float(np.max(np.abs(got[:, 0] - want))), float(np.max(np.abs(got[:, 1] + 0.5 * want))))
        else:
            worst = max(worst, float(np.max(np.abs(got - want))))
    print(f"impulses {up}/{down} ch={channels} tile {tile}: worst {worst:.2e}")
    assert worst <= 2e-7


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("up,down", [(1, 8), (147, 160)])
def test_ragged_batch(eng, up, down, channels):
    h = design(up, down)
    ragged_batch(eng, up, down, channels, h, [1, 4097, 30001, 8, 12345])
    # signals without a tile share their successor's first tile: outputs of 0, 1, tile, 0, tile + 1, 0 frames
    tile = tile_frames(up, down, h.size, channels)
    lens = [0, 1, tile * down // up, 0, (tile + 1) * down // up, 0]
    assert [resample_len(n, up, down) for n in lens] == [0, 1, tile, 0, tile + 1, 0]
    ragged_batch(eng, up, down, channels, h, lens)


def ragged_batch(eng, up, down, channels, h, lens):
    torch = eng.torch
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])        # back to back: mono rows start at odd floats
    rng = np.random.default_rng(5)
    x = rng.standard_normal((sum(lens), 2) if channels == 2 else sum(lens)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    total = sum(resample_len(n, up, down) for n in lens)
    guard = 1000
    out = torch.full((total + guard, 2) if channels == 2 else (total + guard,), float("nan"),
                     dtype=torch.float32, device="cuda")
    y, yo, yn = eng.resample(xd, offs, lens, channels, up, down, h, out=out)
    assert y is out
    alone = [eng.resample(xd[o:o + n].clone(), [0], [n], channels, up, down, h)[0].cpu().numpy() if n else x[:0]
             for o, n in zip(offs, lens)]
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert np.isnan(y[total:]).all()                          # the guard after the last output
    assert np.isfinite(y[:total]).all()
    for i, (o, n) in enumerate(zip(offs, lens)):
        got = y[yo[i]:yo[i] + yn[i]]
        assert got.shape == alone[i].shape and np.array_equal(got, alone[i])
        if n == 0:
            continue
        want = reference(x[o:o + n], up, down, h)
        for c in range(channels):
            err = rel_rms(got[:, c] if channels == 2 else got, want[:, c] if channels == 2 else want)
            print(f"ragged {up}/{down} ch={channels} n={n}: rel rms {err:.2e}")
            assert err <= REL


def test_stop_band_and_pass_band():
    n, sr_in, sr_out = 96000, 384000, 48000
    t = np.arange(n) / sr_in
    edge = 100                                                # output frames dropped at each end (half a filter is 32)
    y = msgpu.resample(np.sin(2 * np.pi * 30000.0 * t).astype(np.float32), sr_in, sr_out)
    rms = float(np.sqrt(np.mean(y[edge:-edge].astype(np.float64) ** 2)))
    print(f"30 kHz at 384 kHz -> 48 kHz: interior rms {20 * math.log10(max(rms, 1e-300)):.1f} dBFS")
    assert rms <= 1e-5                                        # -100 dBFS
    y = msgpu.resample(np.sin(2 * np.pi * 1000.0 * t).astype(np.float32), sr_in, sr_out)
    ideal = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / sr_out)
    err = float(np.max(np.abs(y[edge:-edge] - ideal[edge:-edge])))
    print(f"1 kHz at 384 kHz -> 48 kHz: max interior error {err:.2e}")
    assert err <= 1e-5


def test_copy_and_device_tensor(eng):
    torch = eng.torch
    x = np.random.default_rng(1).standard_normal((1000, 2)).astype(np.float32)
    y = msgpu.resample(x, 48000, 48000)
    assert np.array_equal(y, x)
    xd = torch.from_numpy(x).cuda()
    yd = msgpu.resample(xd, 96000, 48000)
    assert isinstance(yd, torch.Tensor) and yd.is_cuda and yd.shape == (500, 2)
    assert np.array_equal(yd.cpu().numpy(), msgpu.resample(x, 96000, 48000))


def test_errors(eng):
    torch = eng.torch
    h = design(1, 8)
    x = torch.zeros(4096, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError):
        eng.resample(x, [0], [4096], 1, 1, 8, h, out=x)       # out aliases the input
    with pytest.raises(ValueError):
        msgpu.resample(np.zeros((64, 3), dtype=np.float32), 384000, 48000)
    with pytest.raises(ValueError):
        eng.resample(x, [0], [1024], 3, 1, 8, h)
    with pytest.raises(ValueError):
        eng.resample(x, [0], [4096], 1, 1, 8, h[:-1])         # even tap count
    with pytest.raises(NotImplementedError):
        msgpu.resample(np.zeros(64, dtype=np.float32), 44100, 48001)
    up, down = ratio(44100, 48001)                            # the library's own limit, past the Python check
    with pytest.raises(NotImplementedError):
        eng.resample(x, [0], [4096], 1, up, down, np.zeros(64 * up + 1))
    torch.cuda.synchronize()


def test_render_variations_export(irs, tmp_path):
    from msgpu import batch
    base = msgpu.config_params("C2", seed=1000, irs=irs, out_dur_s=0.25)
    assert base["base_sr"] == 192000
    seeds = [1000, 1001]
    plain = msgpu.render_variations(base, seeds, [10], [1])
    again = msgpu.render_variations(base, seeds, [10], [1], export_sr=None)
    for (na, a, sa), (nb, b, sb) in zip(plain, again):
        assert na == nb and sa == sb == 192000 and np.array_equal(a, b)
    out_n = plain[0][1].shape[0]
    got = msgpu.render_variations(base, seeds, [10], [1], folder=str(tmp_path), export_sr=48000)
    assert len(got) == 2
    for (name, y, sr), (_, a, _) in zip(got, plain):
        assert name.endswith("_48000Hz.wav") and sr == 48000
        assert y.shape == (-(-out_n // 4), 2) and y.dtype == np.float32
        back, rate = batch.read_wav_float32(os.path.join(str(tmp_path), name))
        assert rate == 48000 and np.array_equal(back, y)
        assert np.array_equal(y, msgpu.resample(a, 192000, 48000))
    peaked = msgpu.render_variations(base, seeds, [10], [1], export_sr=48000, export_peak="preset")
    for (_, y, _), (_, raw, _) in zip(peaked, got):
        m = float(np.max(np.abs(y)))
        print(f"export peak {m:.8f} (preset {base['peak']}, as resampled {float(np.max(np.abs(raw))):.6f})")
        assert abs(m - float(base["peak"])) <= 1e-6
    dev = msgpu.render_batch([dict(base, seed=s) for s in seeds], results="device", out_sr=48000)
    for d, (_, y, _) in zip(dev, got):
        assert d.is_cuda and tuple(d.shape) == y.shape
