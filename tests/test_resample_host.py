"""Host side of the resampler (msgpu/resample.py): the filter design, the float64
restatement of the formula against scipy, the helpers, and the export rate in
file names and WAV headers.  No GPU."""
import numpy as np
import pytest

import msgpu
from msgpu import batch
from msgpu.resample import design, ratio, resample_len, resample_reference, tile_frames


@pytest.mark.parametrize("up,down", [(1, 8), (147, 1280), (160, 147)])
def test_design(up, down):
    h = design(up, down)
    D = max(up, down)
    assert h.dtype == np.float64 and h.size == 2 * 32 * D + 1
    assert np.array_equal(h, h[::-1])
    assert abs(h.sum() - 1.0) <= 1e-12
    # response on a zero-padded FFT; f in units of the lower Nyquist rate: bin b of N is f = 2 D b / N
    N = 1 << int(np.ceil(np.log2(h.size * 16)))
    H = np.abs(np.fft.rfft(h, N))
    f = 2.0 * D * np.arange(H.size) / N
    db = 20 * np.log10(np.maximum(H, 1e-300))
    ripple = float(np.max(np.abs(db[f <= 0.8])))
    stop = float(np.max(db[f >= 1.1]))
    print(f"design {up}/{down}: ripple {ripple:.4f} dB, stop band {stop:.1f} dB")
    assert ripple <= 0.01
    assert stop <= -115.0


@pytest.mark.parametrize("up,down", [(1, 8), (147, 160), (160, 147), (147, 1280), (3, 2), (2, 1)])
@pytest.mark.parametrize("n", [1, 7, 333, 3000])
def test_reference_matches_scipy(up, down, n):
    signal = pytest.importorskip("scipy.signal")
    h = design(up, down)
    x = np.random.default_rng(n * 1000 + up).standard_normal(n)
    want = signal.resample_poly(x, up, down, window=h)
    got = resample_reference(x, up, down, h)
    assert got.shape == want.shape == (resample_len(n, up, down),)
    err = float(np.max(np.abs(got - want)))
    print(f"reference vs scipy {up}/{down} n={n}: {err:.2e}")
    assert err <= 1e-12


def test_reference_channels():
    h = design(1, 2)
    x = np.random.default_rng(3).standard_normal((50, 2))
    y = resample_reference(x, 1, 2, h)
    assert y.shape == (25, 2)
    assert np.array_equal(y[:, 1], resample_reference(x[:, 1], 1, 2, h))


def test_helpers():
    assert ratio(384000, 48000) == (1, 8)
    assert ratio(384000, 44100) == (147, 1280)
    assert ratio(44100, 48000) == (160, 147)
    assert ratio(48000, 48000) == (1, 1)
    assert ratio(48000, 96000) == (2, 1)
    with pytest.raises(ValueError):
        ratio(0, 48000)
    assert resample_len(16, 1, 8) == 2
    assert resample_len(17, 1, 8) == 3
    assert resample_len(1, 1, 8) == 1
    assert resample_len(0, 1, 8) == 0
    assert resample_len(160, 147, 160) == 147
    assert resample_len(161, 147, 160) == 148
    assert resample_len(7, 2, 1) == 14
    assert resample_len(20011, 147, 1280) == -(-20011 * 147 // 1280)


def test_tiles_and_limits():
    from msgpu.resample import TILE_DECIMATE
    assert tile_frames(1, 8, 513, 2) == TILE_DECIMATE == tile_frames(1, 2, 129, 1)
    assert tile_frames(147, 160, 10241, 2) == 4 * 147
    assert tile_frames(2, 1, 129, 2) == 4 * 256
    # every pair of the supported rates fits, mono and stereo
    rates = (44100, 48000, 88200, 96000, 176400, 192000, 384000)
    for a in rates:
        for b in rates:
            if a != b:
                up, down = ratio(a, b)
                assert max(up, down) <= 1280
                for ch in (1, 2):
                    assert tile_frames(up, down, 64 * max(up, down) + 1, ch) > 0
    with pytest.raises(NotImplementedError):
        up, down = ratio(44100, 48001)
        tile_frames(up, down, 64 * max(up, down) + 1, 2)


def test_names_and_headers_carry_the_export_rate(tmp_path):
    assert batch.variant_name(7, 10.0, 1.0, 48000) == "ms_seed7_unf10_st1_48000Hz.wav"
    a = np.zeros((5, 2), dtype=np.float32)
    a[2, 1] = 0.5
    path = tmp_path / "x.wav"
    batch.write_wav_float32(str(path), a, 48000)
    back, sr = batch.read_wav_float32(str(path))
    assert sr == 48000 and np.array_equal(back, a)


def test_multi_device_export_is_refused_before_any_gpu():
    base = dict(msgpu.DEFAULTS)
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(base, [1000, 1001], [10], [1], export_sr=48000, devices=[0, 1])
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([base], devices=[0, 1], out_sr=48000)
    with pytest.raises(ValueError):
        msgpu.render_variations(base, [1000], [10], [1], export_peak="preset")
