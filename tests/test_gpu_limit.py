"""The look-ahead limiter on the device (msg_limit, csrc/kernels_limit.h): samples and records
to the bit against the library's host loop (msg_limit_host) over ragged batches, with and
without the measured true-peak records, at the largest look-ahead, and end to end through
render_batch(out_limiter=...).  Signals and bounds: tests/limit_cases.py.  NaN frames lie around
and between the signals of every packed call, so an over-read shows as a state-2 record and
an over-write as changed bytes between the signals."""
import numpy as np
import pytest

import limit_cases as LC
import truepeak_cases as TC
import msgpu
from msgpu.limit import limit_host, limit_reference, lookahead_frames, records, tile
from msgpu.loudness import loudness_reference
from msgpu.truepeak import true_peak_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def batch(channels, sr, la):
    """A ragged batch: the edge lengths, an empty signal, one under the ceiling, one with a
    NaN, and the boundary-distance signals."""
    t = tile(la)
    sig = [LC.case(n, channels, sr, la)[0] for n in (0, 1, 25, t - 1, t + 1, 20011)]
    sig.append(TC.noise(t + 7, channels, 5))                          # under the ceiling
    bad = np.array(LC.spiky(t + 9, channels, 79))
    bad[t + 2] = np.nan
    sig.append(bad)
    return sig + LC.boundary_signals(la, channels)


def run(eng, signals, channels, sr, la, with_tp):
    """One msg_limit call over the packed signals: (buffer before, buffer after, offsets, lens, records)."""
    buf, offs, lens = LC.pack(signals, channels)
    x = eng.torch.from_numpy(buf).cuda()
    tp = eng.true_peak(x, offs, lens, channels, sr) if with_tp else None
    rec = eng.limit(x, offs, lens, channels, sr, LC.C, la, tp_rec=tp)
    return buf, x.cpu().numpy(), offs, lens, records(rec)


def check_equals_host(buf, got, offs, lens, rec, signals, sr, la, what):
    inside = np.zeros(len(buf), dtype=bool)
    for i, (s, o, n) in enumerate(zip(signals, offs, lens)):
        y, host = limit_host(s, sr, LC.CEILING_DB, lookahead=la)
        inside[o:o + n] = True
        assert np.array_equal(bits(got[o:o + n]), bits(y)), (what, i, n)
        assert rec[i].tobytes() == host.tobytes(), (what, i, n, rec[i], host)
    assert np.array_equal(bits(got[~inside]), bits(buf[~inside])), what       # the gaps keep their NaNs' bits


@pytest.mark.parametrize("la", LC.LOOKAHEADS)
@pytest.mark.parametrize("sr", LC.RATES)
@pytest.mark.parametrize("channels", [1, 2])
def test_device_equals_host(eng, channels, sr, la):
    sig = batch(channels, sr, la)
    buf, got, offs, lens, rec = run(eng, sig, channels, sr, la, False)
    check_equals_host(buf, got, offs, lens, rec, sig, sr, la, f"ch={channels} {sr} Hz L={la}")
    states = [int(r["state"]) for r in rec]
    assert states[:8] == [0, 1, 1, 1, 1, 1, 0, 2] and all(s == 1 for s in states[8:]), states
    n = len(sig[5])                                                   # and the long one against the reference
    x, y_ref, g_ref, border = LC.case(n, channels, sr, la)
    LC.check_against_reference(x, got[offs[5]:offs[5] + n], rec[5], sr, la, (y_ref, g_ref, border), "device")


@pytest.mark.parametrize("sr", [48000, 192000])
@pytest.mark.parametrize("channels", [1, 2])
def test_measured_records_change_nothing(eng, channels, sr):
    """With the signals' msg_truepeak records the under-ceiling ones are skipped on the device:
    the same bytes and records as without; under-ceiling signals keep their bytes."""
    la = 72
    sig = batch(channels, sr, la)
    buf, got, offs, lens, rec = run(eng, sig, channels, sr, la, False)
    buf2, got2, _, _, rec2 = run(eng, sig, channels, sr, la, True)
    assert np.array_equal(bits(got), bits(got2)) and rec.tobytes() == rec2.tobytes()
    check_equals_host(buf2, got2, offs, lens, rec2, sig, sr, la, f"tp_rec ch={channels} {sr} Hz")
    for i in (0, 6):
        o, n = offs[i], lens[i]
        assert rec2[i]["state"] == 0 and np.array_equal(bits(got2[o:o + n]), bits(buf[o:o + n]))


def test_largest_lookahead(eng):
    """L = 4096 at 384 kHz, one stereo signal of three tiles: the 16384-frame tile, the
    1024-thread workgroup and 139 KiB of LDS."""
    la, sr = 4096, 384000
    assert tile(la) == 16384 and lookahead_frames(sr, 10.0) < la
    x = LC.spiky(2 * tile(la) + 4001, 2, 4096)
    buf, got, offs, lens, rec = run(eng, [x], 2, sr, la, False)
    check_equals_host(buf, got, offs, lens, rec, [x], sr, la, "L=4096")
    assert rec[0]["state"] == 1 and rec[0]["lookahead"] == la


def test_public_limit(eng):
    x = np.array(LC.spiky(6000, 2, 80))
    y_host, r_host = limit_host(x, 48000, -1.0, 5.0)
    y, r = msgpu.limit(x, 48000)
    assert np.array_equal(bits(y), bits(y_host)) and r.tobytes() == r_host.tobytes() and r["lookahead"] == 240
    t = eng.torch.from_numpy(x).cuda()
    rec = msgpu.limit(t, 48000, -1.0, 5.0)
    assert isinstance(rec, eng.torch.Tensor) and rec.is_cuda
    assert records(rec)[0].tobytes() == r_host.tobytes() and np.array_equal(bits(t.cpu().numpy()), bits(y_host))
    with pytest.raises(NotImplementedError):
        eng.limit(t, [0], [6000], 2, 48000, LC.C, 4097)
    with pytest.raises(ValueError):
        eng.limit(t, [0], [6000], 2, 48000, 0.0, 12)
    with pytest.raises(ValueError):
        eng.limit(t, [0], [6000], 2, 48000, LC.C, 0)


# ---- end to end -------------------------------------------------------------------------------
SEED = 1003          # C1's crest factor at this seed is 27 dB: one gain for -1 dBTP leaves it LU short


def test_render_batch_with_the_limiter(irs):
    """C1 (1 s at 48 kHz) to R 128 with the limiter: under the ceiling, no quieter than the
    gain-only delivery, and as near the target as the float64 restatement of the chain gets
    from the same float32 render.  (C2, the export-chain tests' preset, has a crest factor
    under 7 dB at every seed tried and is never short of -23 LUFS under -1 dBTP, so it would
    show nothing; C1 is the smallest shipped preset, and at this seed one gain leaves it
    4.8 LU short.)"""
    sr, target, ceiling_db = 48000, -23.0, -1.0
    c = 10.0 ** (ceiling_db / 20.0)
    p = msgpu.config_params("C1", seed=SEED, irs=irs)
    rules = dict(out_sr=sr, out_lufs=target, out_true_peak=ceiling_db)
    plain = msgpu.render_batch([p])[0]
    gain_only = msgpu.render_batch([p], **rules)[0]
    limited = msgpu.render_batch([p], out_limiter=True, **rules)[0]
    l_gain, l_lim = loudness_reference(gain_only, sr), loudness_reference(limited, sr)
    tp = true_peak_reference(limited, sr)
    # the chain in float64 from the same render: level, limit, trim
    x = plain.astype(np.float64) * 10.0 ** ((target - loudness_reference(plain, sr)) / 20.0)
    y, _ = limit_reference(x, sr, c, lookahead_frames(sr, 5.0))
    y = y * min(1.0, c / true_peak_reference(y, sr))
    l_ref = loudness_reference(y, sr)
    print(f"C1 seed {SEED}: gain-only {l_gain:.3f} LUFS, limiter {l_lim:.3f} LUFS, float64 chain {l_ref:.3f} LUFS, "
          f"true peak {20 * np.log10(tp):+.4f} dBTP")
    assert target - l_gain >= 1.0                                     # the premise: the gain-only path is short
    assert tp <= c * (1 + TC.E_GAIN)
    assert l_lim >= l_gain
    assert target - l_lim <= max(0.0, target - l_ref) + 0.01
    pcm = msgpu.render_batch([p], out_limiter=True, out_bits=24, **rules)[0]
    assert pcm.dtype == np.int32 and pcm.shape == limited.shape and pcm.any()
    # the sample peak is under c (1 + 2^-22); TPDF dither and the rounding add at most 1.5 steps
    assert np.abs(pcm).max() <= c * (1 + 2.0 ** -22) * 2 ** 23 + 1.5
    same = msgpu.render_variations(p, [SEED], [p["time_unfold"]], [p["partial_stretch"]], export_sr=sr,
                                   export_lufs=target, export_true_peak=ceiling_db, export_limiter=True)
    assert np.array_equal(bits(same[0][1]), bits(limited))
