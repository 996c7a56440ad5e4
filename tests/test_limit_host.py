"""The look-ahead limiter on the host (msg_limit_host, csrc/limit.h) against the float64
restatement of its definition (msgpu.limit.limit_reference), its two guarantees, its
locality and NaN rules, the chain's trim on dense material, and the delivery rules of the new
option.  Signals and bounds: tests/limit_cases.py.  No GPU here."""
import ctypes as C

import numpy as np
import pytest

import limit_cases as LC
import truepeak_cases as TC
import msgpu
from msgpu import _lib as L
from msgpu.limit import (LIMIT_DTYPE, envelope_reference, limit_host, limit_reference, lookahead_frames, tile)
from msgpu.truepeak import Z, true_peak_host, true_peak_reference


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("la", LC.LOOKAHEADS)
@pytest.mark.parametrize("sr", LC.RATES)
def test_host_is_within_the_bound_of_the_reference(sr, la):
    for channels in (1, 2):
        for n in LC.lengths(la):
            x, y_ref, g_ref, border = LC.case(n, channels, sr, la)
            y, rec = limit_host(x, sr, LC.CEILING_DB, lookahead=la)
            what = f"{sr} Hz L={la} ch={channels} n={n}"
            LC.check_against_reference(x, y, rec, sr, la, (y_ref, g_ref, border), what)
            assert y.shape == x.shape and y.dtype == np.float32
            if n >= 12:
                assert rec["state"] == 1, what                            # the spikes are over the ceiling


@pytest.mark.parametrize("la", LC.LOOKAHEADS)
@pytest.mark.parametrize("channels", [1, 2])
def test_boundary_distances(channels, la):
    """One over-ceiling frame at each distance from a tile boundary: the host has no tiles, so
    this pins the signals the device test compares with, and their reach to the frame."""
    for x in LC.boundary_signals(la, channels):
        y, rec = limit_host(x, 48000, LC.CEILING_DB, lookahead=la)
        LC.check_against_reference(x, y, rec, 48000, la, what=f"L={la} ch={channels}")
        e = envelope_reference(x, 48000)
        over = np.flatnonzero(e > LC.C)
        assert 1 <= len(over) <= 3 and rec["state"] == 1
        reach = 2 * la + Z
        assert rec["limited_frames"] == min(over[-1] + reach, len(x) - 1) - max(over[0] - reach, 0) + 1


@pytest.mark.parametrize("la", LC.LOOKAHEADS)
@pytest.mark.parametrize("sr", [48000, 96000])
def test_isolated_peaks_come_out_at_the_ceiling(sr, la):
    for name, x, ceiling_db in (("pair", TC.pair_signal(3000, 1500, 1), -1.0),
                                ("pair stereo", TC.pair_signal(3000, 1500, 2), -1.0),
                                ("faded sine", TC.faded_sine(), -8.0)):
        c = 10.0 ** (ceiling_db / 20.0)
        before = true_peak_reference(x, sr)
        y, rec = limit_host(x, sr, ceiling_db, lookahead=la)
        after = true_peak_reference(y, sr)
        print(f"{name} {sr} Hz L={la}: true peak {before:.6f} -> {after:.9f}, c {c:.9f}, relative {after / c - 1:+.3e}")
        if before > c * (1 + TC.E_GAIN):
            assert rec["state"] == 1
            assert c * (1 - TC.E_GAIN) <= after <= c * (1 + TC.E_GAIN), (name, after / c - 1)
        else:                                                    # the pair at 96 kHz may read under the ceiling
            assert after <= c * (1 + TC.E_GAIN)


@pytest.mark.parametrize("channels", [1, 2])
def test_untouched_signals_keep_their_bytes(channels):
    for sr in LC.RATES:
        x = TC.noise(5000, channels, 5)                            # peaks near 0.45: under -1 dBTP
        assert true_peak_reference(x, sr) < LC.C * 0.9
        y, rec = limit_host(x, sr, LC.CEILING_DB, lookahead=72)
        assert np.array_equal(bits(y), bits(x))
        assert (rec["state"], rec["limited_frames"], rec["min_gain"], rec["reduction_db"], rec["lookahead"]) == \
            (0, 0, 1.0, 0.0, 72)
    y, rec = limit_host(np.zeros((0, 2) if channels == 2 else 0, dtype=np.float32), 48000, LC.CEILING_DB)
    assert y.shape[0] == 0 and rec["state"] == 0 and rec["lookahead"] == 240 and rec["min_gain"] == 1.0


@pytest.mark.parametrize("la", [1, 72])
def test_locality(la):
    """Frames farther than 2 L + Z + 1 from every over-ceiling frame keep their bits; nearer
    ones are written (a zero sample stays a zero)."""
    for sr in LC.RATES:
        x, _, _, _ = LC.case(20011, 2, sr, la)
        y, rec = limit_host(x, sr, LC.CEILING_DB, lookahead=la)
        over = np.flatnonzero(envelope_reference(x, sr) > LC.C * (1 + TC.E))
        dist = np.abs(np.arange(len(x))[:, None] - over[None, :]).min(axis=1)
        far = dist > 2 * la + Z + 1
        assert far.any() and np.array_equal(bits(y)[far], bits(x)[far])
        near = dist <= 2 * la + Z
        assert (bits(y)[near] != bits(x)[near]).any(axis=1).all()


def test_stereo_link():
    """A silent right channel: the left channel gets the mono result's bits."""
    for sr in LC.RATES:
        mono = LC.spiky(6000, 1, 77)
        st = np.stack([mono, np.zeros_like(mono)], axis=1)
        ym, rm = limit_host(mono, sr, LC.CEILING_DB, lookahead=12)
        ys, rs = limit_host(st, sr, LC.CEILING_DB, lookahead=12)
        assert np.array_equal(bits(ys[:, 0]), bits(ym)) and not ys[:, 1].any()
        assert rm.tobytes() == rs.tobytes() and rm["state"] == 1


def test_nan_leaves_the_signal_as_it_was():
    for sr in LC.RATES:
        x = np.array(LC.spiky(6000, 2, 78))
        x[4000, 1] = np.nan
        y, rec = limit_host(x, sr, LC.CEILING_DB, lookahead=12)
        assert np.array_equal(bits(y), bits(x))
        assert (rec["state"], rec["limited_frames"], rec["min_gain"]) == (2, 0, 1.0)


def test_dense_material_overshoots_and_the_trim_closes_it():
    """Dense over-ceiling material at L = 2: the gain moves inside the interpolator's window, so
    the limiter alone may leave the true peak over the ceiling (printed, not required); the
    chain's trim, true_peak_host plus one float32 gain, holds it."""
    sr, x = 48000, LC.dense(8000)
    y, rec = limit_host(x, sr, LC.CEILING_DB, lookahead=2)
    assert float(np.max(np.abs(y))) <= LC.PEAK_ROOF and rec["state"] == 1
    after = true_peak_reference(y, sr)
    print(f"dense, L=2: true peak {true_peak_reference(x, sr):.4f} -> {after:.6f} = {after / LC.C:.4f} c after the limiter alone")
    t = true_peak_host(y, sr)
    g = np.float32(LC.C / t["true_peak"]) if t["true_peak"] > LC.C else np.float32(1.0)
    trimmed = y * g
    assert true_peak_reference(trimmed, sr) <= LC.C * (1 + TC.E_GAIN)


def _host_status(x, channels, n, sr, ceiling, la):
    rec = np.zeros(1, dtype=LIMIT_DTYPE)
    return L.lib().msg_limit_host(x.ctypes.data_as(C.c_void_p), channels, n, sr, ceiling, la,
                                  rec.ctypes.data_as(C.c_void_p))


def test_value_rules():
    x = np.zeros(64, dtype=np.float32)
    assert _host_status(x, 1, 32, 48000, 0.9, 12) == L.MSG_OK
    for bad in (0.0, -0.5, float("nan"), float("inf"), 1e-60, 1e60):
        assert _host_status(x, 1, 32, 48000, bad, 12) == L.MSG_E_VALUE, bad
    assert _host_status(x, 1, 32, 48000, 0.9, 0) == L.MSG_E_VALUE
    assert _host_status(x, 1, 32, 48000, 0.9, -3) == L.MSG_E_VALUE
    assert _host_status(x, 1, 32, 48000, 0.9, 4096) == L.MSG_OK
    assert _host_status(x, 1, 32, 48000, 0.9, 4097) == L.MSG_E_UNSUPPORTED
    assert _host_status(x, 3, 16, 48000, 0.9, 12) == L.MSG_E_VALUE
    assert _host_status(x, 1, 32, 0, 0.9, 12) == L.MSG_E_VALUE
    assert _host_status(x, 1, -1, 48000, 0.9, 12) == L.MSG_E_ARG
    with pytest.raises(NotImplementedError):
        limit_host(x, 48000, -1.0, lookahead=5000)
    with pytest.raises(ValueError):
        limit_host(x, 48000, float("nan"))
    assert lookahead_frames(48000, 5.0) == 240 and lookahead_frames(48000, 0.001) == 1 and lookahead_frames(384000, 10) == 3840
    assert [tile(v) for v in (1, 256, 257, 512, 513, 1024, 1025, 4096)] == [2048, 2048, 4096, 4096, 8192, 8192, 16384, 16384]
    assert L.lib().msg_sizeof(7) == C.sizeof(L.MsgLimitRec) == LIMIT_DTYPE.itemsize == 32


VE, NIE = ValueError, NotImplementedError


@pytest.mark.parametrize("prefix", ["out_", "export_"])
def test_delivery_rules(prefix):
    from msgpu.export import Delivery
    with pytest.raises(VE, match=f"{prefix}limiter needs {prefix}true_peak"):
        Delivery(lufs=-23.0, limiter=True).check(prefix)
    for bad in (False, 0, -5.0, float("nan"), float("inf"), "fast", [5]):
        with pytest.raises(VE, match=f"{prefix}limiter must be"):
            Delivery(true_peak=-1.0, limiter=bad).check(prefix)
    with pytest.raises(NIE, match=f"{prefix}limiter on more than one"):
        Delivery(limiter=True).one_device(prefix, 2, ("limiter",))
    with pytest.raises(NIE):
        Delivery(true_peak=-1.0, limiter=True).check(prefix, n_devices=2)
    with pytest.raises(VE, match="applies to results"):
        Delivery(true_peak=-1.0, limiter=True).check(prefix, "stats")
    for good, ms in ((True, 5.0), (1.5, 1.5), (3, 3.0)):
        d = Delivery(48000, None, -23.0, None, -1.0, 24, "tpdf", 0, good)
        d.check(prefix)
        assert d.limiter_ms() == ms
    assert Delivery(limiter=None).limiter_ms() is None
    # callers build Delivery positionally: the field is the last, and None is today's delivery
    assert Delivery(48000, None, -23.0, 0.9, -1.0, 24, "none", 7) == Delivery(48000, None, -23.0, 0.9, -1.0, 24, "none", 7, None)
    assert Delivery(48000, None, -23.0, 0.9, -1.0, 24, "none", 7, limiter=None) == Delivery(48000, None, -23.0, 0.9, -1.0, 24, "none", 7)


def test_front_ends_refuse_before_any_device_call():
    p = dict(msgpu.DEFAULTS)
    with pytest.raises(VE, match="out_limiter needs out_true_peak"):
        msgpu.render_batch([p], out_limiter=True)
    with pytest.raises(VE, match="export_limiter needs export_true_peak"):
        msgpu.render_variations(p, [1000], [1.0], [1.0], export_limiter=2.5)
    with pytest.raises(NIE):
        msgpu.render_batch([p], devices=[0, 1], out_true_peak=-1.0, out_limiter=True)
    with pytest.raises(NIE, match="out_limiter on more than one"):
        msgpu.render_batch([p], devices=[0, 1], out_limiter=True)
    with pytest.raises(VE):
        msgpu.render_batch([p], results="stats", out_true_peak=-1.0, out_limiter=True)


# ---- the header under the sanitizers -----------------------------------------------------------
@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
def test_host_loop_under_asan_ubsan(tmp_path):
    """csrc/limit.h in a stand-alone program (tests/limit_check.cpp) under ASan + UBSan: the
    weight table, the host loop in place on exactly-sized heap blocks at the edge lengths,
    the sample-peak guarantee, the NaN rule, the largest look-ahead."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "limit_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(repo, "audio-suite_amd", "csrc"),
                    "-o", exe, os.path.join(repo, "tests", "limit_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "bad 0" in out, out[-4000:]
