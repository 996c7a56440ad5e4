"""Noise-shaped dither on the host: msg_quantize_shaped_host (csrc/pcm_shape.h) against
msgpu.pcm.quantize_shaped_reference (the definition in NumPy) for equal bits, the chain's
causality and channel independence, NaN and infinities, the error's spectrum against the
noise transfer function, what shaping keeps of TPDF's properties, and the rule table.
Signals: tests/pcm_shape_cases.py."""
import os
import re

import numpy as np
import pytest

import pcm_shape_cases as SC
import msgpu
from msgpu import pcm
from msgpu.pcm import PCM_DTYPE, quantize_host, quantize_shaped_host, quantize_shaped_reference

N = 65536
E_BOUND = 3 << 23                                            # |E| < 1.5 2^24
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SC.NAMES)
@pytest.mark.parametrize("mode", SC.DITHERS)
@pytest.mark.parametrize("bits", SC.BITS)
@pytest.mark.parametrize("channels", [1, 2])
def test_host_equals_reference(channels, bits, mode, shape):
    xs = SC.signals(channels)
    keys = [3 + 5 * i for i in range(len(xs))]
    qs, recs, max_e = quantize_shaped_reference(xs, bits, mode, shape, SC.SEED, keys)
    clipped = 0
    for x, key, q2, rec2 in zip(xs, keys, qs, recs):
        q, rec = quantize_shaped_host(x, bits, mode, shape, SC.SEED, key)
        SC.same(q, rec, q2, rec2, bits, f"W={x.size} ch={channels} {bits} bits {mode} {shape}")
        assert q.shape == x.shape and q.dtype == (np.int16 if bits == 16 else np.int32)
        assert rec["bits"] == bits and rec["dither"] == (1 if mode == "tpdf" else 0)
        if x.size == 0:
            assert rec["q_min"] == 0 and rec["q_max"] == 0 and rec["clipped"] == 0
        clipped += int(rec["clipped"])
    assert clipped > 0                                      # the 1.2 signals clip
    print(f"max |E| = {max_e / 2.0 ** 24:.4f} x 2^24")
    assert max_e < E_BOUND


def test_shaping_changes_the_words_and_nothing_else_does():
    x = SC.signal(2 * SC.CHUNK + 3, 1, 0.3)
    plain = quantize_host(x, 16, "tpdf", SC.SEED, 3)[0]
    got = {s: quantize_shaped_host(x, 16, "tpdf", s, SC.SEED, 3)[0] for s in SC.NAMES}
    for s, q in got.items():
        assert q[0] == plain[0]                             # the first word has an empty history
        assert not np.array_equal(q, plain)
        assert np.array_equal(q, quantize_shaped_host(x, 16, "tpdf", pcm.shape_code(s), SC.SEED, 3)[0])
        assert not np.array_equal(q, quantize_shaped_host(x, 16, "tpdf", s, SC.SEED, 4)[0])
    assert not np.array_equal(got["e3"], got["f9"])


# ---- one chain per channel ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", SC.NAMES)
def test_a_prefix_quantises_as_it_does_in_the_longer_signal(shape):
    for channels in (1, 2):
        x = SC.signal(20011 - (channels - 1), channels, 0.3)
        head = x[:1000 // channels]
        for mode in SC.DITHERS:
            a = quantize_shaped_host(x, 16, mode, shape, SC.SEED, 3)[0]
            assert np.array_equal(a[:1000 // channels], quantize_shaped_host(head, 16, mode, shape, SC.SEED, 3)[0])


@pytest.mark.parametrize("shape", SC.NAMES)
def test_the_right_channel_does_not_reach_the_left(shape):
    x = np.array(SC.signal(8192, 2, 0.3))
    y = x.copy()
    y[:, 1] = SC.signal(4096, 1, 1.2)                       # another right channel, one that clips
    for bits in SC.BITS:
        a = quantize_shaped_host(x, bits, "tpdf", shape, SC.SEED, 3)[0]
        b = quantize_shaped_host(y, bits, "tpdf", shape, SC.SEED, 3)[0]
        assert np.array_equal(a[:, 0], b[:, 0]) and not np.array_equal(a[:, 1], b[:, 1])


@pytest.mark.parametrize("shape", SC.NAMES)
@pytest.mark.parametrize("bits", SC.BITS)
def test_nan_and_infinities_feed_nothing_back(bits, shape):
    S = 1 << (bits - 1)
    for channels in (1, 2):
        x = np.array(SC.signal(2000, channels, 0.3))
        flat = x.reshape(-1)
        flat[[700, 1400]] = np.nan
        flat[[300, 1100]] = [np.inf, -np.inf]
        for mode in SC.DITHERS:
            q, rec = quantize_shaped_host(x, bits, mode, shape, SC.SEED, 9)
            (q2,), (rec2,), max_e = quantize_shaped_reference([x], bits, mode, shape, SC.SEED, [9])
            SC.same(q, rec, q2, rec2, bits, f"{channels} ch {mode}")
            qf = q.reshape(-1)
            assert qf[700] == 0 and qf[1400] == 0 and qf[300] == S - 1 and qf[1100] == -S
            assert rec["nan"] == 2 and rec["clipped"] >= 2
            assert max_e < E_BOUND
            assert rec["q_min"] == -S and rec["q_max"] == S - 1


def test_bad_arguments_raise():
    x = np.zeros(8, dtype=np.float32)
    for bad in ("shaped", "tpdf", 0, 4, True, None, 1.5):
        with pytest.raises(ValueError):
            quantize_shaped_host(x, 16, "tpdf", bad)
        with pytest.raises(ValueError):
            pcm.shape_code(bad)
    for bad in (8, 32, True):
        with pytest.raises(ValueError):
            quantize_shaped_host(x, bad, "tpdf", "f9")
    for bad in ("shaped", 2, None):
        with pytest.raises(ValueError):
            quantize_shaped_host(x, 16, bad, "f9")
    with pytest.raises(ValueError):
        quantize_shaped_host(np.zeros((4, 3), dtype=np.float32), 16, "tpdf", "f9")
    # the C ABI's own check
    import ctypes as C
    from msgpu import _lib as L
    out = np.zeros(16, dtype=np.uint8)
    rec = np.zeros(1, dtype=PCM_DTYPE)
    for bad in (0, 4, -1):
        rc = L.lib().msg_quantize_shaped_host(x.ctypes.data_as(C.c_void_p), 1, 8, 16, 1, bad, 0, 0,
                                              out.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p))
        assert rc == L.MSG_E_VALUE
    assert not out.any()


# ---- the rule table ----------------------------------------------------------------------------
VE, NIE = ValueError, NotImplementedError
RULES = [
    ({"shape": "f9"}, {}, VE),                                      # shape without bits
    ({"bits": 16, "shape": "shaped"}, {}, VE),                      # an unknown shape
    ({"bits": 16, "shape": 4}, {}, VE),
    ({"bits": 16, "shape": True}, {}, VE),
    ({"bits": 20, "shape": "f9"}, {}, VE),
    ({"bits": 16, "dither": "shaped", "shape": "f9"}, {}, VE),      # never a third dither value
    ({"bits": 16, "shape": "f9"}, {"devices": [0, 1]}, NIE),        # refused with bits, as bits alone is
    ({"shape": "f9"}, {"devices": [0, 1]}, VE),
]
STATS = [({"bits": 16, "shape": "f9"}, {"results": "stats"}, VE)]


def ident(case):
    opts, extra, exc = case
    return "-".join(f"{k}={v}" for k, v in {**opts, **extra}.items()).replace(" ", "")


@pytest.mark.parametrize("case", RULES + STATS, ids=ident)
def test_render_batch_rules(case):
    opts, extra, exc = case
    with pytest.raises(exc):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], **{"out_" + k: v for k, v in opts.items()}, **extra)


@pytest.mark.parametrize("case", RULES, ids=ident)
def test_render_variations_rules(case):
    opts, extra, exc = case
    with pytest.raises(exc):
        msgpu.render_variations(dict(msgpu.DEFAULTS), [1000], [1.0], [1.0],
                                **{"export_" + k: v for k, v in opts.items()}, **extra)


def test_delivery_words_the_shape_rules_with_the_prefix():
    from msgpu.export import Delivery
    for prefix in ("out_", "export_"):
        with pytest.raises(VE, match=f"{prefix}shape needs {prefix}bits"):
            Delivery(shape="f9").check(prefix)
        with pytest.raises(VE, match=f"{prefix}shape must be"):
            Delivery(bits=16, shape="lipshitz").check(prefix)
        with pytest.raises(NIE, match=f"{prefix}bits on more than one"):
            Delivery(bits=16, shape="e3").check(prefix, n_devices=2)
    assert Delivery.shape is None and Delivery().shape is None and Delivery(bits=16, shape=None).shape is None
    d = Delivery(bits=16, shape="f9")
    d.check("out_")
    assert d.shape == "f9" and Delivery(bits=16).shape is None     # an instance's own, never the class's
    Delivery(sr=48000, lufs=-23.0, true_peak=-1.0, bits=24, shape=2).check("export_")
    import dataclasses
    names = [f.name for f in dataclasses.fields(Delivery) if f.init]
    # the first ten fields and their positional order stand; the newer rules are fields after them
    assert names[:10] == ["sr", "peak", "lufs", "ceiling", "true_peak", "bits", "dither", "dither_seed", "limiter", "report"]
    assert names[10:] == ["shape", "edges"]
    # and equality, repr and replace see them
    assert d != Delivery(bits=16) and d != Delivery(bits=16, shape="e3") and d == Delivery(bits=16, shape="f9")
    assert "shape='f9'" in repr(d) and dataclasses.replace(d, bits=24).shape == "f9"


# ---- what shaping is for -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def errors():
    """e = q - x S of 16 signals x 65 536 mono words of 0.1 normal (never clips), 16 bits, TPDF,
    seed 7, keys 0 .. 15, for every shape: {shape: (16, 65536) float64}.  Do not write to it."""
    rng = np.random.default_rng(48000)
    x = (0.1 * rng.standard_normal((16, N))).astype(np.float32)
    out = {}
    for shape in SC.NAMES:
        e = np.empty((16, N))
        for key in range(16):
            q, rec = quantize_shaped_host(x[key], 16, "tpdf", shape, 7, key)
            assert rec["clipped"] == 0 and rec["nan"] == 0
            e[key] = q.astype(np.float64) - x[key].astype(np.float64) * 32768.0
        out[shape] = e
    return out


BANDS = ((0, 2000), (2000, 5000), (5000, 10000), (10000, 16000), (16000, 24000))
# band means in dB relative to white TPDF, the prototype's (for the printed comparison)
TABLE = {"e3": (-12.55, -16.69, -4.69, 5.29, 10.44), "lipshitz5": (-16.00, -18.54, -3.12, 0.49, 16.85),
         "f9": (-13.37, -22.03, -4.93, -2.86, 23.14)}


@pytest.mark.parametrize("shape", SC.NAMES)
def test_error_spectrum_is_the_noise_transfer_function(errors, shape):
    """The delivered error is NTF * e with e white of variance 1/4 (rounding 1/12 + TPDF 1/6), so
    its power spectrum is 0.25 |NTF(f)|^2, formed here from the integer table.  Periodograms:
    Hann, 1024 words, no overlap, the mean over all 1024 segments, the rate taken as 48 kHz.
    Bounds: every band mean within 0.25 dB of the prediction (a wrong tap or sign moves a band
    by whole decibels), every bin but DC within 1 dB (the mean of 1024 periodograms has a
    sigma of 1 / 32 = 0.14 dB), the variance within 2 % of 0.25 (1 + sum c^2)."""
    e = errors[shape]
    L = 1024
    w = np.hanning(L + 1)[:L]                                # the periodic Hann window
    seg = e.reshape(-1, L) * w
    assert seg.shape[0] == 1024
    P = (np.abs(np.fft.rfft(seg, axis=1)) ** 2).mean(axis=0) / np.sum(w * w)
    want = 0.25 * SC.ntf_power(shape, L)
    f = np.arange(L // 2 + 1) * 48000.0 / L
    worst_band = 0.0
    for (lo, hi), tab in zip(BANDS, TABLE[shape]):
        m = (f >= lo) & (f < hi) if hi < 24000 else (f >= lo) & (f <= hi)
        got_db = 10 * np.log10(P[m].mean() / 0.25)
        want_db = 10 * np.log10(want[m].mean() / 0.25)
        print(f"{shape} {lo:5d}-{hi:5d} Hz: measured {got_db:+7.2f} dB, predicted {want_db:+7.2f} dB, table {tab:+7.2f} dB")
        worst_band = max(worst_band, abs(got_db - want_db))
        assert abs(got_db - want_db) <= 0.25
    bins = 10 * np.log10(P[1:] / want[1:])
    var, var_want = e.var(), 0.25 * (1.0 + np.sum((np.array(pcm.SHAPES[shape][1]) / 65536.0) ** 2))
    print(f"{shape}: worst band {worst_band:.3f} dB, bins [{bins.min():+.2f}, {bins.max():+.2f}] dB, "
          f"variance {var:.4f} against {var_want:.4f}")
    assert np.all(np.abs(bins) <= 1.0)
    assert abs(var / var_want - 1.0) <= 0.02


@pytest.mark.parametrize("shape", SC.NAMES)
@pytest.mark.parametrize("bits", SC.BITS)
def test_shaped_error_is_independent_of_the_signal(bits, shape):
    """Constant inputs (100 + f) / S: the shaped total error still has zero mean whatever f
    is, and a smaller one than white noise would give: NTF(1) = 1 - sum c_k is small, so the
    mean of 65 536 errors has a sigma well under TPDF's 0.002.  Bound 0.004."""
    S = float(1 << (bits - 1))
    worst = 0.0
    for f in (0.0, 0.125, 0.25, 0.5, 0.75, 0.9):
        x = np.full(N, (100 + f) / S, dtype=np.float32)
        q, _ = quantize_shaped_host(x, bits, "tpdf", shape, 7, 3)
        e = q.astype(np.float64) - x.astype(np.float64) * S
        worst = max(worst, abs(e.mean()))
        assert abs(e.mean()) <= 0.004, (f, e.mean())
    print(f"{bits} bits {shape}: worst |mean error| {worst:.2e}")


@pytest.mark.parametrize("shape", SC.NAMES)
def test_tone_under_one_step_survives_shaping(shape):
    n = np.arange(N)
    ref = np.sin(2 * np.pi * n * 1000 / 48000)
    x = (0.4 / 32768 * ref).astype(np.float32)
    q, _ = quantize_shaped_host(x, 16, "tpdf", shape, 7, 3)
    amp = 2 * float(np.mean(q * ref))
    print(f"{shape}: 0.4 LSB tone, recovered amplitude {amp:.4f} LSB")
    assert abs(amp - 0.4) <= 0.02


# ---- the header under the sanitizers -----------------------------------------------------------------
@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
def test_host_loop_under_asan_ubsan(tmp_path):
    """csrc/pcm_shape.h in a stand-alone program (tests/pcm_shape_check.cpp) under ASan + UBSan:
    the host loop over exactly-sized heap blocks, input and output, at the edge lengths (a
    byte written past W bits / 8 is an ASan report), NaN and infinities in mid-signal (a NaN
    or an infinity converted to an integer is a UBSan report), the bound on |E|."""
    import subprocess
    exe = str(tmp_path / "pcm_shape_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(REPO, "audio-suite_amd", "csrc"),
                    "-o", exe, os.path.join(REPO, "tests", "pcm_shape_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "bad 0" in out, out[-4000:]


def test_python_constants_match_the_kernels():
    src = open(os.path.join(REPO, "audio-suite_amd", "csrc", "pcm_shape.h")).read()
    table = re.search(r"PCM_SHAPE_H\[3\]\[PCM_SHAPE_KMAX\] = \{(.*?)\};", src, flags=re.S).group(1)
    rows = [[int(v) for v in re.findall(r"-?\d+", row)] for row in re.findall(r"\{([^{}]*)\}", table)]
    taps = {"e3": (1.623, -0.982, 0.109), "lipshitz5": (2.033, -2.165, 1.959, -1.590, 0.6149),
            "f9": (2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847)}
    assert len(rows) == 3 and all(len(r) == 9 for r in rows)
    for (name, (code, h)), row in zip(pcm.SHAPES.items(), rows):
        K = len(h)
        assert tuple(row[:K]) == h and not any(row[K:])
        assert h == tuple(-int(np.floor(abs(c) * 65536 + 0.5)) * (1 if c > 0 else -1) for c in taps[name])
        assert code == int(re.search(rf"PCM_SHAPE_{name.upper()} = (\d)", src).group(1))
    assert pcm.SHAPE_CHUNK == int(re.search(r"constexpr int PCM_SHAPE_CHUNK = (\d+);", src).group(1))
    hdr = open(os.path.join(REPO, "include", "msgpu.h")).read()
    enum = re.search(r"enum msg_shape \{(.*?)\}", hdr, flags=re.S).group(1)
    vals = {k: int(v) for k, v in re.findall(r"MSG_SHAPE_([A-Z0-9]+)\s*=\s*(\d+)", enum)}
    assert vals == {"E3": 1, "LIPSHITZ5": 2, "F9": 3} == {k.upper(): c for k, (c, _) in pcm.SHAPES.items()}
    assert all(abs(sum(abs(c) for c in taps[s]) - v) < 0.005 for s, v in (("e3", 2.71), ("lipshitz5", 8.36), ("f9", 21.39)))
