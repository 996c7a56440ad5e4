"""BS.1770-4 integrated loudness on the host: msg_loudness_host (csrc/loudness.h, a
sequential float64 loop) against msgpu.loudness.loudness_reference (the definition
in float64 NumPy, scipy.signal.lfilter where scipy imports).  Both run float64 on
identical float32 samples and differ by rounding order only, about 1e-9 relative even
through the high-pass's noise gain; the bar of 1e-6 LU (2.3e-7 relative) leaves two
orders of margin and a float32 filter (1e-4 LU or worse) does not pass it."""
import math

import numpy as np
import pytest

import loudness_cases as LC
from msgpu.loudness import kweight, loudness_host, loudness_reference


def test_coefficients_48k():
    (b1, a1), (b2, a2) = kweight(48000)
    assert np.allclose(b1, [1.53512485958697, -2.69169618940638, 1.19839281085285], rtol=0, atol=1e-9)
    assert np.allclose(a1, [1.0, -1.69065929318241, 0.73248077421585], rtol=0, atol=1e-9)
    assert np.array_equal(b2, [1.0, -2.0, 1.0])
    assert np.allclose(a2, [1.0, -1.99004745483398, 0.99007225036621], rtol=0, atol=1e-9)


@pytest.mark.parametrize("sr", LC.RATES)
@pytest.mark.parametrize("dbfs", [-23.0, -33.0])
def test_sine_anchors(sr, dbfs):
    """A 1 kHz stereo sine at dbfs peak per channel reads dbfs LUFS within the standard's
    conformance window of 0.1 LU."""
    x, ref = LC.case(f"sine:{dbfs}", sr)
    got = float(loudness_host(x, sr)["lufs"])
    print(f"sine {dbfs} dBFS at {sr} Hz: host {got:.4f} reference {ref:.4f}")
    assert abs(got - dbfs) <= 0.1
    assert abs(ref - dbfs) <= 0.1
    assert LC.close_lu(got, ref)


@pytest.mark.parametrize("name,sr", [(n, sr) for n, rates in LC.CPU_CASES for sr in rates])
def test_gates_against_reference(name, sr):
    x, ref = LC.case(name, sr)
    rec = loudness_host(x, sr)
    print(f"{name} at {sr} Hz: host {rec['lufs']:.9f} reference {ref:.9f} diff {rec['lufs'] - ref:.2e} "
          f"kept {rec['n_kept']}/{rec['n_blocks']}")
    assert LC.close_lu(float(rec["lufs"]), ref)
    assert rec["n_kept"] < rec["n_blocks"]              # a gate dropped something
    assert rec["peak"] == float(np.max(np.abs(x)))
    assert rec["gain"] == 0.0


@pytest.mark.parametrize("sr", (44100, 48000))
def test_flanks_leave_the_value(sr):
    """The absolute gate drops the -72 dBFS flanks and the blocks that straddle them fall
    to the relative gate, so the kept blocks are the unflanked signal's, ten hops later,
    over the same samples.  The filter reaches them in another state, a transient that
    has decayed by e^-250 a second on (the high-pass's time constant is 4 ms)."""
    a = float(loudness_host(LC.case("sequence", sr)[0], sr)["lufs"])
    b = float(loudness_host(LC.case("flanked", sr)[0], sr)["lufs"])
    print(f"{sr} Hz: unflanked {a:.9f} flanked {b:.9f}")
    assert abs(a - b) <= LC.TOL
    assert abs(LC.case("sequence", sr)[1] - LC.case("flanked", sr)[1]) <= LC.TOL


@pytest.mark.parametrize("n,blocks", LC.lengths_48k())
def test_lengths_48k(n, blocks):
    x = np.random.default_rng(n).standard_normal((n, 2)).astype(np.float32) * 0.1
    rec = loudness_host(x, 48000)
    ref = loudness_reference(x, 48000)
    assert rec["n_blocks"] == blocks
    if blocks == 0:
        assert rec["lufs"] == -math.inf and ref == -math.inf and rec["mean_sq"] == 0.0 and rec["n_kept"] == 0
    else:
        assert LC.close_lu(float(rec["lufs"]), ref)
    mono = loudness_host(x[:, 0], 48000)
    assert mono["n_blocks"] == blocks and LC.close_lu(float(mono["lufs"]), loudness_reference(x[:, 0], 48000))


def test_silence_is_minus_infinity():
    x = np.zeros((48000, 2), dtype=np.float32)
    rec = loudness_host(x, 48000)
    assert rec["lufs"] == -math.inf and rec["mean_sq"] == 0.0 and rec["n_blocks"] == 7 and rec["n_kept"] == 0
    assert loudness_reference(x, 48000) == -math.inf


def test_bad_rate_raises():
    x = np.zeros(1000, dtype=np.float32)
    with pytest.raises(ValueError):
        loudness_host(x, 11025)
    with pytest.raises(ValueError):
        loudness_reference(x, 11025)
    with pytest.raises(ValueError):
        kweight(11025)


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
def test_tables_and_host_loop_under_asan_ubsan(tmp_path):
    """csrc/loudness.h in a stand-alone program (tests/loudness_check.cpp) under ASan +
    UBSan: every power of the table against the recurrence it stands for, the tiles of
    short and ragged lengths, the host loop at the edge lengths."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "loudness_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(repo, "audio-suite_amd", "csrc"),
                    "-o", exe, os.path.join(repo, "tests", "loudness_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "bad 0" in out, out[-4000:]


def test_python_tile_constants_match_the_kernels():
    import os
    import re
    from msgpu.loudness import CHUNK, SR_MIN, TILE
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(repo, "audio-suite_amd", "csrc", "loudness.h")).read()
    val = lambda name: int(re.search(r"constexpr int(?:64_t)? %s = (\d+);" % name, src).group(1))
    assert CHUNK == val("LD_C") and TILE == val("LD_T") * val("LD_C") and SR_MIN == val("LD_SR_MIN")
