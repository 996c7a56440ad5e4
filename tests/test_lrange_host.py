"""Loudness range and maximum momentary / short-term loudness on the host:
msg_loudness_range_host and msg_lrange_hops_host (csrc/lrange.h, plain C++) against
msgpu.lrange.lrange_reference / hops_reference (the definition in float64 NumPy), the EBU
Tech 3342 tone sequences, and the delivery rule table of ``report``.  Signals, the input
rule and the bars: tests/lrange_cases.py."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import lrange_cases as RC
from msgpu import _lib as L
from msgpu.export import REPORT_DTYPE, Delivery, write_report_csv
from msgpu.loudness import loudness_host
from msgpu.lrange import (LRANGE_DTYPE, curves_reference, hop_sums_reference, hops_reference, lrange_hops_host,
                          lrange_host, lrange_reference)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_layout():
    assert LRANGE_DTYPE.itemsize == 96 == L.lib().msg_sizeof(8)
    assert LRANGE_DTYPE.names[:3] == ("lra", "lo", "hi") and LRANGE_DTYPE.names[-1] == "n_kept"


@pytest.mark.parametrize("which", sorted(RC.TECH_3342))
def test_tech_3342_sequences(which):
    """The four tone sequences of EBU Tech 3342 at 48 kHz: host and reference each within 1 LU
    of the expected range, and within the bars of each other."""
    x, sr, ref = RC.case(f"tech48k:{which}")
    want = RC.TECH_3342[which][1]
    rec, loud = lrange_host(x, sr, loudness=True)
    RC.check_record(rec, ref, f"Tech 3342 {want} LU")
    assert abs(ref["lra"] - want) <= 1.0 and abs(float(rec["lra"]) - want) <= 1.0
    assert RC.same_bits(loud, loudness_host(x, sr))              # the loudness record: msg_loudness_host's bytes
    if which == "15":
        assert rec["n_kept"] < rec["n_abs"] == rec["n_short"]    # the relative gate at work


def hop_sums(kind, hops, seed=0):
    rng = np.random.default_rng(1000 + hops + seed)
    hop = 4800
    if kind == "random":          # seven decades around the gates
        return hop * 10.0 ** rng.uniform(-9.0, -1.0, hops), hop
    if kind == "equal":
        return np.full(hops, 0.0625 * hop), hop
    if kind == "silent":
        return np.zeros(hops), hop
    if kind == "ties":            # runs of equal windows straddling both ranks
        return np.where((np.arange(hops) // 45) % 2 == 1, 0.25 * hop, 0.002 * hop).astype(np.float64), hop
    raise KeyError(kind)


def check_hops(H, hop, what):
    ref = hops_reference(H, hop)
    if ref["margin"] < RC.MARGIN:                      # a level at a gate: draw again, never widen
        return None
    rec = lrange_hops_host(H, hop)
    RC.check_record(rec, ref, what)
    for k in RC.ZS:
        assert RC.same_bits(rec[k], np.float64(ref[k])), (what, k, float(rec[k]), ref[k])
    return rec


@pytest.mark.parametrize("hops", [0, 3, 4, 29, 30, 31, 39, 40, 41, 1200])
def test_hops_host_against_numpy(hops):
    checked = 0
    for seed in range(8):
        H, hop = hop_sums("random", hops, seed)
        checked += check_hops(H, hop, f"random {hops} hops seed {seed}") is not None
    assert checked >= 4
    rec = check_hops(*hop_sums("equal", hops), f"equal {hops}")
    assert rec["lra"] == 0.0 and rec["n_kept"] == rec["n_short"] == max(0, hops - 29)
    rec = check_hops(*hop_sums("silent", hops), f"silent {hops}")
    assert rec["n_abs"] == rec["n_kept"] == 0 and rec["lra"] == 0.0 and rec["gate"] == -math.inf
    assert rec["lo"] == rec["hi"] == rec["max_short"] == rec["max_momentary"] == -math.inf
    rec = check_hops(*hop_sums("ties", hops), f"ties {hops}")
    if hops == 1200:
        assert rec["n_kept"] > 256 and rec["z_lo"] < rec["z_hi"]


def test_ties_straddle_the_ranks():
    """60 equal windows, 29 in transition, 60 equal windows (integer hop sums: equal windows are
    equal to the bit): both ranks, 15 and 141 of 149, fall inside a run of ties and give its value."""
    hop, a, b = 4800, 48.0, 1200.0
    H = np.concatenate([np.full(89, a), np.full(89, b)])
    rec = check_hops(H, hop, "two runs of ties")
    assert rec["n_kept"] == rec["n_short"] == 149
    assert float(rec["z_lo"]) == a / hop and float(rec["z_hi"]) == b / hop
    assert abs(float(rec["lra"]) - 10.0 * math.log10(b / a)) <= 1e-12


@pytest.mark.parametrize("c2", [1, 2])
def test_one_and_two_kept_windows(c2):
    hop = 400
    H = np.concatenate([np.full(29, 0.01 * hop), np.full(c2, 0.04 * hop)])
    rec = check_hops(H, hop, f"c2 = {c2}")
    assert rec["n_kept"] == c2 == rec["n_short"]
    assert RC.same_bits(rec["z_lo"], rec["z_hi"]) == (c2 == 1)         # ranks 0 and 0, then 0 and 1
    assert (rec["lra"] == 0.0) == (c2 == 1)


def test_curves_of_a_stepped_signal():
    x, sr, ref = RC.case("tech4k:15")
    m, s = curves_reference(x, sr)
    H = hop_sums_reference(x, sr)
    assert m.shape == (ref["n_momentary"],) and s.shape == (ref["n_short"],)
    rec = lrange_host(x, sr)
    assert RC.close(float(m.max()), float(rec["max_momentary"]), RC.TOL)
    assert RC.close(float(s.max()), float(rec["max_short"]), RC.TOL)
    # each segment's plateau: a window wholly inside a 6 s segment reads the tone's level
    for seg, dbfs in enumerate(RC.TECH_3342["15"][0]):
        assert abs(s[seg * 60 + 15] - (dbfs - 0.691 + 0.0)) <= 0.5, (seg, s[seg * 60 + 15])
    assert H.size == x.shape[0] // (sr // 10)


@pytest.mark.parametrize("hops,extra", RC.LENGTHS_4K)
def test_lengths_4k(hops, extra):
    for ch in (1, 2):
        x, sr, ref = RC.case(f"len4k:{hops}:{extra}:{ch}")
        RC.check_record(lrange_host(x, sr), ref, f"{hops} hops + {extra} ch={ch}")


def test_bad_arguments_raise():
    x = np.zeros(1000, dtype=np.float32)
    with pytest.raises(ValueError):
        lrange_host(x, 11025)
    with pytest.raises(ValueError):
        lrange_reference(x, 11025)
    with pytest.raises(ValueError):
        lrange_host(np.zeros((10, 3), dtype=np.float32), 48000)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_definition_under_asan_ubsan(tmp_path):
    """csrc/lrange.h in a stand-alone program (tests/lrange_check.cpp) under ASan + UBSan."""
    exe = str(tmp_path / "lrange_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(REPO, "audio-suite_amd", "csrc"),
                    "-o", exe, os.path.join(REPO, "tests", "lrange_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "bad 0" in out, out[-4000:]


# ---- the delivery rule table of ``report`` ----------------------------------------------------
def test_report_rules():
    Delivery().check("out_")                                             # nothing asked: nothing checked
    Delivery(report=[]).check("out_", rates=[48000])
    Delivery(report=[]).check("out_", "device", rates=[44100, 96000])
    Delivery(sr=48000, report=[]).check("out_", rates=[11025])           # metered at the delivered rate
    with pytest.raises(ValueError):
        Delivery(report=[]).check("out_", "stats", rates=[48000])
    with pytest.raises(ValueError):
        Delivery(report=()).check("out_", rates=[48000])                 # a list is what gets the rows
    with pytest.raises(ValueError):
        Delivery(report=[]).check("out_", rates=[48000, 11025])          # a rate the loudness meter refuses
    with pytest.raises(ValueError):
        Delivery(sr=22055, report=[]).check("export_", rates=[48000])
    with pytest.raises(NotImplementedError):
        Delivery(report=[]).check("export_", n_devices=2, rates=[48000])
    with pytest.raises(NotImplementedError):
        Delivery(report=[]).one_device("out_", 2, companions=True)
    Delivery().one_device("out_", 2, companions=True)
    assert Delivery.__dataclass_fields__["report"].default is None
    # the tenth positional field, where its callers have it; the rules after it are fields behind it
    assert [f for f in Delivery.__dataclass_fields__ if not f.startswith("_")][9:] == ["report", "shape", "edges"]


def test_report_csv_round_trip(tmp_path):
    import csv
    rows = np.zeros(2, dtype=REPORT_DTYPE)
    rows["lufs"], rows["lra"], rows["lo"], rows["frames"], rows["rate"] = [-23.0, -math.inf], [3.25, 0.0], \
        [-30.1, -math.inf], [480000, 0], 48000
    path = str(tmp_path / "loudness_report.csv")
    write_report_csv(path, ["a.wav", "b.wav"], rows)
    with open(path, newline="") as fh:
        got = list(csv.DictReader(fh))
    assert [g["file"] for g in got] == ["a.wav", "b.wav"] and list(got[0]) == ["file"] + list(REPORT_DTYPE.names)
    assert float(got[0]["lufs"]) == -23.0 and float(got[1]["lufs"]) == -math.inf and int(got[0]["frames"]) == 480000
