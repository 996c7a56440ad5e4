"""Device loudness range and maximum momentary / short-term loudness (msg_loudness_range,
csrc/kernels_lrange.h) against the float64 reference (msgpu.lrange.lrange_reference) at
1e-6 LU (2e-6 on lra) and against the library's plain C++ on the device's own hop sums
(msg_lrange_hops_host) to the bit; the delivery reports on top of it.  Signals, the input
rule and the bars: tests/lrange_cases.py."""
import csv
import math
import os

import numpy as np
import pytest

import lrange_cases as RC
import msgpu
from msgpu.loudness import records as loud_records
from msgpu.export import REPORT_DTYPE
from msgpu.lrange import curves_reference, lrange_hops_host, records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from msgpu.engine import default_engine
    return default_engine(0)


def pack(signals, channels, gap=3):
    """The signals back to back with `gap` frames of NaN around and between them (an odd gap:
    mono signals start at odd floats): (buffer, offsets, lens)."""
    nan = np.full((gap, 2) if channels == 2 else gap, np.nan, dtype=np.float32)
    offs, lens, parts, at = [], [], [nan], gap
    for s in signals:
        offs.append(at)
        lens.append(len(s))
        parts += [np.asarray(s, dtype=np.float32), nan]
        at += len(s) + gap
    return np.concatenate(parts), np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)


def measure(eng, signals, channels, sr):
    """One msg_loudness_range call over the signals between NaN gaps: (range records, loudness
    records, each signal's exported hop sums, the device buffer, offsets, lens), on the host."""
    buf, offs, lens = pack(signals, channels)
    x = eng.torch.from_numpy(buf).cuda()
    loud, rng, hops, hop_off = eng.loudness_range(x, offs, lens, channels, sr, hops=True)
    H = hops.cpu().numpy()
    per = [H[int(o):int(o) + int(n) // (sr // 10)] for o, n in zip(hop_off, lens)]
    return records(rng), loud_records(loud), per, x, offs, lens


def check_against_hops_host(r, H, hop, what):
    """The device record against the library's plain C++ on the device's exported hop sums: the
    mean squares and the counts as bits, the levels within 1e-12 LU (two log10 implementations)."""
    h = lrange_hops_host(H, hop)
    for k in RC.ZS + RC.COUNTS:
        assert RC.same_bits(r[k], h[k]), (what, k, r[k], h[k])
    for k in RC.LEVELS + ("lra", "gate"):
        assert RC.close(float(r[k]), float(h[k]), 1e-12), (what, k, float(r[k]), float(h[k]))


ACCURACY = ["tech4k:10", "tech4k:20", "tech4k:15", "noise48k", "noise384k"]


@pytest.mark.parametrize("name", ACCURACY)
def test_accuracy(eng, name):
    x, sr, ref = RC.case(name)
    got, loud, H, dx, offs, lens = measure(eng, [x], 2, sr)
    RC.check_record(got[0], ref, name)
    check_against_hops_host(got[0], H[0], sr // 10, name)
    if name.startswith("tech4k") and name != "tech4k:15":
        assert abs(float(got[0]["lra"]) - RC.TECH_3342[name.split(":")[1]][1]) <= 1.0
    # the loudness records: msg_loudness's bytes
    assert RC.same_bits(loud, loud_records(eng.loudness(dx, offs, lens, 2, sr)))


def test_public_functions(eng):
    x, sr, ref = RC.case("tech4k:20")
    d = msgpu.loudness_range(np.asarray(x), sr)
    assert all(isinstance(d[k], float) for k in ("lufs", "lra", "lo", "hi", "max_momentary", "max_short"))
    assert RC.close(d["lra"], ref["lra"], RC.TOL_LRA) and RC.close(d["max_short"], ref["max_short"], RC.TOL)
    assert RC.close(d["lufs"], msgpu.loudness(np.asarray(x), sr), 0.0)
    t = eng.torch.from_numpy(np.array(x)).cuda()
    dd = msgpu.loudness_range(t, sr)
    assert all(v.is_cuda and tuple(v.shape) == (1,) for v in dd.values())
    assert float(dd["lra"].cpu()[0]) == d["lra"] and float(dd["lufs"].cpu()[0]) == d["lufs"]
    m, s = msgpu.loudness_curves(np.asarray(x), sr)
    rm, rs = curves_reference(x, sr)
    assert m.shape == rm.shape and s.shape == rs.shape == (ref["n_short"],)
    assert np.max(np.abs(m - rm)) <= RC.TOL and np.max(np.abs(s - rs)) <= RC.TOL
    assert RC.close(float(s.max()), d["max_short"], 1e-12) and RC.close(float(m.max()), d["max_momentary"], 1e-12)
    tm, ts = msgpu.loudness_curves(t, sr)
    assert tm.is_cuda and np.max(np.abs(ts.cpu().numpy() - s)) <= 1e-12
    with pytest.raises(ValueError):
        msgpu.loudness_range(t, 11025)


@pytest.mark.parametrize("channels", [1, 2])
def test_lengths_4k(eng, channels):
    """Either side of one short-term window (29, 30, 31 hops), a trailing incomplete hop, fewer
    hops than a momentary block, and no frame at all: one ragged call."""
    cases = [RC.case(f"len4k:{h}:{e}:{channels}") for h, e in RC.LENGTHS_4K]
    got, loud, H, dx, offs, lens = measure(eng, [c[0] for c in cases], channels, 4000)
    for r, l, h, (x, sr, ref), (hops, extra) in zip(got, loud, H, cases, RC.LENGTHS_4K):
        what = f"{hops} hops + {extra} ch={channels}"
        RC.check_record(r, ref, what)
        check_against_hops_host(r, h, 400, what)
        assert h.size == hops and r["n_short"] == max(0, hops - 29) and r["n_momentary"] == max(0, hops - 3)
        if hops < 30:
            assert r["lra"] == 0.0 and r["lo"] == r["hi"] == r["max_short"] == -math.inf and r["gate"] == -math.inf
            assert r["z_lo"] == r["z_hi"] == r["z_max_s"] == 0.0
        if hops < 4:
            assert r["max_momentary"] == -math.inf and r["z_max_m"] == 0.0
    assert RC.same_bits(loud, loud_records(eng.loudness(dx, offs, lens, channels, 4000)))


@pytest.mark.parametrize("name,kept", [("long4k:2", None), ("long4k:1", None), ("kept257", 257)])
def test_more_windows_than_threads(eng, name, kept):
    x, sr, ref = RC.case(name)
    channels = 1 if x.ndim == 1 else 2
    got, loud, H, *_ = measure(eng, [x], channels, sr)
    RC.check_record(got[0], ref, name)
    check_against_hops_host(got[0], H[0], sr // 10, name)
    assert got[0]["n_short"] > 256
    if kept is not None:
        assert got[0]["n_kept"] == kept and got[0]["n_abs"] > kept
    else:
        assert got[0]["n_short"] == 1171 and got[0]["n_kept"] < got[0]["n_abs"]


def test_ragged_batch(eng):
    """Every signal above of one rate in one call between NaN gaps, an empty one first and one
    last: each record's bytes are the signal's alone, and the call repeated gives the same bytes."""
    names = ["tech4k:10", "long4k:2", "len4k:30:399:2", "kept257", "len4k:3:0:2", "tech4k:15", "len4k:31:0:2"]
    empty = np.zeros((0, 2), dtype=np.float32)
    sig = [empty] + [RC.case(n)[0] for n in names] + [empty]
    got, loud, H, dx, offs, lens = measure(eng, sig, 2, 4000)
    for r, n in zip(got[1:-1], names):
        RC.check_record(r, RC.case(n)[2], "ragged " + n)
        assert all(math.isfinite(float(r[k])) for k in RC.ZS)
    for r in (got[0], got[-1]):
        assert r["n_short"] == 0 and r["n_momentary"] == 0 and r["lra"] == 0.0 and r["max_momentary"] == -math.inf
    l2, r2 = eng.loudness_range(dx, offs, lens, 2, 4000)          # no hop sums taken: the same records
    assert RC.same_bits(got, records(r2)) and RC.same_bits(loud, loud_records(l2))
    assert RC.same_bits(loud, loud_records(eng.loudness(dx, offs, lens, 2, 4000)))
    for i, s in enumerate(sig):
        a_rng, a_loud, a_H, *_ = measure(eng, [s], 2, 4000)
        assert RC.same_bits(a_rng, got[i:i + 1]), i
        assert RC.same_bits(a_loud, loud[i:i + 1]), i
        assert RC.same_bits(a_H[0], H[i]), i


# ---- delivery reports ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(irs):
    return msgpu.config_params("C2", irs=irs, out_dur_s=0.75)


def check_report_row(row, y, sr):
    """A report row against the meters run on the audio it describes."""
    y = np.ascontiguousarray(y)
    d = msgpu.loudness_range(y, sr)
    for k in ("lufs", "lra", "lo", "hi", "max_momentary", "max_short"):
        assert RC.close(float(row[k]), d[k], 0.0), (k, float(row[k]), d[k])
    assert float(row["peak"]) == float(np.max(np.abs(y)))
    assert float(row["true_peak"]) == msgpu.true_peak(y, sr)
    assert RC.close(float(row["dbtp"]), 20.0 * math.log10(float(row["true_peak"])), 1e-9)
    assert int(row["frames"]) == y.shape[0] and int(row["rate"]) == sr


def test_render_batch_report(c2, irs):
    ps = [c2, msgpu.config_params("C2", seed=1001, irs=irs, out_dur_s=0.75)]
    sr = int(c2["base_sr"])
    rep = []
    out = msgpu.render_batch(ps, out_lufs=-23.0, out_true_peak=-1.0, out_report=rep)
    assert len(rep) == 2 and all(r.dtype == REPORT_DTYPE for r in rep)
    for row, y in zip(rep, out):
        check_report_row(row, y, sr)
        print(f"report: {float(row['lufs']):.9f} LUFS, lra {float(row['lra']):.6f}, {float(row['dbtp']):.6f} dBTP")
        bound = float(row["dbtp"]) >= -1.0 - 1e-3            # the ceiling bound: the render lies under the target
        assert abs(float(row["lufs"]) + 23.0) <= 1e-5 or (bound and float(row["lufs"]) < -23.0)
        assert float(row["dbtp"]) <= -1.0 + 1e-6
    plain = msgpu.render_batch(ps, out_lufs=-23.0, out_true_peak=-1.0)
    assert all(np.array_equal(a, b) for a, b in zip(out, plain))        # reporting changes no sample
    with pytest.raises(ValueError):
        msgpu.render_batch(ps, results="stats", out_report=[])
    with pytest.raises(NotImplementedError):
        msgpu.render_batch(ps, devices=[0, 1], out_report=[])


def test_render_variations_report_csv(c2, tmp_path):
    rep = []
    got = msgpu.render_variations(c2, [1000, 1001], [c2["time_unfold"]], [c2["partial_stretch"]], folder=str(tmp_path),
                                  export_lufs=-23.0, export_true_peak=-1.0, export_report=rep)
    assert len(rep) == len(got) == 2
    with open(os.path.join(str(tmp_path), "loudness_report.csv"), newline="") as fh:
        rows = list(csv.DictReader(fh))
    assert [r["file"] for r in rows] == [name for name, _, _ in got]
    for line, row, (name, y, rate) in zip(rows, rep, got):
        check_report_row(row, y, rate)
        assert float(line["lufs"]) == float(row["lufs"]) and float(line["lra"]) == float(row["lra"])
        assert float(line["dbtp"]) == float(row["dbtp"]) and int(line["frames"]) == y.shape[0]
    quiet = tmp_path / "plain"
    quiet.mkdir()
    msgpu.render_variations(c2, [1000], [c2["time_unfold"]], [c2["partial_stretch"]], folder=str(quiet))
    assert not os.path.exists(os.path.join(str(quiet), "loudness_report.csv"))     # no report asked: nothing written
