"""The stereo rule without a device: the matrices of msgpu/stereo.py, the library's host loops
(msg_stereo_host to the bit against exact arithmetic, msg_stereo_meter_host against math.fsum on the
exact float64 products; csrc/image.h), the refusals, and the delivery rule (msgpu/export.py).  The
meter's tolerances and what the device tests share are in tests/stereo_cases.py."""
import ctypes as C
import dataclasses
import inspect
import math
from fractions import Fraction

import numpy as np
import pytest

import msgpu
from msgpu import _lib as L
from msgpu.stereo import (STEREO_DTYPE, STEREO_ROW_DTYPE, Stereo, derive, meter_reference, stereo_host,
                          stereo_meter_host)

from stereo_cases import bits, check_meter, samples, separated


# ---- the matrices -----------------------------------------------------------------------------------
def test_matrix_at():
    m, fold = Stereo().matrix_at()
    assert m.dtype == np.float32 and fold.dtype == np.float32 and m.shape == (2, 2) and fold.shape == (2,)
    assert np.array_equal(m, np.eye(2)) and np.array_equal(fold, [0.5, 0.5])
    m, fold = Stereo(width=0).matrix_at()
    assert np.array_equal(m[0], m[1]) and np.array_equal(m, [[0.5, 0.5], [0.5, 0.5]]) and np.array_equal(fold, [0.5, 0.5])
    m, fold = Stereo(width=2).matrix_at()
    assert np.array_equal(m, [[1.5, -0.5], [-0.5, 1.5]]) and np.array_equal(fold, [0.5, 0.5])   # the mid is kept
    assert np.array_equal(Stereo(swap=True).matrix_at()[0], [[0, 1], [1, 0]])
    assert np.array_equal(Stereo(invert="left").matrix_at()[0], [[-1, 0], [0, 1]])
    assert np.array_equal(Stereo(invert="right").matrix_at()[0], [[1, 0], [0, -1]])
    assert np.array_equal(Stereo(invert="right").matrix_at()[1], [0.5, -0.5])
    assert np.array_equal(Stereo(invert="auto").matrix_at()[0], np.eye(2))                      # the device's flip
    g = np.float32(10.0 ** (-6.0 / 20.0))
    assert np.array_equal(Stereo(balance_db=6).matrix_at()[0], [[g, 0], [0, 1]])                # positive: left down
    assert np.array_equal(Stereo(balance_db=-6).matrix_at()[0], [[1, 0], [0, g]])
    raw = [[0.25, -1.5], [3.0, 0.125]]
    m, fold = Stereo(matrix=raw).matrix_at()
    assert np.array_equal(m, raw) and np.array_equal(fold, [1.625, -0.6875])
    # a composition against the float64 product M = G W P D, rounded once
    s = Stereo(width=1.3, balance_db=-2.5, swap=True, invert="left")
    G = np.diag([1.0, 10.0 ** (-2.5 / 20.0)])
    W = np.array([[1.15, -0.15], [-0.15, 1.15]])
    P = np.array([[0.0, 1.0], [1.0, 0.0]])
    D = np.diag([-1.0, 1.0])
    M = G @ W @ P @ D
    m, fold = s.matrix_at()
    assert np.allclose(s.matrix64(), M, rtol=0, atol=1e-15)
    assert np.array_equal(m, s.matrix64().astype(np.float32))
    assert np.array_equal(fold, (0.5 * (s.matrix64()[0] + s.matrix64()[1])).astype(np.float32))
    assert np.max(np.abs(m - M)) <= 2.0 ** -24 * 1.2
    # D met the input first: L' = a R + b (-L); had it come last, L' = -(a R + b L)
    assert np.array_equal(m[0], np.array([0.15, 1.15]).astype(np.float32)) and m[1, 0] < 0 and m[1, 1] < 0


@pytest.mark.parametrize("kw, words", [
    (dict(width=-0.1), "width"), (dict(width=4.5), "width"), (dict(width="wide"), "width"), (dict(width=True), "width"),
    (dict(width=float("nan")), "width"), (dict(balance_db=float("inf")), "balance_db"), (dict(balance_db="l"), "balance_db"),
    (dict(swap=1), "swap"), (dict(invert="both"), "invert"), (dict(invert=True), "invert"), (dict(channels=3), "channels"),
    (dict(channels=0), "channels"), (dict(channels=True), "channels"), (dict(matrix=[1, 0, 0, 1]), "matrix"),
    (dict(matrix=[[1, 0], [0, float("nan")]]), "matrix"), (dict(matrix=[[1e39, 0], [0, 1]]), "matrix"),
    (dict(matrix="m"), "matrix"), (dict(matrix=np.eye(2), width=2), "instead of"),
    (dict(matrix=np.eye(2), invert="auto"), "instead of"), (dict(matrix=np.eye(2), swap=True), "instead of"),
    (dict(meter=()), "meter"), (dict(meter={}), "meter")])
def test_check_refuses(kw, words):
    with pytest.raises(ValueError, match=words):
        Stereo(**kw).check()
    with pytest.raises(ValueError, match=words):
        Stereo(**kw).matrix_at()


def test_check_accepts():
    for s in (Stereo(), Stereo(width=0), Stereo(width=4), Stereo(balance_db=-90), Stereo(invert="auto", channels=1, meter=[]),
              Stereo(matrix=np.eye(2), channels=1, meter=[])):
        assert s.check() is s
    assert Stereo(meter=[]).metering() and Stereo(invert="auto").metering() and not Stereo(width=0, channels=1).metering()
    assert Stereo(width=2) == Stereo(width=2) and Stereo(width=2) != Stereo(width=2, channels=1)


# ---- msg_stereo_host --------------------------------------------------------------------------------
def round32(v):
    """A Fraction rounded to the nearest float32, ties to even (the values here stay finite)."""
    if v == 0:
        return np.float32(0.0)
    f = np.float32(float(v))                     # float(Fraction) is correctly rounded to float64; then once more:
    lo, hi = sorted((np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))))
    best = min((lo, f, hi), key=lambda c: (abs(Fraction(float(c)) - v), int(bits(c)[0]) & 1))   # double rounding repaired
    return np.float32(best) if best != 0 else np.float32(-0.0 if v < 0 else 0.0)         # an underflow keeps the sign


def mix_exact(a, l, b, r):
    """fma(a, l, round32(b r)) in exact arithmetic; the sign of a zero result as IEEE 754 gives it."""
    t = np.float32(b) * np.float32(r)            # one float32 product: correctly rounded by definition
    assert t == round32(Fraction(float(b)) * Fraction(float(r))) or not np.isfinite(t)
    v = Fraction(float(a)) * Fraction(float(l)) + Fraction(float(t))
    if v != 0:
        return round32(v)
    p = np.float32(a) * np.float32(l)            # an exact zero sum: the signs of the two zeros or of x + (-x)
    if p == 0 and t == 0:
        return np.float32(p) + np.float32(t)
    return np.float32(0.0)


@pytest.mark.parametrize("stereo", [Stereo(width=1.3, balance_db=-2.5, swap=True, invert="left"), Stereo(width=0.37),
                                    Stereo(matrix=[[0.3, -1.7], [1e-3, 2.5]]), Stereo(width=2, channels=1),
                                    Stereo(matrix=[[0.3, -1.7], [1e-3, 2.5]], channels=1)], ids=repr)
@pytest.mark.parametrize("flip", [False, True], ids=["as it is", "right inverted"])
def test_host_image_is_exact(stereo, flip):
    x = samples()
    rec = np.zeros(1, dtype=STEREO_DTYPE)[0]
    rec["corr"] = -0.5 if flip else 0.5
    got = stereo_host(x, stereo, rec=rec)
    m, fold = stereo.matrix_at()
    sg = np.float32(-1.0 if flip else 1.0)
    if stereo.channels == 1:
        want = np.array([[mix_exact(fold[0], l, sg * fold[1], r)] for l, r in x], dtype=np.float32)
    else:
        want = np.array([[mix_exact(m[0, 0], l, sg * m[0, 1], r), mix_exact(m[1, 0], l, sg * m[1, 1], r)] for l, r in x],
                        dtype=np.float32)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))
    if not flip:
        assert np.array_equal(bits(stereo_host(x, stereo)), bits(got))                  # no record: as it is


def test_host_identity_and_width_zero():
    x = samples()
    x[40, 0] = np.nan
    x[41, 1] = np.inf
    assert np.array_equal(bits(stereo_host(x, Stereo())), bits(x))                  # the bits alone: -0, NaN, inf
    assert np.array_equal(bits(stereo_host(x, Stereo(matrix=np.eye(2)))), bits(x))
    y = stereo_host(samples(), Stereo(width=0))
    assert np.array_equal(bits(y[:, 0]), bits(y[:, 1]))
    mono = stereo_host(samples(), Stereo(channels=1))
    assert mono.shape == (300, 1) and np.array_equal(bits(mono[:, 0]), bits(y[:, 0]))   # the same row, folded


def test_host_argument_errors():
    lib = L.lib()
    x = samples()
    m = np.eye(2, dtype=np.float32).reshape(4) * 2
    f = np.array([0.5, 0.5], dtype=np.float32)
    y = np.zeros(300, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.msg_stereo_host(p(x), 2, 300, p(m), None, None, None) == 0
    assert lib.msg_stereo_host(None, 2, 300, p(m), None, None, None) == L.MSG_E_ARG
    assert lib.msg_stereo_host(p(x), 2, 300, None, None, None, None) == L.MSG_E_ARG
    assert lib.msg_stereo_host(p(x), 2, -1, p(m), None, None, None) == L.MSG_E_ARG
    assert lib.msg_stereo_host(p(x), 2, 300, p(m), p(f), None, None) == L.MSG_E_ARG            # a fold needs its output
    assert lib.msg_stereo_host(p(x), 1, 300, p(m), None, None, None) == L.MSG_E_VALUE
    assert lib.msg_stereo_host(p(x), 2, 300, p(m), p(f), p(x), None) == L.MSG_E_VALUE          # the fold onto its input
    flat = x.reshape(-1)
    assert lib.msg_stereo_host(p(x), 2, 300, p(m), p(f), p(flat[599:]), None) == L.MSG_E_VALUE  # its last float
    assert lib.msg_stereo_host(p(x), 2, 300, p(m), p(f), p(y), None) == 0
    bad = np.array([1, 0, 0, np.inf], dtype=np.float32)
    assert lib.msg_stereo_host(p(x), 2, 300, p(bad), None, None, None) == L.MSG_E_VALUE
    assert lib.msg_stereo_host(None, 2, 0, p(m), None, None, None) == 0
    rec = np.zeros(1, dtype=STEREO_DTYPE)
    assert lib.msg_stereo_meter_host(None, 2, 10, 48000, p(rec)) == L.MSG_E_ARG
    assert lib.msg_stereo_meter_host(p(x), 2, 10, 48000, None) == L.MSG_E_ARG
    assert lib.msg_stereo_meter_host(p(x), 1, 10, 48000, p(rec)) == L.MSG_E_VALUE
    assert lib.msg_stereo_meter_host(p(x), 2, 10, 44101, p(rec)) == L.MSG_E_VALUE
    assert lib.msg_stereo_meter_host(p(x), 2, 10, 3990, p(rec)) == L.MSG_E_VALUE
    assert C.sizeof(L.MsgStereoRec) == STEREO_DTYPE.itemsize == 64                       # eight float64, nothing to pad
    with pytest.raises(ValueError):
        stereo_host(np.zeros(10, dtype=np.float32), Stereo(width=0))
    with pytest.raises(ValueError):
        stereo_meter_host(np.zeros((10, 1), dtype=np.float32), 48000)


# ---- msg_stereo_meter_host --------------------------------------------------------------------------
SR = 4000
HOP = SR // 10


def noise(n, seed, scale=0.25):
    return (np.random.default_rng(seed).standard_normal((n, 2)) * scale).astype(np.float32)


def planted():
    """Correlated noise (rho about +0.8) with an antiphase stretch filling block 3 exactly."""
    n = 12 * HOP + 57
    a = noise(n, 21)
    x = np.stack([a[:, 0], 0.8 * a[:, 0] + 0.6 * a[:, 1]], axis=1).astype(np.float32)
    x[3 * HOP:7 * HOP, 1] = -x[3 * HOP:7 * HOP, 0]
    return x


def gate_case():
    """Twelve hops of a constant level a factor 4 under the gate (L = R; hop 2: L = -R) but hop 5, antiphase
    and so loud that each of the four blocks holding it lies a factor 4 over the gate.  Per hop SLL + SRR is
    gate / 16 = hop 0.5e-7, and in hop 5 it is 4 gate - 3 gate / 16.  Blocks 2 .. 5 are kept; block 2 holds
    the other antiphase hop and is the minimum, -15 / 16 against -14.5 / 16."""
    under, loud = math.sqrt(0.25e-7), math.sqrt(15.25e-7)
    x = np.full((12 * HOP, 2), under, dtype=np.float32)
    x[2 * HOP:3 * HOP, 1] = -under
    x[5 * HOP:6 * HOP] = [loud, -loud]
    return x


CASES = {"L = R": lambda: np.repeat(noise(7 * HOP + 3, 1)[:, :1], 2, axis=1),
         "L = -R": lambda: noise(7 * HOP + 3, 2)[:, :1] * np.array([[1, -1]], dtype=np.float32),
         "independent noise": lambda: noise(1 << 16, 3),
         "silent right": lambda: noise(6 * HOP, 4) * np.array([[1, 0]], dtype=np.float32),
         "n = 0": lambda: np.zeros((0, 2), dtype=np.float32),
         "shorter than a block": lambda: noise(4 * HOP - 1, 5),
         "planted": planted, "gate": gate_case}


@pytest.mark.parametrize("name", list(CASES))
def test_meter_host_against_fsum(name):
    x = CASES[name]()
    ref = meter_reference(x, SR)
    got = stereo_meter_host(x, SR)
    if name in ("L = R", "L = -R"):                      # every block has |rho| = 1: the index is a tie of roundings
        ref["corr_min_block"] = int(got["corr_min_block"])
        assert abs(ref["corr"]) == pytest.approx(1.0, abs=1e-12)
    else:
        assert separated(ref), name
    check_meter(name, got, ref)
    if name == "silent right":
        assert got["corr"] == 0.0 and got["blocks_kept"] == 0 and got["corr_min_block"] == -1 and got["corr_min"] == 0.0
    if name in ("n = 0", "shorter than a block"):
        assert got["blocks"] == 0 and got["corr_min_block"] == -1 and got["corr_min"] == got["corr"]
    if name == "planted":
        assert got["corr_min_block"] == 3 and got["corr_min"] == pytest.approx(-1.0, abs=1e-12) and got["corr"] > 0.2
    if name == "gate":
        gate = 8.0 * HOP * 1e-7
        e = ref["energy"]
        assert not np.any((e > gate / 2) & (e < gate * 2))                           # nothing within a factor 2 of it
        assert e[2] == pytest.approx(4 * gate, rel=1e-6) and e[8] == pytest.approx(gate / 4, rel=1e-6)
        assert got["blocks"] == 9 and got["blocks_kept"] == 4 and got["corr_min_block"] == 2
        assert got["corr_min"] == pytest.approx(-15.0 / 16.0, abs=1e-6)
        quiet = stereo_meter_host(x[6 * HOP:], SR)                                     # under the gate: nothing kept
        assert quiet["blocks"] == 3 and quiet["blocks_kept"] == 0 and quiet["corr_min"] == quiet["corr"] == 1.0


def test_derived_columns():
    rows = derive(np.array([stereo_meter_host(CASES[k](), SR) for k in ("L = R", "L = -R", "independent noise",
                                                                        "silent right", "n = 0")]))
    assert rows.dtype == STEREO_ROW_DTYPE and rows.dtype.names[:8] == STEREO_DTYPE.names
    assert rows["mono_db"][0] == pytest.approx(0.0, abs=1e-9) and rows["balance_db"][0] == pytest.approx(0.0, abs=1e-9)
    assert rows["side_db"][0] == -math.inf
    assert rows["mono_db"][1] == -math.inf and rows["side_db"][1] == math.inf
    assert rows["mono_db"][2] == pytest.approx(-3.0103, abs=0.05)                    # corr of 65536 frames: ~ 1 / 256
    assert rows["balance_db"][3] == -math.inf and rows["mono_db"][3] == pytest.approx(-3.0103, abs=1e-3)
    assert np.isnan(rows["mono_db"][4])
    x = CASES["independent noise"]() * np.array([[1.0, 0.5]], dtype=np.float32)
    assert derive(stereo_meter_host(x, SR))["balance_db"] == pytest.approx(-6.0206, abs=0.1)


# ---- the delivery rule ------------------------------------------------------------------------------
def test_delivery_rule():
    from msgpu import batch, dropin
    from msgpu.export import RULES, Delivery
    mono = Stereo(channels=1)
    names = [r[0] for r in RULES]
    assert RULES[names.index("stereo")] == ("stereo", None, "", False)
    assert names.index("stereo") + 1 == names.index("edges") and names.index("filter") == len(names) - 1
    assert [f.name for f in dataclasses.fields(Delivery) if f.init][-1] == "edges"
    d = Delivery(48000, None, -23.0, None, -1.0, 16, stereo=mono)
    assert d.stereo is mono and Delivery().stereo is None and Delivery.stereo is None
    assert d.channels() == 1 and Delivery().channels() == 2 and Delivery(stereo=Stereo(width=0)).channels() == 2
    assert d != Delivery(48000, None, -23.0, None, -1.0, 16) and d == Delivery(48000, None, -23.0, None, -1.0, 16, stereo=mono)
    assert d != Delivery(48000, None, -23.0, None, -1.0, 16, stereo=Stereo(width=0))
    assert repr(d).endswith(", filter=None, stereo=Stereo(width=1.0, balance_db=0.0, swap=False, invert=None, channels=1, "
                            "matrix=None, meter=None))")
    with pytest.raises(TypeError):
        Delivery(*([None] * 12), mono)                                                     # by keyword only
    for fn, word in ((dropin.render_batch, "out_"), (msgpu.render_batch, "out_"), (batch.render_variations, "export_")):
        assert list(inspect.signature(fn).parameters)[-3:] == [word + "stereo", word + "filter", word + "edges"]
    for prefix in ("out_", "export_"):
        Delivery(stereo=mono).check(prefix)
        Delivery(sr=48000, lufs=-23.0, true_peak=-1.0, bits=16, stereo=mono).check(prefix, "device")
        Delivery(stereo=mono).check(prefix, rates=[44101])                                 # a fold meters nothing
        with pytest.raises(ValueError, match=f"{prefix}stereo must be None or a Stereo"):
            Delivery(stereo="mono").check(prefix)
        with pytest.raises(ValueError, match=f"{prefix}stereo: width must be"):
            Delivery(stereo=Stereo(width=5)).check(prefix)
        with pytest.raises(ValueError, match=f"{prefix}stereo: channels must be"):
            Delivery(stereo=Stereo(channels=3)).check(prefix)
        for metering in (Stereo(meter=[]), Stereo(invert="auto")):
            with pytest.raises(ValueError, match=f"{prefix}stereo meters rates that are multiples of 10, at least 4000"):
                Delivery(stereo=metering).check(prefix, rates=[48000, 44101])
            with pytest.raises(ValueError, match=f"{prefix}stereo meters rates"):
                Delivery(sr=44101, stereo=metering).check(prefix, rates=[48000])
            Delivery(sr=48000, stereo=metering).check(prefix, rates=[44101])               # metered at the delivered rate
        with pytest.raises(NotImplementedError, match=f"{prefix}stereo on more than one device"):
            Delivery(stereo=mono).check(prefix, n_devices=2)
        with pytest.raises(ValueError, match=f"{prefix}stereo applies to results 'audio' or 'device'"):
            Delivery(stereo=mono).check(prefix, "stats")
        with pytest.raises(ValueError, match=f"{prefix}edges"):                             # the earlier rules' lines win
            Delivery(edges="x", stereo="y").check(prefix)
        with pytest.raises(ValueError, match=f"{prefix}filter must be"):
            Delivery(filter="x", stereo="y").check(prefix)
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], devices=[0, 1], out_stereo=mono)
    with pytest.raises(ValueError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], results="stats", out_stereo=mono)
    with pytest.raises(ValueError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], out_stereo=Stereo(width=-1))
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(dict(msgpu.DEFAULTS), [1000], [1.0], [1.0], devices=[0, 1], export_stereo=mono)
    with pytest.raises(ValueError):
        msgpu.render_variations(dict(msgpu.DEFAULTS), [1000], [1.0], [1.0], export_stereo=Stereo(invert="up"))
    assert callable(msgpu.stereo) and callable(msgpu.stereo_meter) and msgpu.Stereo is Stereo


def test_mono_through_the_host_side_of_the_chain(tmp_path):
    """The shapes a mono delivery takes on the host: unpack_all by channel count, the WAV writers by shape."""
    from msgpu.batch import read_wav_float32, write_wav_float32
    from msgpu.export import unpack_all
    from msgpu.pcm import pack, read_wav_pcm, write_wav_pcm
    q = (np.arange(-5, 6, dtype=np.int32) * 1000).reshape(-1, 1)
    for b, dt in ((16, np.int16), (24, np.int32)):
        raw = pack(q.astype(dt), b)
        got = unpack_all(raw, [0], [raw.size], b, channels=1)[0]
        assert got.shape == (11, 1) and np.array_equal(got, q)
        assert unpack_all(np.concatenate([raw, raw]), [0], [2 * raw.size], b)[0].shape == (11, 2)   # the default stays 2
        path = str(tmp_path / f"mono{b}.wav")
        write_wav_pcm(path, got, 48000, b)
        back, sr, bb = read_wav_pcm(path)
        assert back.shape == (11, 1) and (sr, bb) == (48000, b) and np.array_equal(back, q)
    path = str(tmp_path / "mono.wav")
    write_wav_float32(path, np.linspace(-1, 1, 7, dtype=np.float32).reshape(-1, 1), 44100)
    back, sr = read_wav_float32(path)
    assert back.shape == (7, 1) and sr == 44100
