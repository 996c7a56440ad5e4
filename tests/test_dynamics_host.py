"""The compressor without a device: the library's own log2 and exp2 against numpy.longdouble, the
host loop (msg_dynamics_host, csrc/dynamics.h) against the float64 reference of msgpu/dynamics.py
at the tolerances of tests/dynamics_cases.py, its behaviour on signals whose answer is known, the
refusals, the tiled evaluation against the sequential one under the sanitizers
(tests/dynamics_check.cpp), and the delivery rule (msgpu/export.py)."""
import ctypes as C
import dataclasses
import inspect
import math

import numpy as np
import pytest

import msgpu
from msgpu import _lib as L
from msgpu.dynamics import (DYNAMICS_DTYPE, DYNAMICS_ROW_DTYPE, E_MAX, UNIT, Dynamics, curve_reference, derive,
                            dynamics_host, dynamics_reference, host, p0, step)

import dynamics_cases as DC

SR = DC.SR


# ---- the math routines --------------------------------------------------------------------------
def _debug(name, arg):
    fn = getattr(L.lib(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    out = np.zeros(len(arg), dtype=np.float64)
    assert fn(arg.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), len(arg)) == 0
    return out


def test_log2_within_2_to_minus_40_over_every_exponent():
    """Every float32 exponent, denormals included, at the mantissa's ends, around sqrt 2 where the
    routine halves m, and at random mantissas: |dyn_log2 - log2| <= 2^-40, absolute."""
    rng = np.random.default_rng(1)
    mant = np.concatenate([[0, 1, 2, 0x3504f2, 0x3504f3, 0x3504f4, 0x400000, 0x7ffffe, 0x7fffff],
                           rng.integers(0, 1 << 23, 64)]).astype(np.uint32)
    expo = np.arange(0, 255, dtype=np.uint32)                     # 0: the denormals
    b = ((expo[:, None] << 23) | mant[None, :]).reshape(-1)
    b = np.concatenate([b[b > 0], (1 << np.arange(23, dtype=np.uint32))])     # every denormal binade too
    p = np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)
    assert np.all(p > 0) and np.all(np.isfinite(p)) and p.min() == np.float32(2.0 ** -149)
    got = _debug("msg_debug_dyn_log2", p)
    want = np.log2(p.astype(np.longdouble))
    err = float(np.max(np.abs(got.astype(np.longdouble) - want)))
    print(f"dyn_log2: {p.size} values, max |error| {err:.3e} (2^-40 = {2.0 ** -40:.3e})")
    assert np.finfo(np.longdouble).nmant >= 63                    # the yardstick is wider than float64
    assert err <= 2.0 ** -40
    assert got[p == 1.0][0] == 0.0 and got[p == 2.0][0] == 1.0


def test_exp2_within_2_to_minus_40_relative():
    """Over [-60, 60], the range csrc/dynamics.h states: the issue's [-43, 43] and beyond it what the gain
    can reach, (makeup - E) log2(10) / 20 from -50.5 (256 dB of reduction under -48 dB of makeup) to 8."""
    rng = np.random.default_rng(2)
    k = np.arange(-60, 61, dtype=np.float64)
    x = np.concatenate([k, k[:-1] + 0.5, np.nextafter(k[:-1] + 0.5, 100.0), np.nextafter(k[1:] - 0.5, -100.0),
                        rng.uniform(-60.0, 60.0, 30000), rng.uniform(-1e-6, 1e-6, 1000),
                        [(-48.0 - 256.0) * math.log2(10.0) / 20.0, 48.0 * math.log2(10.0) / 20.0]])
    got = _debug("msg_debug_dyn_exp2", np.ascontiguousarray(x))
    want = np.exp2(x.astype(np.longdouble))
    err = float(np.max(np.abs(got.astype(np.longdouble) - want) / want))
    print(f"dyn_exp2: {x.size} values, max relative error {err:.3e} (2^-40 = {2.0 ** -40:.3e})")
    assert err <= 2.0 ** -40
    assert _debug("msg_debug_dyn_exp2", np.zeros(1))[0] == 1.0
    assert np.array_equal(_debug("msg_debug_dyn_exp2", k), 2.0 ** k)          # 2^k by bits


def test_steps_and_threshold():
    assert step(0.0, SR) == E_MAX and step(1e-9, SR) == E_MAX     # instant
    assert step(5.0, SR) == math.floor(10.0 * UNIT / 240.0 + 0.5)
    assert step(1e12, SR) == 1
    for thr, knee in ((-18.0, 6.0), (-150.0, 0.0), (24.0, 48.0), (-23.7, 1.3)):
        v = p0(thr, knee)
        lin = 10.0 ** ((thr - knee / 2.0) / 20.0)
        assert v.dtype == np.float32 and float(v) <= lin < float(np.nextafter(v, np.float32(np.inf)))


# ---- the host loop against the reference --------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", list(DC.OPTIONS))
def test_host_against_reference(name, channels):
    dyn = DC.OPTIONS[name]
    for n in (1, 17, DC.TILE + 1, 3 * DC.TILE + 5):
        x = DC.texture(n, channels, 10 * n + channels)
        y, rec, e = dynamics_host(x, SR, dyn, env=True)
        y2, rec2 = dynamics_host(x, SR, dyn)
        assert np.array_equal(DC.bits(y), DC.bits(y2)) and rec.tobytes() == rec2.tobytes()
        y_ref, e_ref = dynamics_reference(x, SR, dyn)
        de, dy = int(np.max(np.abs(e - e_ref))), DC.within(y, y_ref)
        if n == 3 * DC.TILE + 5:
            print(f"{name}, {channels} ch: max |E - E_ref| {de} units, samples at {dy:.3f} of their allowance, "
                  f"max reduction {rec['max_e'] / UNIT:.3f} dB over {int(rec['reduced_frames'])} frames")
        assert de <= DC.E_UNITS and dy <= 1.0
        assert rec["max_e"] == e.max() and rec["sum_e16"] == int(np.sum(e >> 16)) and rec["reduced_frames"] == np.sum(e > 0)
        assert rec["hold_frames"] == dyn.opts(SR).hold_frames
        assert rec["state"] == (1 if (e > 0).any() or dyn.makeup_db != 0 else 0)
        assert y.dtype == np.float32 and y.shape == x.shape


# ---- behaviour ----------------------------------------------------------------------------------
def test_steady_sine_settles_at_the_static_curve():
    """-6 dBFS at 1 kHz, 4:1 over -18 dB, hard knee: the samples hit the crest every 24 frames, so the
    reduction sits between the curve at the crest and one release step per frame of half a period under it."""
    dyn = Dynamics(threshold_db=-18.0, ratio=4.0, knee_db=0.0, attack_ms=5.0, release_ms=150.0)
    x = (10.0 ** (-6.0 / 20.0) * np.sin(2.0 * np.pi * np.arange(SR) / 48.0)).astype(np.float32)
    _, rec, e = dynamics_host(x, SR, dyn, env=True)
    crest = 20.0 * math.log10(float(np.abs(x).max()))
    top = 0.75 * (crest + 18.0) * UNIT
    inner = e[480:-480]
    print(f"steady sine: reduction {inner.min() / UNIT:.4f} .. {inner.max() / UNIT:.4f} dB, the curve at the crest "
          f"{top / UNIT:.4f} dB, ripple allowed {24 * step(150.0, SR) / UNIT:.4f} dB")
    assert abs(inner.max() - top) <= 1.0 and rec["max_e"] == inner.max()
    assert inner.min() >= top - 24 * step(150.0, SR) - 1.0
    assert top / UNIT == pytest.approx(9.0, abs=0.01)


def test_ramp_follows_the_three_branches_of_the_knee():
    dyn = Dynamics(threshold_db=-20.0, ratio=5.0, knee_db=10.0, attack_ms=0.0, release_ms=0.0)
    lev = np.linspace(-40.0, 0.0, 4001)
    x = (10.0 ** (lev / 20.0)).astype(np.float32) * np.where(np.arange(4001) % 2, -1.0, 1.0).astype(np.float32)
    _, _, e = dynamics_host(x, SR, dyn, env=True)                 # instant ballistics: E is the demand
    got = 20.0 * np.log10(np.abs(x).astype(np.float64))
    want = curve_reference(got, -20.0, 5.0, 10.0)
    below, knee, above = got < -25.0 - 1e-9, np.abs(got + 20.0) < 5.0 - 1e-9, got > -15.0 + 1e-9
    assert below.sum() > 1000 and knee.sum() > 900 and above.sum() > 1000
    assert np.all(e[below] == 0)
    assert np.max(np.abs(e - want * UNIT)) <= 1.0                 # the rounding to a unit, either way at a tie
    assert np.allclose(want[above], 0.8 * (got[above] + 20.0), atol=1e-12)
    assert np.allclose(want[knee], 0.8 * (got[knee] + 25.0) ** 2 / 20.0, atol=1e-12)
    assert np.all(np.diff(e) >= 0)                                # monotone through both joins


def test_ratio_inf_pins_the_level_at_the_threshold():
    dyn = Dynamics(threshold_db=-12.0, ratio=math.inf, knee_db=0.0, attack_ms=0.0, release_ms=0.0)
    lev = np.linspace(-11.9, 0.0, 500)
    x = (10.0 ** (lev / 20.0)).astype(np.float32)
    y, rec = dynamics_host(np.stack([x, -0.5 * x], axis=1), SR, dyn)
    out_db = 20.0 * np.log10(np.abs(y[:, 0]).astype(np.float64))
    print(f"ratio inf: output level {out_db.min():.7f} .. {out_db.max():.7f} dB")
    assert np.max(np.abs(out_db + 12.0)) <= 20.0 * math.log10(1.0 + 2.0 ** -22)      # two float32 roundings
    assert np.array_equal(y[:, 1], (-0.5 * y[:, 0]).astype(np.float32))              # linked: one gain for both
    assert rec["state"] == 1 and rec["reduced_frames"] == 500


def test_untouched_makeup_nonfinite_and_short_signals():
    x = DC.texture(5000, 2, 3)
    y, rec = dynamics_host(x, SR, Dynamics(threshold_db=0.5, knee_db=0.0))
    assert np.array_equal(DC.bits(y), DC.bits(x)) and rec["state"] == 0 and rec["max_e"] == 0 and rec["reduced_frames"] == 0
    y, rec = dynamics_host(x, SR, Dynamics(threshold_db=6.0, knee_db=6.0))           # the knee starts above full scale too
    assert np.array_equal(DC.bits(y), DC.bits(x)) and rec["state"] == 0
    # makeup alone is one multiply by one float32 gain
    up = Dynamics(threshold_db=24.0, knee_db=0.0, makeup_db=6.0)
    g = dynamics_host(np.ones(1, dtype=np.float32), SR, up)[0][0]
    assert abs(float(g) - 10.0 ** 0.3) <= 2.0 ** -24 * 10.0 ** 0.3
    y, rec = dynamics_host(x, SR, up)
    assert np.array_equal(DC.bits(y), DC.bits(x * g)) and rec["state"] == 1 and rec["reduced_frames"] == 0
    for poison in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (4999, 1), (2500, 0)):
            z = x.copy()
            z[at] = poison
            y, rec = dynamics_host(z, SR, Dynamics(makeup_db=3.0))
            assert np.array_equal(DC.bits(y), DC.bits(z)), (poison, at)
            assert rec["state"] == 2 and rec["max_e"] == 0 and rec["sum_e16"] == 0 and rec["reduced_frames"] == 0
    for ch in (1, 2):
        y, rec = dynamics_host(np.zeros((0, 2) if ch == 2 else (0,), dtype=np.float32), SR, Dynamics(makeup_db=3.0))
        assert y.shape[0] == 0 and rec["state"] == 0 and rec["max_e"] == 0
        one = np.full((1, 2) if ch == 2 else (1,), 0.5, dtype=np.float32)
        y, rec, e = dynamics_host(one, SR, Dynamics(), env=True)
        want = curve_reference(20.0 * math.log10(0.5), -18.0, 3.0, 6.0)
        assert abs(int(e[0]) - float(want) * UNIT) <= 1.0 and rec["reduced_frames"] == 1 and rec["state"] == 1
        assert DC.within(y, one.astype(np.float64) * 10.0 ** (-float(e[0]) / UNIT / 20.0)) <= 1.0


def test_derived_columns():
    _, rec, e = dynamics_host(DC.texture(9000, 2, 8), SR, Dynamics(), env=True)
    rows = derive(np.array([rec, np.zeros(1, dtype=DYNAMICS_DTYPE)[0]]))
    assert rows.dtype == DYNAMICS_ROW_DTYPE and rows.dtype.names[:5] == DYNAMICS_DTYPE.names
    assert rows["max_reduction_db"][0] == e.max() / UNIT
    assert rows["mean_reduction_db"][0] == pytest.approx(e[e > 0].mean() / UNIT, abs=2.0 ** -16)
    assert rows["mean_reduction_db"][1] == 0.0 and rows["reduced_frames"][0] == (e > 0).sum() and rows["state"][0] == 1


# ---- refusals -----------------------------------------------------------------------------------
BAD_FIELDS = [("threshold_db", -151.0), ("threshold_db", 24.5), ("threshold_db", math.nan), ("threshold_db", "loud"),
              ("ratio", 0.99), ("ratio", math.nan), ("ratio", None), ("knee_db", -0.1), ("knee_db", 48.5),
              ("knee_db", math.inf), ("attack_ms", -1.0), ("attack_ms", math.inf), ("release_ms", -0.5),
              ("release_ms", True), ("hold_ms", -1.0), ("hold_ms", math.nan), ("makeup_db", 48.5), ("makeup_db", -49.0),
              ("makeup_db", math.inf)]


@pytest.mark.parametrize("field,value", BAD_FIELDS, ids=[f"{k}={v}" for k, v in BAD_FIELDS])
def test_check_names_the_field(field, value):
    with pytest.raises(ValueError, match=f"^{field} must be"):
        Dynamics(**{field: value}).check()


def test_check_at_a_rate_and_the_library_refusals():
    Dynamics(hold_ms=DC.hold_ms(4096)).check(SR)
    Dynamics(ratio=math.inf, knee_db=0, attack_ms=0, release_ms=0).check(SR)
    with pytest.raises(ValueError, match="^hold_ms is more than 4096 frames at 48000 Hz"):
        Dynamics(hold_ms=DC.hold_ms(4097)).check(SR)
    with pytest.raises(ValueError, match="the sample rate must be positive"):
        Dynamics().check(0)
    x = np.zeros((8, 2), dtype=np.float32)
    good = Dynamics().opts(SR)

    def call(channels=2, **kw):
        o = L.MsgDynamicsOpts.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            setattr(o, k, v)
        return host(x.copy(), channels, o)

    call()
    for kw, wording in (({"threshold_db": math.nan}, "the threshold must be a finite number of dB from -150 to 24"),
                        ({"threshold_db": -150.5}, "the threshold must be"), ({"threshold_db": 24.5}, "the threshold must be"),
                        ({"ratio": 0.5}, "the ratio must be at least 1"), ({"ratio": math.nan}, "the ratio must be at least 1"),
                        ({"knee_db": -1.0}, "the knee must be a finite number of dB from 0 to 48"),
                        ({"knee_db": math.inf}, "the knee must be"), ({"makeup_db": 48.5}, "the makeup gain must be"),
                        ({"makeup_db": math.nan}, "the makeup gain must be a finite number of dB from -48 to 48"),
                        ({"attack_step": 0}, r"the attack and release steps must lie in 1 \.\. 2\^40"),
                        ({"release_step": E_MAX + 1}, "the attack and release steps"), ({"flags": 1}, "flags must be 0"),
                        ({"hold_frames": -1}, "the hold must be a frame count from 0 up")):
        with pytest.raises(ValueError, match=wording):
            call(**kw)
    with pytest.raises(NotImplementedError, match="hold beyond 4096 frames"):
        call(hold_frames=4097)
    with pytest.raises(ValueError, match="channels must be 1 or 2"):
        call(channels=3)
    call(attack_step=E_MAX, release_step=1, hold_frames=4096, ratio=math.inf)
    with pytest.raises(ValueError, match=r"x must be \(n,\) or \(n, 2\)"):
        dynamics_host(np.zeros((4, 3), dtype=np.float32), SR, Dynamics())


def test_struct_sizes():
    assert C.sizeof(L.MsgDynamicsOpts) == 56 and C.sizeof(L.MsgDynamicsRec) == DYNAMICS_DTYPE.itemsize == 32
    assert L.lib().msg_sizeof(12) == -1                            # no msg_sizeof entry: the sizes are pinned here
    assert [f[0] for f in L.MsgDynamicsRec._fields_] == list(DYNAMICS_DTYPE.names)
    # the last fields of both structs meet in the record: a layout slip would not survive the round trip
    _, rec = dynamics_host(np.ones(3, dtype=np.float32), SR, Dynamics(hold_ms=DC.hold_ms(77)))
    assert rec["hold_frames"] == 77 and rec["reduced_frames"] == 3 and rec["state"] == 1


# ---- the header under the sanitizers ------------------------------------------------------------
@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
def test_tiled_equals_sequential_under_asan_ubsan(tmp_path):
    """csrc/dynamics.h in a stand-alone program (tests/dynamics_check.cpp) under ASan + UBSan: every
    case through the sequential loop and tile by tile through the kernels' helpers, at tile sizes 16,
    4096 and 1000: the envelope, the samples and the record are equal."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "dynamics_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(repo, "audio-suite_amd", "csrc"),
                    "-o", exe, os.path.join(repo, "tests", "dynamics_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "bad 0" in out, out[-4000:]


# ---- the delivery rule --------------------------------------------------------------------------
def test_delivery_rule():
    from msgpu import batch, dropin
    from msgpu.export import RULES, Delivery
    dyn = Dynamics(ratio=4.0)
    names = [r[0] for r in RULES]
    assert RULES[names.index("dynamics")] == ("dynamics", None, "", False)
    assert names[-4:] == ["dynamics", "stereo", "edges", "filter"]
    assert [f.name for f in dataclasses.fields(Delivery) if f.init][-1] == "edges"
    d = Delivery(48000, None, -23.0, None, -1.0, 16, dynamics=dyn)
    assert d.dynamics is dyn and Delivery().dynamics is None and Delivery.dynamics is None and d.channels() == 2
    assert d != Delivery(48000, None, -23.0, None, -1.0, 16) and d == Delivery(48000, None, -23.0, None, -1.0, 16, dynamics=Dynamics(ratio=4.0))
    assert d != Delivery(48000, None, -23.0, None, -1.0, 16, dynamics=Dynamics(ratio=5.0))
    assert repr(d).endswith(", dynamics=Dynamics(threshold_db=-18.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=150.0, "
                            "hold_ms=0.0, makeup_db=0.0), filter=None, stereo=None)")
    with pytest.raises(TypeError):
        Delivery(*([None] * 12), dyn)                                                      # by keyword only
    for fn, word in ((dropin.render_batch, "out_"), (msgpu.render_batch, "out_"), (batch.render_variations, "export_")):
        assert list(inspect.signature(fn).parameters)[-4:] == [word + k for k in ("dynamics", "stereo", "filter", "edges")]
    for prefix in ("out_", "export_"):
        Delivery(dynamics=dyn).check(prefix)
        Delivery(sr=48000, lufs=-23.0, true_peak=-1.0, bits=16, dynamics=dyn).check(prefix, "device", rates=[44101])
        with pytest.raises(ValueError, match=f"{prefix}dynamics must be None or a Dynamics"):
            Delivery(dynamics="squash").check(prefix)
        with pytest.raises(ValueError, match=f"{prefix}dynamics: ratio must be at least 1"):
            Delivery(dynamics=Dynamics(ratio=0.5)).check(prefix)
        with pytest.raises(ValueError, match=f"{prefix}dynamics: threshold_db must be"):
            Delivery(dynamics=Dynamics(threshold_db=30)).check(prefix)
        long_hold = Dynamics(hold_ms=50.0)                                                 # 2400 frames at 48 kHz, 9600 at 192 kHz
        Delivery(dynamics=long_hold).check(prefix, rates=[48000])
        with pytest.raises(ValueError, match=f"{prefix}dynamics: hold_ms is more than 4096 frames at 192000 Hz"):
            Delivery(dynamics=long_hold).check(prefix, rates=[48000, 192000])
        with pytest.raises(ValueError, match=f"{prefix}dynamics: hold_ms is more than"):
            Delivery(sr=192000, dynamics=long_hold).check(prefix, rates=[48000])
        Delivery(sr=48000, dynamics=long_hold).check(prefix, rates=[192000])               # held at the delivered rate
        with pytest.raises(NotImplementedError, match=f"{prefix}dynamics on more than one device"):
            Delivery(dynamics=dyn).check(prefix, n_devices=2)
        with pytest.raises(ValueError, match=f"{prefix}dynamics applies to results 'audio' or 'device'"):
            Delivery(dynamics=dyn).check(prefix, "stats")
        with pytest.raises(ValueError, match=f"{prefix}stereo must be"):                    # the earlier rules' lines win
            Delivery(stereo="x", dynamics="y").check(prefix)
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], devices=[0, 1], out_dynamics=dyn)
    with pytest.raises(ValueError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], results="stats", out_dynamics=dyn)
    with pytest.raises(ValueError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], out_dynamics=Dynamics(knee_db=-1))
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(dict(msgpu.DEFAULTS), [1000], [1.0], [1.0], devices=[0, 1], export_dynamics=dyn)
    with pytest.raises(ValueError):
        msgpu.render_variations(dict(msgpu.DEFAULTS), [1000], [1.0], [1.0], export_dynamics=Dynamics(makeup_db=60))
    assert callable(msgpu.dynamics) and msgpu.Dynamics is Dynamics
