"""The delivery filter without a device: the designs of msgpu/filter.py against scipy and the Audio EQ
Cookbook, the library's host loop (msg_filter_host, csrc/filter.h) against scipy.signal.sosfilt, the
struct layout and the refusals, and the delivery rule (msgpu/export.py).  Cases and bars are in
tests/filter_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.signal import butter

import filter_cases as FC
import msgpu
from msgpu import _lib as L
from msgpu.filter import (MAX_SECTIONS, REVERSE, Filter, _opts, filter_host, filter_reference, sos_host,
                          sos_reference)


# ---- designs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["highpass", "lowpass"])
@pytest.mark.parametrize("sr", FC.BUTTER_RATES)
def test_butterworth_against_scipy(kind, sr):
    """Each design's float64 impulse response over 2^16 frames lies no further from the
    extended-precision design's than 4 x scipy's own does (filter_cases.MEASURED_SCIPY)."""
    for order in FC.BUTTER_ORDERS:
        for f in FC.BUTTER_FREQS:
            mine, theirs = FC.design_distances(order, f, kind, sr)
            print(f"butter({order}, {f:g} Hz, {kind}, {sr}): under test {mine:.2e}, scipy {theirs:.2e}")
            assert mine <= FC.DESIGN_FACTOR * theirs, (order, f, kind, sr, mine, theirs)
            sos = Filter(**{kind: (f, order)}).design(sr)
            assert sos.shape == ((order + 1) // 2, 6) and sos.dtype == np.float64 and np.all(sos[:, 3] == 1.0)
            if order % 2:                               # the real pole: one first-order section
                assert sos[-1, 2] == 0.0 and sos[-1, 5] == 0.0
            # the same poles as scipy's, whatever the pairing: the denominators' product
            a_mine, a_ref = np.ones(1), np.ones(1)
            for row in sos:
                a_mine = np.convolve(a_mine, row[3:])
            for row in butter(order, f, kind, fs=sr, output="sos"):
                a_ref = np.convolve(a_ref, row[3:])
            assert np.allclose(a_mine[:len(a_ref)], a_ref, rtol=1e-6, atol=1e-9)


def test_default_order_is_two():
    assert np.array_equal(Filter(highpass=20).design(48000), Filter(highpass=(20, 2)).design(48000))
    assert np.array_equal(Filter(lowpass=18000.0).design(48000), Filter(lowpass=(18000.0, 2)).design(48000))


COOKBOOK = [(kind, f, g, q, sr) for kind in ("peak", "low_shelf", "high_shelf")
            for f, g, q in ((100.0, 6.0, 0.7), (1000.0, -9.0, 2.0), (8000.0, 3.5, 1.0 / np.sqrt(2.0)))
            for sr in (44100, 48000, 384000)]


@pytest.mark.parametrize("kind,f,g,q,sr", COOKBOOK)
def test_cookbook_sections(kind, f, g, q, sr):
    spec = {"peaks": [(f, g, q)]} if kind == "peak" else {kind: (f, g, q)}
    sos = Filter(**spec).design(sr)
    assert sos.shape == (1, 6)
    # the float64 restatement: 1 - cos w0 loses digits at low f / sr, the extended evaluation does not
    ref = FC.cookbook_reference(kind, f, g, q, sr)
    lost = 2.0 ** -52 / (1.0 - np.cos(2.0 * np.pi * f / sr))
    assert np.allclose(sos[0], ref, rtol=0, atol=64.0 * lost * max(1.0, 10.0 ** (abs(g) / 20.0)))
    tol = 1e-9                                          # dB: float64 coefficients, extended evaluation
    dc, ny = FC.gain_db_at(sos, sr * 1e-9, sr), FC.gain_db_at(sos, sr / 2.0, sr)
    if kind == "peak":
        assert abs(FC.gain_db_at(sos, f, sr) - g) <= tol and abs(dc) <= 1e-6 and abs(ny) <= tol
    elif kind == "low_shelf":
        assert abs(dc - g) <= 1e-6 and abs(ny) <= tol
    else:
        assert abs(dc) <= 1e-6 and abs(ny - g) <= tol
    flat = Filter(**({"peaks": [(f, 0.0, q)]} if kind == "peak" else {kind: (f, 0.0, q)})).design(sr)
    assert np.array_equal(flat[0, :3], flat[0, 3:])     # gain_db = 0: b == a


def test_cascade_order_and_raw_sections():
    raw = butter(2, 5000, "lowpass", fs=48000, output="sos")
    flt = Filter(highpass=(20, 3), low_shelf=(100, 2, 0.7), peaks=[(1000, -3, 1)], high_shelf=(8000, 1, 0.7),
                 lowpass=(16000, 2), sos=raw)
    sos = flt.design(48000)
    assert sos.shape == (7, 6) and flt.n_sections() == 7
    assert np.array_equal(sos[:2], Filter(highpass=(20, 3)).design(48000))
    assert np.array_equal(sos[2:3], Filter(low_shelf=(100, 2, 0.7)).design(48000))
    assert np.array_equal(sos[3:4], Filter(peaks=[(1000, -3, 1)]).design(48000))
    assert np.array_equal(sos[4:5], Filter(high_shelf=(8000, 1, 0.7)).design(48000))
    assert np.array_equal(sos[5:6], Filter(lowpass=(16000, 2)).design(48000))
    assert np.array_equal(sos[6:], raw)


BAD = [Filter(), Filter(highpass=0), Filter(highpass=-5), Filter(highpass=(20, 0)), Filter(highpass=(20, 9)),
       Filter(highpass=(20, 2.5)), Filter(lowpass=float("nan")), Filter(lowpass="20"), Filter(low_shelf=(100, 3)),
       Filter(low_shelf=(100, 3, 0)), Filter(high_shelf=(100, 3, 1000)), Filter(peaks=[(100, float("inf"), 1)]),
       Filter(peaks=[(100, 3, 1)] * 9), Filter(highpass=(20, 8), lowpass=(18000, 8), peaks=[(100, 3, 1)]),
       Filter(sos=np.zeros((0, 6))), Filter(sos=np.ones((2, 5))), Filter(sos=[[1, 0, 0, 2, 0, 0]]),
       Filter(sos=[[1, 0, 0, 1, 0, 1.0]]), Filter(sos=[[1, 0, 0, 1, 2.0, 0.5]]), Filter(sos=[[np.nan, 0, 0, 1, 0, 0]]),
       Filter(highpass=20, zero_phase=1)]


@pytest.mark.parametrize("flt", BAD, ids=[str(i) for i in range(len(BAD))])
def test_check_refuses(flt):
    with pytest.raises(ValueError):
        flt.check()


def test_check_knows_the_rate():
    Filter(highpass=20).check().check(48000)
    Filter(lowpass=23000).check(48000)
    for flt in (Filter(lowpass=24000), Filter(lowpass=30000), Filter(peaks=[(100, 3, 1), (25000, 3, 1)])):
        flt.check()
        with pytest.raises(ValueError, match="sr / 2"):
            flt.check(48000)
        with pytest.raises(ValueError):
            flt.design(48000)
    assert Filter(highpass=(20, 8), sos=np.tile([1.0, 0, 0, 1, 0, 0], (4, 1))).check(48000).n_sections() == MAX_SECTIONS


# ---- msg_filter_host against sosfilt -----------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", list(FC.FILTERS))
def test_host_against_sosfilt(name, channels, reverse):
    flt, sr = FC.FILTERS[name]
    sos = flt.design(sr)
    for label, x in FC.signals(channels):
        ref = sos_reference(x, sos, reverse)
        out = filter_host(x, sr, flt, reverse)
        err, bar = FC.check_against(f"{name} / {label} ch={channels} rev={reverse}", out, ref)
        if len(x) > FC.T:
            print(f"host {name} / {label} ch={channels} rev={reverse}: rms error {err:.3e}, e32 {bar:.3e}")


def test_reverse_is_the_forward_run_of_the_reversed_signal():
    flt, sr = FC.FILTERS["eight sections @ 48k"]
    x = FC.noise(5000, 2, 3)
    assert np.array_equal(FC.bits(filter_host(x, sr, flt, True)), FC.bits(filter_host(x[::-1].copy(), sr, flt)[::-1]))


def test_channels_are_independent_and_start_from_zero_state():
    flt, sr = FC.FILTERS["three sections @ 44.1k"]
    x = FC.noise(3000, 2, 4)
    y = filter_host(x, sr, flt)
    for ch in (0, 1):
        assert np.array_equal(FC.bits(y[:, ch]), FC.bits(filter_host(x[:, ch].copy(), sr, flt)))
    assert np.array_equal(FC.bits(filter_host(x, sr, flt)), FC.bits(y))            # no state is kept between calls


def test_zero_phase_is_forward_then_reverse():
    flt, sr = FC.FILTERS["hp2 20 Hz @ 48k"]
    zp = Filter(highpass=(20, 2), zero_phase=True)
    x = FC.noise(6000, 2, 5)
    two = filter_host(filter_host(x, sr, flt), sr, flt, reverse=True)
    assert np.array_equal(FC.bits(filter_host(x, sr, zp)), FC.bits(two))
    # twice the gain in dB and no phase shift: a symmetric click stays symmetric (to the roundings of two runs)
    peak = Filter(peaks=[(2000, 6.0, 1.0)], zero_phase=True)
    n = 4001
    click = np.exp(-0.5 * ((np.arange(n) - n // 2) / 3.0) ** 2).astype(np.float32)
    y = filter_host(click, 48000, peak).astype(np.float64)
    assert np.max(np.abs(y - y[::-1])) <= 1e-6 * np.max(np.abs(y))
    tone = np.sin(2 * np.pi * 2000 / 48000 * np.arange(48000)).astype(np.float32)
    out = filter_host(tone, 48000, peak)[12000:36000].astype(np.float64)
    assert abs(20 * np.log10(FC.rms(out) / FC.rms(tone[12000:36000])) - 12.0) <= 1e-3


# ---- struct layout and refusals ----------------------------------------------------------------------
def test_struct_layout():
    assert L.lib().msg_sizeof(11) == C.sizeof(L.MsgFilterOpts) == 8 + MAX_SECTIONS * 6 * 8
    assert L.lib().msg_sizeof(12) == -1
    assert L.MsgFilterOpts.sos.offset == 8
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msgpu.h")).read()
    assert "MSG_FILTER_MAX_SECTIONS = 8" in src and "MSG_FILTER_REVERSE = 1" in src and REVERSE == 1


def host_status(sos, n_sections=None, flags=0, channels=1):
    o = _opts(np.asarray(sos, dtype=np.float64).reshape(-1, 6)[:MAX_SECTIONS], False)
    if n_sections is not None:
        o.n_sections = n_sections
    o.flags = flags
    x = np.zeros((8, channels), dtype=np.float32)
    return L.lib().msg_filter_host(x.ctypes.data_as(C.c_void_p), channels, 8, C.byref(o))


def test_value_errors_of_the_library():
    ok = [1.0, 0.5, 0.25, 1.0, -0.5, 0.25]
    assert host_status([ok]) == L.MSG_OK and host_status([ok] * 8) == L.MSG_OK
    assert host_status([ok], flags=REVERSE) == L.MSG_OK
    bad = {"no section": dict(sos=[ok], n_sections=0), "nine sections": dict(sos=[ok] * 8, n_sections=9),
           "negative count": dict(sos=[ok], n_sections=-1), "unknown flag": dict(sos=[ok], flags=2),
           "nan b": dict(sos=[[np.nan, 0, 0, 1, 0, 0]]), "inf a": dict(sos=[[1, 0, 0, 1, np.inf, 0]]),
           "a0 = 2": dict(sos=[[1, 0, 0, 2, 0, 0]]), "a0 = 0": dict(sos=[[1, 0, 0, 0, 0, 0]]),
           "a2 = 1": dict(sos=[[1, 0, 0, 1, 0, 1.0]]), "a2 = -1": dict(sos=[[1, 0, 0, 1, 0, -1.0]]),
           "a1 = 1 + a2": dict(sos=[[1, 0, 0, 1, 1.5, 0.5]]), "a1 = -(1 + a2)": dict(sos=[[1, 0, 0, 1, -1.5, 0.5]]),
           "first order on the circle": dict(sos=[[1, 0, 0, 1, -1.0, 0.0]]),
           "second of two": dict(sos=[ok, [1, 0, 0, 1, 0, 1.5]]), "three channels": dict(sos=[ok], channels=3)}
    for name, kw in bad.items():
        assert host_status(**kw) == L.MSG_E_VALUE, name
        with pytest.raises(ValueError):
            L.check(host_status(**kw), None)
    # inside the triangle, close to its sides
    for a1, a2 in ((1.999, 0.9995), (-1.999, 0.9995), (0.0, -0.999), (0.999, 0.0)):
        assert host_status([[1, 0, 0, 1, a1, a2]]) == L.MSG_OK
    o = _opts([ok], False)
    assert L.lib().msg_filter_host(None, 1, 4, C.byref(o)) == L.MSG_E_ARG
    assert L.lib().msg_filter_host(None, 1, 0, C.byref(o)) == L.MSG_OK
    assert L.lib().msg_filter_host(None, 1, 0, None) == L.MSG_E_ARG
    with pytest.raises(ValueError):
        sos_host(np.zeros(4, np.float32), [[1, 0, 0, 1, 0, 1.0]])


# ---- the delivery rule -------------------------------------------------------------------------------
def test_delivery_rule():
    from msgpu.export import RULES, Delivery
    import dataclasses
    import inspect

    from msgpu import batch, dropin
    hp = Filter(highpass=(20, 4))
    # the rule after edges: a keyword of Delivery (the dataclass fields and their order are pinned by the
    # earlier rules' tests), seen by == and repr, kept by check and one_device like any other rule
    assert RULES[-2][0] == "edges" and RULES[-1] == ("filter", None, "", False)
    assert [f.name for f in dataclasses.fields(Delivery) if f.init][-1] == "edges"
    d = Delivery(48000, None, -23.0, None, -1.0, 16, filter=hp)
    assert d.filter is hp and Delivery().filter is None and Delivery.filter is None
    assert d != Delivery(48000, None, -23.0, None, -1.0, 16) and d == Delivery(48000, None, -23.0, None, -1.0, 16, filter=hp)
    assert "filter=Filter(highpass=(20, 4)" in repr(d)
    with pytest.raises(TypeError):
        Delivery(*([None] * 12), hp)                                                       # by keyword only
    # in the front ends' signatures it stands in front of the edges keyword, as in the chain
    for fn, word in ((dropin.render_batch, "out_"), (msgpu.render_batch, "out_"), (batch.render_variations, "export_")):
        assert list(inspect.signature(fn).parameters)[-2:] == [word + "filter", word + "edges"]
    for prefix in ("out_", "export_"):
        Delivery(filter=hp).check(prefix)
        Delivery(sr=48000, lufs=-23.0, true_peak=-1.0, bits=16, filter=hp).check(prefix, "device")
        with pytest.raises(ValueError, match=f"{prefix}filter must be None or a Filter"):
            Delivery(filter="highpass").check(prefix)
        with pytest.raises(ValueError, match=f"{prefix}filter: the filter is empty"):
            Delivery(filter=Filter()).check(prefix)
        with pytest.raises(ValueError, match=f"{prefix}filter: the frequency of lowpass"):
            Delivery(filter=Filter(lowpass=23000)).check(prefix, rates=[48000, 44100])
        with pytest.raises(ValueError, match=f"{prefix}filter: the frequency of lowpass"):
            Delivery(sr=44100, filter=Filter(lowpass=23000)).check(prefix, rates=[48000])
        Delivery(sr=48000, filter=Filter(lowpass=23000)).check(prefix, rates=[44100])      # filtered at the delivered rate
        with pytest.raises(NotImplementedError, match=f"{prefix}filter on more than one device"):
            Delivery(filter=hp).check(prefix, n_devices=2)
        with pytest.raises(ValueError, match=f"{prefix}filter applies to results 'audio' or 'device'"):
            Delivery(filter=hp).check(prefix, "stats")
        with pytest.raises(ValueError, match=f"{prefix}edges"):                             # the earlier rule's lines win
            Delivery(edges="x", filter="y").check(prefix)
    hp = Filter(highpass=(20, 4))
    with pytest.raises(NotImplementedError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], devices=[0, 1], out_filter=hp)
    with pytest.raises(ValueError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], results="stats", out_filter=hp)
    with pytest.raises(ValueError):
        msgpu.render_batch([dict(msgpu.DEFAULTS)], out_filter=Filter())
    with pytest.raises(NotImplementedError):
        msgpu.render_variations(dict(msgpu.DEFAULTS), [1000], [1.0], [1.0], devices=[0, 1], export_filter=hp)
    with pytest.raises(ValueError):
        msgpu.render_variations(dict(msgpu.DEFAULTS), [1000], [1.0], [1.0], export_filter=Filter(highpass=40000))
    assert callable(msgpu.filter) and msgpu.Filter is Filter
