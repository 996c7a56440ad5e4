"""The edges pass on the host (msg_edges_host, csrc/edges.h) against the NumPy restatement of
its definition (msgpu.edges.edges_reference): records exactly, samples to the bit around the
library's own gains, the gains within the derived 2^-24 of the float64 curves, and the
delivery rules of the new option.  Signals and options: tests/edges_cases.py.  No GPU here."""
import ctypes as C

import numpy as np
import pytest

import edges_cases as EC
import msgpu
from msgpu import _lib as L
from msgpu.edges import (EDGES_DTYPE, SILENT, TILE, Edges, curve_reference, edges_host, edges_reference, frames, gains,
                         gains_reference, loop_gains, loop_gains_reference, threshold)

T = TILE
VE, NIE = ValueError, NotImplementedError


@pytest.mark.parametrize("config", list(EC.CONFIGS))
@pytest.mark.parametrize("channels", [1, 2])
def test_host_equals_the_definition(channels, config):
    """Every signal under every option: the record exactly, every word to the bit."""
    e = EC.CONFIGS[config]
    for name, x in EC.signals(channels):
        y, rec = edges_host(x, EC.SR, e)
        y_want, rec_want = EC.library_reference(x, e)
        EC.assert_same(f"{config} / {name} ch={channels}", y, rec, y_want, rec_want)
        # outside the fades, and outside the span, nothing is touched
        n, s, end = len(x), int(rec["start"]), int(rec["end"])
        keep = np.ones(n, dtype=bool)
        keep[s:s + int(rec["fade_in"]) + int(rec["loop"])] = False
        keep[end - int(rec["fade_out"]):end] = False
        assert np.array_equal(EC.bits(y)[keep], EC.bits(x)[keep]), name
        assert 0 <= s <= end <= n and rec["fade_in"] + rec["fade_out"] <= end - s


@pytest.mark.parametrize("channels", [1, 2])
def test_spans(channels):
    """The spans written out: the single frames, the threshold, the pads' clipping, the silent
    signals, n = 0."""
    sig = dict(EC.signals(channels))
    both = Edges(trim_db=EC.TRIM_DB)
    for f in (0, EC.N - 1, T - 1, T):
        x = sig[f"one sound frame at {f}"]
        for sides, want in (("both", (f, f + 1)), ("head", (f, EC.N)), ("tail", (0, f + 1))):
            rec = edges_host(x, EC.SR, Edges(trim_db=EC.TRIM_DB, sides=sides))[1]
            assert (rec["first"], rec["last"], rec["start"], rec["end"], rec["flags"]) == (f, f, *want, 0)
        # the fades of one frame: Fi' = floor(1 * 96 / 1056) = 0, Fo' = 1
        y, rec = edges_host(x, EC.SR, EC.CONFIGS["fades clip"])
        assert (rec["fade_in"], rec["fade_out"]) == (0, 1)
        assert np.array_equal(y[f], (x[f].astype(np.float64) * np.float64(gains("hann", 1)[1][0])).astype(np.float32))
        rec = edges_host(x, EC.SR, EC.CONFIGS["fade-in only"])[1]
        assert (rec["fade_in"], rec["fade_out"]) == (1, 0)
    rec = edges_host(sig["at the threshold"], EC.SR, both)[1]
    assert (rec["first"], rec["last"], rec["start"], rec["end"], rec["flags"]) == (100, 100, 100, 101, 0)
    for name in ("one ulp below the threshold", "all silent", "all zero"):
        x = sig[name]
        y, rec = edges_host(x, EC.SR, EC.CONFIGS["both"])
        assert (rec["first"], rec["last"], rec["start"], rec["end"], rec["flags"]) == (-1, -1, 0, len(x), SILENT), name
        assert (rec["fade_in"], rec["fade_out"]) == (96, 960)            # a silent render is delivered whole, faded
    rec = edges_host(sig["NaN and inf frames"], EC.SR, both)[1]
    assert (rec["first"], rec["last"]) == (500, 900)
    rec = edges_host(sig["pads clip at both ends"], EC.SR, EC.CONFIGS["pads clip"])[1]
    assert (rec["first"], rec["last"], rec["start"], rec["end"]) == (3, EC.N - 2, 0, EC.N)
    rec = edges_host(sig["pads clip at both ends"], EC.SR, Edges(trim_db=EC.TRIM_DB, pad_ms=(0.05, 0)))[1]
    assert (rec["start"], rec["end"]) == (1, EC.N - 1)
    a, b = EC.wave_edge(channels)
    for name, want in (("last lane of a wave", (a, a)), ("first lane of the next wave", (b, b)), ("both sides of a wave", (a, b))):
        rec = edges_host(sig[name], EC.SR, both)[1]
        assert (rec["first"], rec["last"]) == want
    rec = edges_host(sig["burst n=0"], EC.SR, EC.CONFIGS["both"])[1]
    assert rec.tobytes() == bytes(64)
    if channels == 2:
        rec = edges_host(sig["sound in R only"], EC.SR, both)[1]
        assert (rec["first"], rec["last"]) == (1000, 1999)
        rec = edges_host(sig["NaN in L, sound in R"], EC.SR, both)[1]
        assert (rec["first"], rec["last"]) == (300, 309)
    # without a trim nothing is searched
    rec = edges_host(sig["all silent"], EC.SR, Edges(fade_ms=1))[1]
    assert (rec["first"], rec["last"], rec["start"], rec["end"], rec["flags"]) == (0, EC.N - 1, 0, EC.N, 0)


@pytest.mark.parametrize("channels", [1, 2])
def test_loop(channels):
    sig = dict(EC.signals(channels))
    x = sig["odd span"]
    first, last = T - 100, T + 900
    # X = 2400 > len / 2 = 500 with len = 1001
    y, rec = edges_host(x, EC.SR, EC.CONFIGS["loop"])
    assert (rec["start"], rec["end"], rec["loop"], rec["fade_in"], rec["fade_out"]) == (first, last + 1 - 500, 500, 0, 0)
    y_def, rec_def = edges_reference(x, EC.SR, EC.CONFIGS["loop"])
    assert rec_def.tobytes() == rec.tobytes()
    assert np.abs(y.astype(np.float64) - y_def.astype(np.float64)).max() <= 2.0 ** -23    # two gains, each within 2^-24, |x| <= 1
    # the loop point: the span's first frame follows the frame before the crossfaded tail, as the
    # frame after it did: y[start] = x[start] c(t0) + x[end'] c(1 - t0), t0 = 1 / (2 X'), and x[end'] follows x[end' - 1]
    s, e2 = int(rec["start"]), int(rec["end"])
    ga, gb = loop_gains("hann", 500)
    want = (x[s].astype(np.float64) * np.float64(ga[0]) + x[e2].astype(np.float64) * np.float64(gb[0])).astype(np.float32)
    assert np.array_equal(EC.bits(y[s]), EC.bits(want))
    assert gb[0] > 1.0 - 1e-5 and ga[0] < 1e-5                      # at the seam the head is the tail's next frame
    assert np.array_equal(EC.bits(y[e2 - 1]), EC.bits(x[e2 - 1]))   # the frame before the seam is untouched
    assert np.array_equal(EC.bits(y[e2:]), EC.bits(x[e2:]))         # the source frames are not written
    # a short crossfade inside a long span
    y, rec = edges_host(sig[f"burst n={EC.N}"], EC.SR, EC.CONFIGS["loop only"])
    assert (rec["start"], rec["end"], rec["loop"]) == (0, EC.N - 480, 480)


@pytest.mark.parametrize("curve", ["linear", "hann", "qsin"])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 480, 4801])
def test_gains_are_within_the_derived_bound(n, curve):
    """|g - c(t)| <= 2^-24 for every frame of a fade: one rounding to float32 of a value in
    [0, 1] (2^-25) and the routine's float64 error (csrc/edges.h, step 5)."""
    k = np.arange(n, dtype=np.float64)
    t_in, t_out = (2 * k + 1) / (2 * n), (2 * (n - k) - 1) / (2 * n)
    g_in, g_out = gains(curve, n)
    assert g_in.dtype == np.float32 and len(g_in) == len(g_out) == n
    for g, t in ((g_in, t_in), (g_out, t_out)):
        assert np.abs(g.astype(np.float64) - curve_reference(curve, t)).max() <= 2.0 ** -24
        assert (g > 0).all() and (g <= 1).all()
    assert np.array_equal(g_out, g_in[::-1])                          # the same arguments, mirrored
    assert (np.diff(g_in.astype(np.float64)) >= 0).all()
    la, lb = loop_gains(curve, n)
    assert np.abs(la.astype(np.float64) - curve_reference(curve, t_in)).max() <= 2.0 ** -24
    assert np.abs(lb.astype(np.float64) - curve_reference(curve, 1.0 - t_in)).max() <= 2.0 ** -24
    for got, ref in zip(gains(curve, n) + loop_gains(curve, n), gains_reference(curve, n) + loop_gains_reference(curve, n)):
        assert np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() <= 2.0 ** -24


def test_values_and_helpers():
    assert [frames(ms, 48000) for ms in (0, 2, 20, 0.01, 0.0104, 0.0105, 1000)] == [0, 96, 960, 0, 0, 1, 48000]
    assert frames(0.03125, 48000) == 2 and frames(5, 44100) == 221      # 1.5 rounds away from zero; 220.5 too
    assert threshold(-60.0) == np.float32(1e-3) and threshold(0.0) == 1.0 and threshold(-2000.0) == 0.0
    assert Edges() == Edges(None, "both", (0, 0), (0, 0), "hann", None)
    assert Edges(pad_ms=5, fade_ms=3).counts(48000) == (0, 240, 240, 144, 144, -1)
    assert Edges(trim_db=-60, sides="tail", pad_ms=(1, 2), loop_ms=10).counts(48000) == (2, 48, 96, 0, 0, 480)
    assert not Edges(fade_ms=5).moves_span() and Edges(trim_db=-60).moves_span() and Edges(loop_ms=5).moves_span()
    for bad in (dict(trim_db=1.0), dict(trim_db=float("nan")), dict(trim_db=float("-inf")), dict(trim_db="quiet"),
                dict(trim_db=True), dict(sides="left"), dict(pad_ms=-1), dict(pad_ms=(1, 2, 3)), dict(pad_ms=(1, float("inf"))),
                dict(fade_ms=(-1, 0)), dict(fade_ms="long"), dict(curve="cubic"), dict(loop_ms=-1.0),
                dict(loop_ms=float("nan")), dict(loop_ms=10, fade_ms=(0, 1)), dict(loop_ms=10, fade_ms=5)):
        with pytest.raises(VE):
            Edges(**bad).check()
    Edges(trim_db=-60, loop_ms=10, fade_ms=0).check()
    with pytest.raises(VE):
        edges_host(np.zeros((4, 3), np.float32), 48000, Edges())
    with pytest.raises(VE):
        edges_host(np.zeros(4, np.float32), 0, Edges())
    assert L.lib().msg_sizeof(9) == C.sizeof(L.MsgEdgesRec) == EDGES_DTYPE.itemsize == 64
    assert L.lib().msg_sizeof(10) == C.sizeof(L.MsgEdgesOpts) == 56


def test_library_value_checks():
    """msg_edges_host's own statuses, as the other passes give them."""
    lib = L.lib()
    x = np.zeros(8, dtype=np.float32)
    rec = np.zeros(1, dtype=EDGES_DTYPE)

    def call(channels=1, n=8, **kw):
        o = dict(trim_db=-60.0, sides=3, curve=1, pre=0, post=0, fade_in=0, fade_out=0, loop=-1)
        o.update(kw)
        opts = L.MsgEdgesOpts(o["trim_db"], o["sides"], o["curve"], o["pre"], o["post"], o["fade_in"], o["fade_out"], o["loop"])
        return lib.msg_edges_host(x.ctypes.data_as(C.c_void_p), channels, n, C.byref(opts), rec.ctypes.data_as(C.c_void_p))

    assert call() == L.MSG_OK
    assert call(loop=-7) == L.MSG_OK and call(sides=0, trim_db=float("nan")) == L.MSG_OK
    for kw in (dict(channels=3), dict(sides=4), dict(sides=-1), dict(trim_db=0.5), dict(trim_db=float("nan")),
               dict(trim_db=float("-inf")), dict(curve=3), dict(curve=-1), dict(pre=-1), dict(post=-1), dict(fade_in=-1),
               dict(fade_out=1 << 40), dict(loop=1 << 40), dict(loop=0, fade_in=1), dict(loop=4, fade_out=1)):
        assert call(**kw) == L.MSG_E_VALUE, kw
        assert lib.msg_last_error(None)
    assert call(n=-1) == L.MSG_E_ARG
    assert lib.msg_edges_host(None, 1, 8, None, rec.ctypes.data_as(C.c_void_p)) == L.MSG_E_ARG


@pytest.mark.parametrize("prefix", ["out_", "export_"])
def test_delivery_rules(prefix):
    import dataclasses

    from msgpu.export import Delivery
    e = Edges(trim_db=-60, pad_ms=5, fade_ms=(2, 20))
    d = Delivery(48000, None, -23.0, None, -1.0, 16, edges=e)
    assert d.edges is e and Delivery().edges is None
    d.check(prefix)
    Delivery(edges=e).check(prefix)                             # needs no other rule
    Delivery(edges=None).check(prefix, "stats")
    for bad in ("trim", -60, dict(trim_db=-60), True):
        with pytest.raises(VE, match=f"{prefix}edges must be None or an Edges"):
            Delivery(edges=bad).check(prefix)
    for bad, word in ((Edges(trim_db=3), "trim_db"), (Edges(sides="left"), "sides"), (Edges(pad_ms=-1), "pad_ms"),
                      (Edges(fade_ms=(1, 2, 3)), "fade_ms"), (Edges(curve="cubic"), "curve"), (Edges(loop_ms=-2), "loop_ms"),
                      (Edges(loop_ms=10, fade_ms=5), "loop_ms and fade_ms")):
        with pytest.raises(VE, match=f"{prefix}edges: .*{word}"):
            Delivery(edges=bad).check(prefix)
    with pytest.raises(VE, match=f"{prefix}edges applies to results"):
        Delivery(edges=e).check(prefix, "stats")
    with pytest.raises(NIE, match=f"{prefix}edges on more than one device"):
        Delivery(edges=e).check(prefix, n_devices=2)
    with pytest.raises(NIE, match=f"{prefix}edges on more than one device"):
        Delivery(edges=e).one_device(prefix, 2, companions=True)
    Delivery(edges=None).one_device(prefix, 2, companions=True)
    # the rule is a field after the first ten: every positional caller stays as it was
    names = [f.name for f in dataclasses.fields(Delivery) if f.init]
    assert names[9] == "report" and names[10:] == ["shape", "edges"]
    # and equality sees it: two deliveries that differ only in their edges are two deliveries
    assert d != Delivery(48000, None, -23.0, None, -1.0, 16) and d == Delivery(48000, None, -23.0, None, -1.0, 16, edges=e)
    assert d != dataclasses.replace(d, edges=Edges(trim_db=-50, pad_ms=5, fade_ms=(2, 20)))


def test_front_ends_refuse_before_any_device_call():
    import inspect

    from msgpu import batch, dropin
    p = dict(msgpu.DEFAULTS)
    e = Edges(trim_db=-60)
    with pytest.raises(VE, match="out_edges: .*curve"):
        msgpu.render_batch([p], out_edges=Edges(curve="cubic"))
    with pytest.raises(VE, match="export_edges must be None or an Edges"):
        msgpu.render_variations(p, [1000], [1.0], [1.0], export_edges="trim")
    with pytest.raises(NIE, match="out_edges on more than one device"):
        msgpu.render_batch([p], devices=[0, 1], out_edges=e)
    with pytest.raises(NIE, match="export_edges on more than one device"):
        msgpu.render_variations(p, [1000], [1.0], [1.0], devices=[0, 1], export_edges=e)
    with pytest.raises(VE, match="out_edges applies to results"):
        msgpu.render_batch([p], results="stats", out_edges=e)
    # the new keywords go last
    assert list(inspect.signature(dropin.render_batch).parameters)[-1] == "out_edges"
    assert list(inspect.signature(msgpu.render_batch).parameters)[-1] == "out_edges"
    assert list(inspect.signature(batch.render_variations).parameters)[-1] == "export_edges"
