"""The delivery rules of render_batch(out_...) and render_variations(export_...): one table of
option combinations (msgpu/export.py, Delivery.check), each refused with the exception class
it always had, before any device call (no GPU here)."""
import pytest

import msgpu

VE, NIE = ValueError, NotImplementedError

# (options without their prefix, extra keywords of the call, the class raised)
RULES = [
    ({"peak": "preset"}, {}, VE),                                   # peak without sr
    ({"sr": 48000, "peak": "preset", "lufs": -23.0}, {}, VE),       # two level rules
    ({"sr": 48000, "peak": "preset", "true_peak": -1.0}, {}, VE),
    ({"ceiling": 0.9}, {}, VE),                                     # a ceiling needs a level rule
    ({"bits": 20}, {}, VE),
    ({"bits": 16, "dither": "shaped"}, {}, VE),
] + [({k: v}, {"devices": [0, 1]}, NIE) for k, v in (("sr", 48000), ("lufs", -23.0), ("true_peak", -1.0), ("bits", 16))]
STATS = [({k: v}, {"results": "stats"}, VE) for k, v in (("sr", 48000), ("lufs", -23.0), ("true_peak", -1.0), ("bits", 16))]


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


def test_both_front_ends_word_one_table():
    """The messages carry the caller's prefix; the table itself is held once."""
    from msgpu.export import Delivery
    for prefix in ("out_", "export_"):
        with pytest.raises(VE, match=f"{prefix}lufs and {prefix}peak are two"):
            Delivery(sr=48000, peak="preset", lufs=-23.0).check(prefix)
        with pytest.raises(NIE, match=f"{prefix}true_peak on more than one"):
            Delivery(true_peak=-1.0, ceiling=0.9).check(prefix, n_devices=2)
    with pytest.raises(NIE, match="out_lufs on more than one"):         # render_batch: the companion asks too
        Delivery(true_peak=-1.0, ceiling=0.9).one_device("out_", 2, companions=True)
    with pytest.raises(VE):
        Delivery().check("out_", None)                                  # no result kind is no default
    with pytest.raises(VE):
        Delivery(sr=48000, peak=0.5).check("export_", numeric_peak=False)
    Delivery(sr=48000, peak=0.5).check("out_")
    Delivery().check("out_", "stats", n_devices=8)                      # nothing asked for: nothing refused
    Delivery(sr=48000, lufs=-23.0, ceiling=0.9, true_peak=-1.0, bits=24).check("export_")
