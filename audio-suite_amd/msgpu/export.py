"""The delivery chain of a rendered batch: resample -> filter -> stereo -> gate -> dynamics -> edges -> level -> report -> quantise -> FLAC, in HBM.

``render_batch`` (dropin.py, ``out_*`` options) and ``render_variations`` (batch.py,
``export_*`` options) describe what they deliver with one ``Delivery``, check it with
``Delivery.check`` and run it with ``deliver``; each pass works on the renders where
they lie (resample.py, filter.py, stereo.py, gate.py, dynamics.py, edges.py, loudness.py, truepeak.py, limit.py, lrange.py, pcm.py) and nothing
here synchronises, with one exception: an ``edges`` rule with a trim or a loop crossfade changes what
is delivered of each render, so ``deliver`` reads the spans the device found (8 int64 per render)
before it sizes the later passes.  That is the chain's one host wait; fades alone wait for nothing.
A ``flac`` rule is the second: the encoded lengths are only known on the device, so ``deliver`` reads
the FLAC records (11 int64 per render) and the front end then copies exactly the encoded bytes.
A new export rule is a field of ``Delivery`` (after the last one, so the positional order stays),
its row in ``RULES``, its lines in ``check`` and its step in ``deliver``; a pass that runs at the
renders' rates is a closure handed to ``per_rate``.  The twelve dataclass fields and their order
are pinned by the earlier rules' tests, so ``filter``, the rule after ``edges``, is a keyword of
``Delivery`` and no dataclass field: ``Delivery(filter=f)``, seen by ``==`` and ``repr``; so is
``stereo``, the rule between them in the chain, ``dynamics``, the compressor between the stereo
rule and the edges, ``gate``, the gate between the stereo rule and the compressor, and ``flac``, the
FLAC encoder after the quantiser.  From the stereo step on a render has one channel or
two: ``deliver`` carries that count through every later pass, each of which takes it as a keyword
that defaults to 2.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# one row of a delivery report: the meters of a render as it is delivered (report_packed)
REPORT_DTYPE = np.dtype([(k, "<f8") for k in ("lufs", "lra", "lo", "hi", "max_momentary", "max_short", "peak",
                                              "true_peak", "dbtp")] + [("frames", "<i8"), ("rate", "<i8")])

# The rules, each a field of Delivery (``filter``, ``stereo``, ``dynamics``, ``gate``, ``flac``: its keywords): (the rule, the option that comes with it, why it works on one
# device only, whether results "stats" may ask for it).  ``dither``, ``dither_seed`` and ``shape`` are
# options of ``bits`` that ask for nothing alone, so they have no row.
RULES = (("sr", "peak", " (multi.py sizes its shared memory by out_n)", False), ("lufs", "ceiling", "", False),
         ("true_peak", None, "", False), ("bits", None, "", False), ("limiter", None, "", False),
         ("report", None, "", False), ("flac", None, "", False), ("gate", None, "", False), ("dynamics", None, "", False), ("stereo", None, "", False), ("edges", None, "", False),
         ("filter", None, "", False))


@dataclass
class DeliveryFields:
    sr: object = None             # deliver at this rate (None: as rendered)
    peak: object = None           # the peak resampled renders are rescaled to: None, "preset" or a number
    lufs: object = None           # BS.1770 integrated loudness to deliver at
    ceiling: object = None        # linear sample peak the levelled renders may not exceed
    true_peak: object = None      # ceiling in dBTP
    bits: object = None           # 16 or 24: fixed-point PCM, quantised last
    dither: object = "tpdf"
    dither_seed: int = 0
    limiter: object = None        # hold true_peak with the look-ahead limiter: None off, True 5 ms, a number of ms
    report: object = None         # a list that gets one REPORT_DTYPE row per render, measured on what is delivered
    shape: object = None          # noise-shaped dither for ``bits``: None, "e3", "lipshitz5" or "f9"
    edges: object = None          # silence trim, fades or loop crossfade before the level rules: an edges.Edges
    _pending: list = field(default_factory=list, init=False, repr=False, compare=False)   # deliver's unread reports

    def flush_report(self):
        """Read the reports ``deliver`` left on the device into ``report``, in render order;
        the caller has waited for the renders' copy, so this waits for nothing new."""
        for pending in self._pending:
            sink = getattr(pending, "sink", None)             # a stereo rule's meter rows go to its own list
            (self.report if sink is None else sink).extend(pending.rows())
        self._pending.clear()

    def limiter_ms(self):
        """The limiter's look-ahead in milliseconds, None when it is off; ValueError for
        anything but None, True or a finite positive number."""
        v = self.limiter
        if v is None:
            return None
        if v is True:
            return 5.0
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                not np.isfinite(float(v)) or not float(v) > 0.0:
            raise ValueError("the limiter is None, True or a positive number of milliseconds")
        return float(v)

    def one_device(self, prefix, n_devices, rules=tuple(r[0] for r in RULES), companions=False):
        """NotImplementedError for the first of ``rules`` asked for on more than one device;
        ``companions``: a rule's companion option alone asks for it too (render_batch, which
        looks at the device count before it looks at the values)."""
        if n_devices > 1:
            for rule, companion, why, _ in RULES:
                asked = getattr(self, rule) is not None or (companions and companion and
                                                            getattr(self, companion) is not None)
                if rule in rules and asked:
                    raise NotImplementedError(f"{prefix}{rule} on more than one device{why}")

    def check(self, prefix, results="audio", n_devices=1, numeric_peak=True, rates=()):
        """The rules' checks, worded with the caller's option prefix ("out_" or "export_"); their
        order decides which exception wins, so a new rule's lines go last, before "stats".
        ``results``: the result kind delivered; ``numeric_peak``: whether ``peak`` may be a
        number (render_variations has one template preset and takes None or "preset");
        ``rates``: the rates the renders are made at, for the rules that meter the delivered rate.
        Runs before any device call."""
        p = prefix
        if results not in ("audio", "stats", "device"):
            raise ValueError("results must be 'audio', 'stats' or 'device'")
        if self.sr is None and self.peak is not None:
            raise ValueError(f"{p}peak needs {p}sr")
        if not numeric_peak and self.peak not in (None, "preset"):
            raise ValueError(f"{p}peak must be None or 'preset'")
        for rule in ("lufs", "true_peak"):
            if getattr(self, rule) is not None and self.peak is not None:
                raise ValueError(f"{p}{rule} and {p}peak are two level rules: give one")
        if self.lufs is None and self.true_peak is None and self.ceiling is not None:
            raise ValueError(f"{p}ceiling needs {p}lufs")
        self.one_device(p, n_devices, ("sr", "lufs", "true_peak"))
        if self.bits is not None:
            from .pcm import check_bits, dither_code
            check_bits(self.bits)
            dither_code(self.dither)
        if self.shape is not None:
            from .pcm import shape_code
            if self.bits is None:
                raise ValueError(f"{p}shape needs {p}bits")
            try:
                shape_code(self.shape)
            except ValueError:
                raise ValueError(f"{p}shape must be None, 'e3', 'lipshitz5' or 'f9'") from None
        self.one_device(p, n_devices, ("bits",))
        if self.limiter is not None:
            try:
                self.limiter_ms()
            except ValueError:
                raise ValueError(f"{p}limiter must be None, True or a positive number of milliseconds") from None
            if self.true_peak is None:
                raise ValueError(f"{p}limiter needs {p}true_peak")
        self.one_device(p, n_devices, ("limiter",))
        if self.report is not None:
            from .loudness import _check_rate
            if not isinstance(self.report, list):
                raise ValueError(f"{p}report must be None or a list")
            for rate in ([self.sr] if self.sr is not None else rates):
                try:
                    _check_rate(rate)
                except ValueError:
                    raise ValueError(f"{p}report meters rates that are multiples of 10, at least 4000") from None
        self.one_device(p, n_devices, ("report",))
        if self.edges is not None:
            from .edges import Edges
            if not isinstance(self.edges, Edges):
                raise ValueError(f"{p}edges must be None or an Edges")
            try:
                self.edges.check()
            except ValueError as e:
                raise ValueError(f"{p}edges: {e}") from None
        self.one_device(p, n_devices, ("edges",))
        if self.filter is not None:
            from .filter import Filter
            if not isinstance(self.filter, Filter):
                raise ValueError(f"{p}filter must be None or a Filter")
            try:
                self.filter.check()
                for rate in ([self.sr] if self.sr is not None else rates):
                    self.filter.check(rate)
            except ValueError as e:
                raise ValueError(f"{p}filter: {e}") from None
        self.one_device(p, n_devices, ("filter",))
        if self.stereo is not None:
            from .loudness import _check_rate
            from .stereo import Stereo
            if not isinstance(self.stereo, Stereo):
                raise ValueError(f"{p}stereo must be None or a Stereo")
            try:
                self.stereo.check()
            except ValueError as e:
                raise ValueError(f"{p}stereo: {e}") from None
            for rate in ([self.sr] if self.sr is not None else rates) if self.stereo.metering() else ():
                try:
                    _check_rate(rate)
                except ValueError:
                    raise ValueError(f"{p}stereo meters rates that are multiples of 10, at least 4000") from None
        self.one_device(p, n_devices, ("stereo",))
        if self.dynamics is not None:
            from .dynamics import Dynamics
            if not isinstance(self.dynamics, Dynamics):
                raise ValueError(f"{p}dynamics must be None or a Dynamics")
            try:
                self.dynamics.check()
                for rate in ([self.sr] if self.sr is not None else rates):
                    self.dynamics.check(rate)
            except ValueError as e:
                raise ValueError(f"{p}dynamics: {e}") from None
        self.one_device(p, n_devices, ("dynamics",))
        if self.gate is not None:
            from .gate import Gate
            if not isinstance(self.gate, Gate):
                raise ValueError(f"{p}gate must be None or a Gate")
            try:
                self.gate.check()
                for rate in ([self.sr] if self.sr is not None else rates):
                    self.gate.check(rate)
            except ValueError as e:
                raise ValueError(f"{p}gate: {e}") from None
        self.one_device(p, n_devices, ("gate",))
        if self.flac is not None:
            from .flac import Flac
            if not isinstance(self.flac, Flac):
                raise ValueError(f"{p}flac must be None or a Flac")
            if self.bits is None:
                raise ValueError(f"{p}flac needs {p}bits")
            try:
                self.flac.check()
                for rate in ([self.sr] if self.sr is not None else rates):
                    self.flac.check(rate)
            except ValueError as e:
                raise ValueError(f"{p}flac: {e}") from None
        self.one_device(p, n_devices, ("flac",))
        if results == "stats":
            for rule, _, _, with_stats in RULES:
                if not with_stats and getattr(self, rule) is not None:
                    raise ValueError(f"{p}{rule} applies to results 'audio' or 'device'")


class Delivery(DeliveryFields):
    """What a front end delivers: DeliveryFields' rules, given as they always were, and after them
    ``filter``, a filter.Filter whose biquad cascade runs in front of the edges and the level rules,
    and ``stereo``, a stereo.Stereo whose meter, image matrix or mono fold runs between the filter and
    the edges, and ``dynamics``, a dynamics.Dynamics whose compressor runs between the stereo rule and
    the edges, and ``gate``, a gate.Gate whose gate runs between the stereo rule and the compressor, and ``flac``, a
    flac.Flac that encodes what the quantiser packed as FLAC frames.  They are given by keyword only and are not dataclass fields (``dataclasses.fields``
    and ``dataclasses.replace`` do not see them; ``==`` and ``repr`` do)."""
    filter = None
    stereo = None
    dynamics = None
    gate = None
    flac = None

    def __init__(self, *args, filter=None, stereo=None, dynamics=None, gate=None, flac=None, **kw):
        super().__init__(*args, **kw)
        self.filter = filter
        self.stereo = stereo
        self.dynamics = dynamics
        self.gate = gate
        self.flac = flac

    def __eq__(self, other):
        same = DeliveryFields.__eq__(self, other)
        if same is NotImplemented:
            return same
        return same and self.filter == other.filter and self.stereo == other.stereo and self.dynamics == other.dynamics \
            and self.gate == other.gate and self.flac == other.flac

    __hash__ = None

    def __repr__(self):
        return DeliveryFields.__repr__(self)[:-1] + \
            f", flac={self.flac!r}, gate={self.gate!r}, dynamics={self.dynamics!r}, filter={self.filter!r}, stereo={self.stereo!r})"

    def channels(self):
        """The channels of what is delivered: 1 when the stereo rule folds to mono, else 2."""
        return 1 if self.stereo is not None and self.stereo.channels == 1 else 2


def deliver(eng, out, offsets, lens, rates, delivery, peaks=None, keys=None):
    """Run ``delivery`` over renders lying in a device tensor ((frames, 2) float32, render i
    at frame offsets[i] with lens[i] frames at rates[i] Hz): resampled to ``delivery.sr``
    (``peaks``: resample_packed's), filtered by ``delivery.filter`` (filter_packed: in front of the edges, so
    that a trim sees the filtered signal and the fades still end at zero, and in front of the level rules, so
    that loudness, true peak, limiter and report measure what is delivered), metered, shaped or folded
    to mono by ``delivery.stereo`` (stereo_packed: after the filter, because DC and rumble are correlation,
    and in front of the edges and the level rules, because a fold changes the level they must see; from there
    on a render has ``delivery.channels()`` channels, (frames, 1) when folded), gated by ``delivery.gate`` (gate_packed:
    in front of the compressor, whose makeup then cannot lift what the gate removed and so that the thresholds mean the
    rendered level, and in front of the edges, so that a trim sees the gated tail), compressed by ``delivery.dynamics``
    (dynamics_packed: the fold is compressed as delivered; in front of the edges, so that a trim sees the
    compressed level and the fades still end at zero, and in front of the level rules), its ends shaped by ``delivery.edges`` (edges_packed; from there
    on a render is the span that rule left of it), levelled at the rate delivered, metered as delivered when
    ``delivery.report`` is a list (report_packed; ``delivery.flush_report`` reads the rows once
    the caller has waited for its copy), quantised with the dither streams
    (``delivery.dither_seed``, keys[i]).  Returns (tensor, offsets, lens,
    rec): the float32 renders with frame offsets and lengths and None, or, quantised, the
    packed bytes with byte offsets and lengths and the device PCM records.  Enqueued on
    the current stream; no host synchronise, but for the spans of an ``edges`` rule that trims or
    loops (the module's docstring).  With ``delivery.flac`` the packed bytes are encoded where they lie
    (flac_packed) and what comes back is the frames' bytes, each render's byte offset and byte count in
    them as the device's records give them, and a FlacDelivery with the PCM records (device) and the
    FLAC records (host): reading those is the chain's second host wait."""
    d = delivery
    if d.sr is not None:
        out, offsets, lens = resample_packed(eng, out, offsets, lens, rates, int(d.sr), peaks)
        rates = [int(d.sr)] * len(lens)
    if d.filter is not None:
        filter_packed(eng, out, offsets, lens, rates, d.filter)
    ch = 2
    if d.stereo is not None:
        out, offsets, ch = stereo_packed(eng, out, offsets, lens, rates, d.stereo, pending=d._pending)
    if d.gate is not None:
        gate_packed(eng, out, offsets, lens, rates, d.gate, channels=ch)
    if d.dynamics is not None:
        dynamics_packed(eng, out, offsets, lens, rates, d.dynamics, channels=ch)
    if d.edges is not None:
        offsets, lens, _ = edges_packed(eng, out, offsets, lens, rates, d.edges, channels=ch)
    _level(eng, out, offsets, lens, rates, d.lufs, d.ceiling, d.true_peak, d.limiter_ms(), channels=ch)
    if d.report is not None:
        d._pending.append(report_packed(eng, out, offsets, lens, rates, channels=ch))
    if d.bits is None:
        return out, offsets, lens, None
    q = quantize_packed(eng, out, offsets, lens, d.bits, d.dither, d.dither_seed, keys, d.shape, channels=ch)
    if d.flac is None:
        return q
    frames, rec = flac_packed(eng, q[0], q[1], lens, rates, d.flac, d.bits, channels=ch)
    return frames, rec["byte_off"].copy(), rec["bytes"].copy(), FlacDelivery(q[3], rec, rates, ch, d.bits, d.flac.block)


def _extents(offsets, lens, rates):
    return np.asarray(offsets, dtype=np.int64), np.asarray(lens, dtype=np.int64), [int(s) for s in rates]


def rate_groups(rates):
    """[(rate, the indices of its renders)], in ascending rate order."""
    return [(rate, [i for i, s in enumerate(rates) if s == rate]) for rate in sorted(set(rates))]


def per_rate(eng, y, offsets, lens, rates, pass_, cols, dtype=None):
    """The one loop over rates: ``pass_(offsets, lens, rate)`` over the renders of each distinct
    rate, in ascending rate order.  It enqueues the rate's library calls and returns their device
    records, one tensor of ``cols`` columns or, ``cols`` a tuple, a tuple of them (``dtype``:
    float64 when None); returns them in render order on y's device.  One rate: the pass's own
    tensors, nothing allocated or scattered; no render: empty ones, the pass not called."""
    torch = eng.torch
    offsets, lens, rates = _extents(offsets, lens, rates)
    groups = rate_groups(rates)
    if len(groups) == 1:
        return pass_(offsets, lens, groups[0][0])
    many = isinstance(cols, tuple)
    recs = [torch.empty((len(rates), w), dtype=dtype or torch.float64, device=y.device) for w in (cols if many else (cols,))]
    for rate, idx in groups:
        got = pass_(offsets[idx], lens[idx], rate)
        at = torch.as_tensor(idx, device=y.device)
        for rec, r in zip(recs, got if many else (got,)):
            rec[at] = r
    return tuple(recs) if many else recs[0]


def resample_packed(eng, out, offsets, lens, sr_in, out_sr, peaks=None):
    """Resample renders lying in a device output tensor ((frames, 2) float32, render i
    at frame offsets[i] with lens[i] frames at sr_in[i] Hz) to out_sr where they lie
    (msg_resample, one call per distinct input rate): returns (y, y_offsets, y_lens),
    the outputs packed back to back in render order, enqueued on the current stream.
    ``peaks`` (one per render, or None): rescale each resampled render so that
    max|y| equals its peak, peak_normalize's rule (MS:26-29: a zero buffer stays
    zero) -- resampling moves the peak.  Renders of one length are rescaled by one
    reduction and one multiply over the batch."""
    from .resample import design, ratio, resample_len
    torch = eng.torch
    offsets, lens, rates = _extents(offsets, lens, sr_in)
    ratios = [ratio(s, out_sr) for s in rates]
    y_lens = np.array([resample_len(n, u, d) for n, (u, d) in zip(lens, ratios)], dtype=np.int64)
    y_off = np.concatenate([[0], np.cumsum(y_lens)[:-1]]).astype(np.int64)
    y = torch.empty((int(y_lens.sum()), 2), dtype=torch.float32, device=out.device)
    for rate, idx in rate_groups(rates):
        up, down = ratio(rate, out_sr)
        h = design(up, down) if up != down else None
        if len(idx) == len(rates):            # one rate: the whole batch in one call
            eng.resample(out, offsets, lens, 2, up, down, h, out=y)
        else:                                 # mixed rates: Engine.resample packs a call's outputs back to back
            for i in idx:
                eng.resample(out, offsets[i:i + 1], lens[i:i + 1], 2, up, down, h, out=y[int(y_off[i]):])
    if peaks is not None and len(y_lens):
        pk = torch.tensor([float(p) for p in peaks], dtype=torch.float32, device=y.device)
        if len(set(int(n) for n in y_lens)) == 1:
            v = y.view(len(y_lens), -1)
            m = v.abs().amax(dim=1)
            v.mul_(torch.where(m > 0, pk / m, torch.ones_like(m)).unsqueeze(1))
        else:
            for i, (o, n) in enumerate(zip(y_off, y_lens)):
                seg = y[int(o):int(o) + int(n)]
                m = seg.abs().amax() if n else pk[i]
                seg.mul_(torch.where(m > 0, pk[i] / m, torch.ones_like(m)))
    return y, y_off, y_lens


def edges_packed(eng, y, offsets, lens, rates, edges, channels=2):
    """Shape the ends of renders lying in a device tensor ((frames, ``channels``) float32, render i at frame
    offsets[i] with lens[i] frames at rates[i] Hz) where they lie: msg_edges per distinct rate
    (edges.py: the milliseconds of ``edges`` are frames at the render's rate).  Nothing is
    moved.  Returns (offsets, lens, rec): where each render's delivered span lies, and the
    device records in render order (engine.Engine.edges).  With a trim or a loop crossfade
    the spans are read from the device, 8 int64 per render: the one host wait; otherwise the
    extents come back as they were and nothing waits."""
    from .edges import records
    offsets, lens, rates = _extents(offsets, lens, rates)
    rec = per_rate(eng, y, offsets, lens, rates, lambda off, cnt, rate: eng.edges(y, off, cnt, channels, rate, edges), 8,
                   eng.torch.int64)
    if not edges.moves_span() or not len(rates):
        return offsets, lens, rec
    spans = records(rec)
    return offsets + spans["start"], spans["end"] - spans["start"], rec


def filter_packed(eng, y, offsets, lens, rates, flt):
    """Run renders lying in a device tensor ((frames, 2) float32, render i at frame offsets[i] with
    lens[i] frames at rates[i] Hz) through the cascade of ``flt``, a filter.Filter, where they lie:
    msg_filter per distinct rate (the design depends on the rate), twice for a zero-phase filter.
    Nothing is moved and there is no record; no host synchronise."""
    def run(off, cnt, rate):
        eng.filter(y, off, cnt, 2, rate, flt)
        return ()
    per_rate(eng, y, offsets, lens, rates, run, ())


def gate_packed(eng, y, offsets, lens, rates, gate, channels=2):
    """Gate renders lying in a device tensor ((frames, ``channels``) float32, render i at frame
    offsets[i] with lens[i] frames at rates[i] Hz) with ``gate``, a gate.Gate, where they lie:
    msg_gate_apply per distinct rate (the milliseconds are steps and frames at the render's rate).
    Nothing is moved.  Returns the device records in render order (engine.Engine.gate_apply); no
    host synchronise."""
    return per_rate(eng, y, offsets, lens, rates, lambda off, cnt, rate: eng.gate_apply(y, off, cnt, channels, rate, gate), 6,
                    eng.torch.int64)


def dynamics_packed(eng, y, offsets, lens, rates, dyn, channels=2):
    """Compress renders lying in a device tensor ((frames, ``channels``) float32, render i at frame
    offsets[i] with lens[i] frames at rates[i] Hz) with ``dyn``, a dynamics.Dynamics, where they lie:
    msg_dynamics per distinct rate (the milliseconds are steps and frames at the render's rate).
    Nothing is moved.  Returns the device records in render order (engine.Engine.dynamics); no host
    synchronise."""
    return per_rate(eng, y, offsets, lens, rates, lambda off, cnt, rate: eng.dynamics(y, off, cnt, channels, rate, dyn), 4,
                    eng.torch.int64)


class MeterRows:
    """The device records of one stereo_packed call's meter, in render order, and the list they are
    for; ``rows`` copies them to the host with the derived columns (it waits for them)."""

    def __init__(self, rec, sink):
        self.rec, self.sink = rec, sink

    def rows(self):
        from .stereo import records
        return records(self.rec)


def stereo_packed(eng, y, offsets, lens, rates, stereo, pending=None):
    """Meter, shape or fold renders lying in a device tensor ((frames, 2) float32, render i at frame
    offsets[i] with lens[i] frames at rates[i] Hz) with ``stereo``, a stereo.Stereo.  It meters first,
    msg_stereo_meter per distinct rate (the blocks are 400 ms at the render's rate), when
    ``stereo.meter`` is a list or ``stereo.invert == "auto"``; then one msg_stereo call applies the
    image to every render, the polarity of each taken from its record on the device.  Returns
    (buffer, offsets, channels): y shaped in place with the offsets as they were and 2, or a new
    (frames, 1) tensor with the folded renders back to back, their offsets and 1.  The meter's rows:
    with ``pending`` (a list, ``Delivery._pending``) a MeterRows is left there and nothing waits;
    without it they are read into ``stereo.meter`` here, the one host wait."""
    offsets, lens, rates = _extents(offsets, lens, rates)
    rec = None
    if stereo.metering():
        rec = per_rate(eng, y, offsets, lens, rates, lambda off, cnt, rate: eng.stereo_meter(y, off, cnt, rate), 8)
        if stereo.meter is not None:
            rows = MeterRows(rec, stereo.meter)
            if pending is None:
                stereo.meter.extend(rows.rows())
            else:
                pending.append(rows)
    out, out_off = eng.stereo(y, offsets, lens, stereo, rec=rec if stereo.invert == "auto" else None)
    return out, out_off, stereo.channels


def loudness_packed(eng, y, offsets, lens, rates, target_lufs, ceiling=None, true_peak=None, channels=2):
    """Bring renders lying in a device tensor ((frames, ``channels``) float32, render i at frame
    offsets[i] with lens[i] frames at rates[i] Hz) to ``target_lufs`` where they lie:
    msg_loudness then msg_loudness_gain per distinct rate, the gain formed on the
    device from each render's record (no host synchronise).  ``ceiling``: a linear
    sample peak no render may exceed (None: no limit).  ``true_peak``: a ceiling in
    dBTP (BS.1770 true peak, truepeak.py) no render may exceed: msg_truepeak is
    measured too and msg_truepeak_gain forms the one gain from both records.  Scales y
    in place and returns the device records in render order (engine.Engine.loudness)."""
    def level(off, cnt, rate):
        r = eng.loudness(y, off, cnt, channels, rate)
        if true_peak is None:
            eng.loudness_gain(y, off, cnt, channels, r, float(target_lufs), ceiling)
        else:
            t = eng.true_peak(y, off, cnt, channels, rate)
            eng.true_peak_gain(y, off, cnt, channels, t, r, float(target_lufs), _dbtp(true_peak), ceiling)
        return r
    return per_rate(eng, y, offsets, lens, rates, level, 5)


def _dbtp(true_peak):
    """A dBTP ceiling as a linear true peak."""
    v = float(true_peak)
    if not np.isfinite(v):
        raise ValueError("the true-peak ceiling must be a number of dBTP")
    return 10.0 ** (v / 20.0)


def truepeak_packed(eng, y, offsets, lens, rates, true_peak, ceiling=None, channels=2):
    """Hold renders lying in a device tensor (as loudness_packed) under ``true_peak`` dBTP
    where they lie, with no loudness target: msg_truepeak then msg_truepeak_gain per
    distinct rate, the gain (1 where the ceiling does not bind) formed on the device.
    ``ceiling``: a linear sample peak as well (None: no limit).  Scales y in place and
    returns the device records in render order (engine.Engine.true_peak)."""
    def level(off, cnt, rate):
        t = eng.true_peak(y, off, cnt, channels, rate)
        eng.true_peak_gain(y, off, cnt, channels, t, None, None, _dbtp(true_peak), ceiling)
        return t
    return per_rate(eng, y, offsets, lens, rates, level, 5)


def limiter_packed(eng, y, offsets, lens, rates, true_peak, lookahead_ms, lufs=None, ceiling=None, channels=2):
    """Hold renders lying in a device tensor (as loudness_packed) under ``true_peak`` dBTP with
    the look-ahead limiter instead of one static gain, per distinct rate: levelled to
    ``lufs`` first when given (msg_loudness, msg_loudness_gain with no ceiling), then
    msg_truepeak and msg_limit (a render measured under the ceiling is skipped on the
    device), then msg_truepeak again and msg_truepeak_gain as a static trim, which is 1
    wherever the limiter was enough and also holds ``ceiling``, the linear sample peak.
    Works in place and returns the limiter's device records in render order
    (engine.Engine.limit); no host synchronise."""
    from .limit import lookahead_frames
    c = _dbtp(true_peak)

    def level(off, cnt, rate):
        if lufs is not None:
            r = eng.loudness(y, off, cnt, channels, rate)
            eng.loudness_gain(y, off, cnt, channels, r, float(lufs), None)
        t = eng.true_peak(y, off, cnt, channels, rate)
        lim = eng.limit(y, off, cnt, channels, rate, c, lookahead_frames(rate, lookahead_ms), tp_rec=t)
        t2 = eng.true_peak(y, off, cnt, channels, rate)
        eng.true_peak_gain(y, off, cnt, channels, t2, None, None, c, ceiling)
        return lim
    return per_rate(eng, y, offsets, lens, rates, level, 4)


def _level(eng, y, offsets, lens, rates, lufs, ceiling, true_peak, limiter_ms=None, channels=2):
    if limiter_ms is not None:
        limiter_packed(eng, y, offsets, lens, rates, true_peak, limiter_ms, lufs, ceiling, channels)
    elif lufs is not None:
        loudness_packed(eng, y, offsets, lens, rates, lufs, ceiling, true_peak, channels)
    elif true_peak is not None:
        truepeak_packed(eng, y, offsets, lens, rates, true_peak, ceiling, channels)


class Report:
    """The device records of one report_packed call, in render order; ``rows`` copies them to
    the host as a REPORT_DTYPE array (it waits for them)."""

    def __init__(self, loud, rng, tp, lens, rates):
        self.loud, self.rng, self.tp = loud, rng, tp
        self.lens, self.rates = np.asarray(lens, dtype=np.int64), np.asarray(rates, dtype=np.int64)

    def rows(self):
        from .loudness import records as loud_records
        from .lrange import records as range_records
        from .truepeak import records as tp_records
        out = np.zeros(len(self.lens), dtype=REPORT_DTYPE)
        if not len(out):
            return out
        loud, rng, tp = loud_records(self.loud), range_records(self.rng), tp_records(self.tp)
        out["lufs"] = loud["lufs"]
        for k in ("lra", "lo", "hi", "max_momentary", "max_short"):
            out[k] = rng[k]
        for k in ("peak", "true_peak", "dbtp"):
            out[k] = tp[k]
        out["frames"], out["rate"] = self.lens, self.rates
        return out


def report_packed(eng, y, offsets, lens, rates, channels=2):
    """The delivery meters of renders lying in a device tensor (as loudness_packed), as they are
    delivered: per distinct rate one msg_loudness_range call (integrated loudness, loudness
    range, maximum momentary and short-term loudness) and msg_truepeak (sample peak, true
    peak, dBTP).  Changes no sample; returns a Report, no host synchronise."""
    def meter(off, cnt, rate):
        return eng.loudness_range(y, off, cnt, channels, rate) + (eng.true_peak(y, off, cnt, channels, rate),)
    return Report(*per_rate(eng, y, offsets, lens, rates, meter, (5, 12, 5)), lens, rates)


def write_report_csv(path, names, rows):
    """``rows`` (REPORT_DTYPE) as a CSV with a header, one line per file name."""
    import csv
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["file"] + list(REPORT_DTYPE.names))
        for name, row in zip(names, rows):
            w.writerow([name] + [repr(row[k].item()) for k in REPORT_DTYPE.names])


def quantize_packed(eng, y, offsets, lens, bits, dither="tpdf", seed=0, keys=None, shape=None, channels=2):
    """Renders lying in a device tensor (as loudness_packed) as ``bits``-bit PCM, quantised
    and packed on the device after every level rule (msg_quantize, pcm.py): render i
    takes its dither from the stream (seed, keys[i]); ``shape``: noise-shaped dither
    (msg_quantize_shaped).  Returns the device byte tensor,
    each render's byte offset and length in it, and the device records (no host synchronise)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    out, byte_off, rec = eng.quantize(y, offsets, lens, channels, bits, dither, seed, keys, shape=shape)
    return out, byte_off, lens * (int(channels) * (int(bits) // 8)), rec


class FlacDelivery:
    """What ``deliver`` hands back with a ``flac`` rule: ``pcm``, the quantiser's device records, and
    ``flac``, the encoder's records on the host (flac.FLAC_DTYPE, ``byte_off`` in the delivered buffer);
    ``files`` cuts the complete .flac files out of the delivered bytes once they are on the host."""

    def __init__(self, pcm, flac, rates, channels, bits, block):
        self.pcm, self.flac, self.rates, self.channels, self.bits, self.block = pcm, flac, rates, channels, bits, block

    def total(self):
        from .flac import total_bytes
        return total_bytes(self.flac)

    def files(self, host):
        from .flac import files
        return [files(host, self.flac[i:i + 1], self.rates[i], self.channels, self.bits, self.block)[0]
                for i in range(len(self.flac))]


def flac_packed(eng, pcm, byte_off, lens, rates, flac, bits, channels=2):
    """The packed PCM quantize_packed left in a device byte tensor (render i at byte_off[i] with lens[i]
    frames of ``channels`` words at rates[i] Hz) as FLAC frames, encoded where it lies: msg_flac per
    distinct rate (the rate is in every frame header) into one output tensor.  Returns (the frames'
    bytes, the records on the host in render order, ``byte_off`` counted in that tensor): reading the
    records waits for the device, because only they know the encoded lengths.  One rate: the output is
    compact, byte_off the 16-byte-rounded prefix of the lengths."""
    from .flac import FLAC_DTYPE, bound, records
    byte_off, lens, rates = _extents(byte_off, lens, rates)
    groups = rate_groups(rates)
    need = [sum((bound(lens[i], channels, bits, flac.block) + 15) // 16 * 16 for i in idx) for _, idx in groups]
    out = eng.torch.empty(int(sum(need)), dtype=eng.torch.uint8, device=pcm.device)
    rec = np.zeros(len(rates), dtype=FLAC_DTYPE)
    got, base = [], 0
    for (rate, idx), size in zip(groups, need):
        got.append(eng.flac(pcm, byte_off[idx], lens[idx], channels, bits, rate, flac.block, flac.md5,
                            out=out[base:base + size])[1])
        base += size
    base = 0
    for (rate, idx), size, r in zip(groups, need, got):
        r = records(r)
        r["byte_off"] += base
        rec[idx] = r
        base += size
    return out, rec


def unpack_all(host, byte_off, nbytes, bits, channels=2):
    """The integer arrays (frames, ``channels``) of quantize_packed's bytes once they are on the host."""
    from .pcm import unpack
    frame = int(channels) * (int(bits) // 8)
    return [unpack(host[int(o):int(o) + int(b)], bits, (int(b) // frame, int(channels))) for o, b in zip(byte_off, nbytes)]
