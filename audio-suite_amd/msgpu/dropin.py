"""Drop-in ``render(params, progress=None)`` for microsound_0.2.1/main_v2.py:588.

Usage from the unchanged PyQt6 front-end::

    import main_v2, msgpu
    main_v2.render = msgpu.render      # RenderWorker.run (MS:811) and on_batch (MS:1585)

Returns ``(audio, meta)`` like the reference: ``audio`` is a C-contiguous
(out_n, 2) float32 array (the consumers only read its shape/columns and cast
with ``astype(np.float32)`` before ``sf.write``, MS:1473-1519, 1589), ``meta``
has ``out_sr``, ``design_sr_base``, ``micro_last``, ``grain_last`` (MS:786-791).
The ``progress`` callback gets the reference's messages: 0 with the SR line,
every 50th event, and 100 "Done." (MS:599-600, 757-758, 783-784).  The event
messages are sent from the render's plan while the device is still rendering
(msg_render_batch returns once the batch is enqueued), "Done." after the
device has finished.

Errors follow the reference: ``KeyError`` for a key ``render`` indexes and the
dict lacks (pass ``msgpu.merged(partial)`` for a partial preset, as the UI's
loader merges it over the factory defaults), ``ValueError`` where MS raises it,
``NotImplementedError`` for the device limits in DESIGN.md.
"""
from __future__ import annotations

import numpy as np

from .engine import default_engine
from .export import (Delivery, deliver, unpack_all,  # noqa: F401  (the packed passes stay importable from here)
                     edges_packed, filter_packed, limiter_packed, loudness_packed, quantize_packed, resample_packed,
                     stereo_packed, truepeak_packed)
from .pack import PackedBatch, design_sr
from .params import first_missing_key, merged

def render(params, progress=None, device: int = 0):
    missing = first_missing_key(params)
    if missing is not None:
        raise KeyError(missing)
    p = merged(params)
    base_sr = int(p["base_sr"])
    if progress:
        progress(0, f"Output SR {base_sr} Hz | Design SR {design_sr(p)} Hz")
    eng = default_engine(device)
    packed = PackedBatch([p])
    out = eng.render_packed(packed)           # returns once enqueued
    info = eng.last_plan()[0]
    if progress:                              # MS:757-758, while the device renders
        events = eng.last_events(0)
        n = len(events)
        for e in events:
            if e.len > 0 and e.index % 50 == 0:
                note = _event_note(p, e.index)
                progress(int(5 + 70 * (e.index / max(1, n))), f"Events {e.index}/{n}  {note}".strip())
    eng.torch.cuda.synchronize(eng.device)
    audio = out.cpu().numpy().reshape(packed.total_frames, 2)
    if progress:
        progress(100, "Done.")
    micro = grain = None
    if info.n_events > 0:
        micro, grain = eng.last_meta(0, int(info.max_n))
    meta = {"out_sr": base_sr, "design_sr_base": int(info.design_sr),
            "micro_last": micro, "grain_last": grain}
    return np.ascontiguousarray(audio), meta


def _event_note(p, i):
    """The generator note of event i (MS:342-362, shown by MS:758): "IR fragment",
    "Image line y=<row>" with the row drawn by default_rng(seed + i).integers(0, h)
    (the library's NumPy-exact stream, msg_rng_integers), or the no-source notes."""
    mode = p["gen_mode"]
    if mode == "IR fragment":
        ir = p.get("_ir_audio")
        return "No IR loaded" if (ir is None or np.asarray(ir).size < 32) else "IR fragment"
    if mode == "Image scanline":
        img = p.get("_img_gray")
        if img is None:
            return "No image loaded"
        from . import _lib as L
        import ctypes as C
        y = C.c_int64(0)
        L.check(L.lib().msg_rng_integers(int(p["seed"]) + int(i), 0, int(np.asarray(img).shape[0]), C.byref(y), 1),
                None)
        return f"Image line y={y.value}"
    return ""


def _out_peaks(params_list, out_peak):
    if out_peak is None:
        return None
    if isinstance(out_peak, str):
        if out_peak != "preset":
            raise ValueError("out_peak must be None, 'preset' or a number")
        return [float(merged(p)["peak"]) for p in params_list]
    return [float(out_peak)] * len(params_list)


def render_batch(params_list, device: int = 0, results: str = "audio", out_sr=None, out_peak=None, out_lufs=None,
                 out_ceiling=None, out_true_peak=None, out_bits=None, out_dither="tpdf", out_dither_seed=0,
                 out_limiter=None, out_report=None, out_shape=None, out_flac=None, out_gate=None, out_dynamics=None,
                 out_stereo=None, out_filter=None, out_edges=None):
    """Render many presets in one device batch; returns a list of (out_n, 2) float32
    arrays ("audio"), per-preset summaries ("stats", multi.rec_stats's fields,
    reduced on the device by msg_digest) or the device tensors themselves ("device").
    ``out_sr``: deliver the renders at that rate, resampled in HBM before any copy
    ("audio" or "device"); ``out_peak``: None, "preset" or a number, the peak the
    resampled renders are rescaled to (export.resample_packed).  ``out_lufs``: deliver each
    render at that BS.1770 integrated loudness, measured at the rate it is delivered at
    and scaled in HBM (loudness_packed); ``out_ceiling``: a linear sample peak the scaled
    renders may not exceed.  ``out_true_peak``: a ceiling in dBTP (BS.1770 true peak at
    the delivered rate) they may not exceed, alone or with ``out_lufs`` / ``out_ceiling``
    (truepeak_packed, loudness_packed).  ``out_bits``: 16 or 24, deliver fixed-point PCM,
    quantised last on the device (quantize_packed) with ``out_dither`` ("tpdf" or "none")
    from the stream (``out_dither_seed``, the preset's index): int16 / int32 arrays
    ("audio") or views of the packed byte tensor ("device").  ``out_limiter``: hold
    ``out_true_peak`` with the look-ahead limiter (export.limiter_packed) instead of one
    static gain, so a render with a stray peak keeps its loudness: None off, True a 5 ms
    look-ahead, a positive number that many milliseconds.  ``out_report``: a list that gets one
    row per render (export.REPORT_DTYPE: lufs, lra, lo, hi, max_momentary, max_short, peak,
    true_peak, dbtp, frames, rate), metered on the device on the float32 render as it is
    delivered, after every level rule and before the quantiser (export.report_packed); the
    rows are read once the renders' copy has been waited for ("device": when the call returns).
    ``out_shape``: with ``out_bits``, noise-shaped dither ("e3", "lipshitz5" or "f9", pcm.py): the
    same streams, the error fed back along each channel of each render.  ``out_edges``: an
    edges.Edges, the ends of every render shaped after the resampler and before the level rules
    (export.edges_packed): trimmed to the span that holds sound, faded in and out, or its tail
    crossfaded into its head as a loop.  The arrays, tensors, reports and dither streams are then
    those of the span; a trim or a loop costs the chain one host wait for the spans.  ``out_filter``: a
    filter.Filter, every render run through its biquad cascade in float64 where it lies
    (export.filter_packed), after the resampler and before the edges and the level rules: a trim sees
    the filtered signal, fades still end at zero, and loudness, true peak, limiter and report
    measure what is delivered.  ``out_stereo``: a stereo.Stereo (export.stereo_packed), after the filter
    and before the edges and the level rules: a phase-correlation meter (``meter``: a list that gets
    one row per render, read with the report's rows), a width, balance, swap or polarity matrix over
    every frame (``invert="auto"`` repairs the renders whose correlation is negative, on the device),
    and ``channels=1``, the fold to mono in HBM, after which every later rule, the report and the
    quantiser work on the mono render and the arrays and tensors are (n, 1).  ``out_dynamics``: a
    dynamics.Dynamics (export.dynamics_packed), after the stereo rule and before the edges and the level
    rules: every render compressed in HBM (threshold, ratio, soft knee, linear-in-dB attack, hold and
    release, makeup), so a report after it shows the loudness range come down.  ``out_gate``: a gate.Gate
    (export.gate_packed), after the stereo rule and before ``out_dynamics`` and the edges: every render
    gated in HBM (threshold, hysteresis, ratio, range, linear-in-dB attack and release, hold), so the
    compressor's makeup cannot lift what the gate removed and a trim sees the gated tail.  ``out_flac``: a
    flac.Flac, with ``out_bits`` (export.flac_packed): the quantised PCM is encoded as FLAC frames in HBM and
    every result is the complete .flac file as a uint8 array, stream header included ("device": the frames'
    device bytes per render, without a header); only the encoded bytes cross to the host."""
    delivery = Delivery(sr=out_sr, peak=out_peak, lufs=out_lufs, ceiling=out_ceiling, true_peak=out_true_peak,
                        bits=out_bits, dither=out_dither, dither_seed=out_dither_seed, limiter=out_limiter,
                        report=out_report, shape=out_shape, edges=out_edges, filter=out_filter, stereo=out_stereo,
                        gate=out_gate, dynamics=out_dynamics, flac=out_flac)
    params_list = list(params_list)
    delivery.check("out_", results, rates=[merged(p)["base_sr"] for p in params_list])
    eng = default_engine(device)
    packed = PackedBatch(params_list)
    out = eng.render_packed(packed)
    peaks = _out_peaks(params_list, out_peak) if out_sr is not None else None
    y, off, lens, rec = deliver(eng, out, packed.offsets, packed.out_n, [merged(p)["base_sr"] for p in params_list],
                              delivery, peaks, range(len(params_list)))
    if results == "device":
        delivery.flush_report()
        return [y[int(o):int(o) + int(n)] for o, n in zip(off, lens)]
    eng.torch.cuda.synchronize(eng.device)
    delivery.flush_report()
    if results == "stats":
        from .multi import device_stats
        return device_stats(eng, out, packed.offsets, packed.out_n)
    if out_flac is not None:                     # the encoded bytes cross and nothing more
        return rec.files(y[:rec.total()].cpu().numpy())
    host = y.cpu().numpy()                       # quantised: the bytes cross, not the float32 renders
    if out_bits is not None:
        return unpack_all(host, off, lens, out_bits, delivery.channels())
    return [host[int(o):int(o) + int(n)].copy() for o, n in zip(off, lens)]
