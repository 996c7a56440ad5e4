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
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    rates = [int(s) for s in sr_in]
    ratios = [ratio(s, out_sr) for s in rates]
    y_lens = np.array([resample_len(n, u, d) for n, (u, d) in zip(lens, ratios)], dtype=np.int64)
    y_off = np.concatenate([[0], np.cumsum(y_lens)[:-1]]).astype(np.int64)
    y = torch.empty((int(y_lens.sum()), 2), dtype=torch.float32, device=out.device)
    for rate in sorted(set(rates)):
        idx = [i for i, s in enumerate(rates) if s == rate]
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


def loudness_packed(eng, y, offsets, lens, rates, target_lufs, ceiling=None, true_peak=None):
    """Bring renders lying in a device tensor ((frames, 2) float32, render i at frame
    offsets[i] with lens[i] frames at rates[i] Hz) to ``target_lufs`` where they lie:
    msg_loudness then msg_loudness_gain per distinct rate, the gain formed on the
    device from each render's record (no host synchronise).  ``ceiling``: a linear
    sample peak no render may exceed (None: no limit).  ``true_peak``: a ceiling in
    dBTP (BS.1770 true peak, truepeak.py) no render may exceed: msg_truepeak is
    measured too and msg_truepeak_gain forms the one gain from both records.  Scales y
    in place and returns the device records in render order (engine.Engine.loudness)."""
    torch = eng.torch
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    rates = [int(s) for s in rates]
    rec = torch.empty((len(rates), 5), dtype=torch.float64, device=y.device)
    for rate in sorted(set(rates)):
        idx = [i for i, s in enumerate(rates) if s == rate]
        r = eng.loudness(y, offsets[idx], lens[idx], 2, rate)
        if true_peak is None:
            eng.loudness_gain(y, offsets[idx], lens[idx], 2, r, float(target_lufs), ceiling)
        else:
            t = eng.true_peak(y, offsets[idx], lens[idx], 2, rate)
            eng.true_peak_gain(y, offsets[idx], lens[idx], 2, t, r, float(target_lufs), _dbtp(true_peak), ceiling)
        if len(idx) == len(rates):
            return r
        rec[torch.as_tensor(idx, device=y.device)] = r
    return rec


def _dbtp(true_peak):
    """A dBTP ceiling as a linear true peak."""
    v = float(true_peak)
    if not np.isfinite(v):
        raise ValueError("the true-peak ceiling must be a number of dBTP")
    return 10.0 ** (v / 20.0)


def truepeak_packed(eng, y, offsets, lens, rates, true_peak, ceiling=None):
    """Hold renders lying in a device tensor (as loudness_packed) under ``true_peak`` dBTP
    where they lie, with no loudness target: msg_truepeak then msg_truepeak_gain per
    distinct rate, the gain (1 where the ceiling does not bind) formed on the device.
    ``ceiling``: a linear sample peak as well (None: no limit).  Scales y in place and
    returns the device records in render order (engine.Engine.true_peak)."""
    torch = eng.torch
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    rates = [int(s) for s in rates]
    rec = torch.empty((len(rates), 5), dtype=torch.float64, device=y.device)
    for rate in sorted(set(rates)):
        idx = [i for i, s in enumerate(rates) if s == rate]
        t = eng.true_peak(y, offsets[idx], lens[idx], 2, rate)
        eng.true_peak_gain(y, offsets[idx], lens[idx], 2, t, None, None, _dbtp(true_peak), ceiling)
        if len(idx) == len(rates):
            return t
        rec[torch.as_tensor(idx, device=y.device)] = t
    return rec


def _level(eng, y, offsets, lens, rates, lufs, ceiling, true_peak):
    if lufs is not None:
        loudness_packed(eng, y, offsets, lens, rates, lufs, ceiling, true_peak)
    elif true_peak is not None:
        truepeak_packed(eng, y, offsets, lens, rates, true_peak, ceiling)


def quantize_packed(eng, y, offsets, lens, bits, dither="tpdf", seed=0, keys=None):
    """Renders lying in a device tensor (as loudness_packed) as ``bits``-bit PCM, quantised
    and packed on the device after every level rule (msg_quantize, pcm.py): render i
    takes its dither from the stream (seed, keys[i]).  Returns the device byte tensor,
    each render's byte offset and length in it, and the device records (no host synchronise)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    out, byte_off, rec = eng.quantize(y, offsets, lens, 2, bits, dither, seed, keys)
    return out, byte_off, lens * (2 * (int(bits) // 8)), rec


def _pcm_results(eng, y, offsets, lens, results, bits, dither, seed):
    from .pcm import unpack
    out, byte_off, nbytes, _ = quantize_packed(eng, y, offsets, lens, bits, dither, seed, range(len(lens)))
    if results == "device":
        return [out[int(o):int(o) + int(b)] for o, b in zip(byte_off, nbytes)]
    eng.torch.cuda.synchronize(eng.device)
    host = out.cpu().numpy()                     # the bytes cross, not the float32 renders
    return [unpack(host[int(o):int(o) + int(b)], bits, (int(n), 2)) for o, b, n in zip(byte_off, nbytes, lens)]


def _out_peaks(params_list, out_peak):
    if out_peak is None:
        return None
    if isinstance(out_peak, str):
        if out_peak != "preset":
            raise ValueError("out_peak must be None, 'preset' or a number")
        return [float(merged(p)["peak"]) for p in params_list]
    return [float(out_peak)] * len(params_list)


def render_batch(params_list, device: int = 0, results: str = "audio", out_sr=None, out_peak=None, out_lufs=None,
                 out_ceiling=None, out_true_peak=None, out_bits=None, out_dither="tpdf", out_dither_seed=0):
    """Render many presets in one device batch; returns a list of (out_n, 2) float32
    arrays ("audio"), per-preset summaries ("stats", multi.rec_stats's fields,
    reduced on the device by msg_digest) or the device tensors themselves ("device").
    ``out_sr``: deliver the renders at that rate, resampled in HBM before any copy
    ("audio" or "device"); ``out_peak``: None, "preset" or a number, the peak the
    resampled renders are rescaled to (resample_packed).  ``out_lufs``: deliver each
    render at that BS.1770 integrated loudness, measured at the rate it is delivered at
    and scaled in HBM (loudness_packed); ``out_ceiling``: a linear sample peak the scaled
    renders may not exceed.  ``out_true_peak``: a ceiling in dBTP (BS.1770 true peak at
    the delivered rate) they may not exceed, alone or with ``out_lufs`` / ``out_ceiling``
    (truepeak_packed, loudness_packed).  ``out_bits``: 16 or 24, deliver fixed-point PCM,
    quantised last on the device (quantize_packed) with ``out_dither`` ("tpdf" or "none")
    from the stream (``out_dither_seed``, the preset's index): int16 / int32 arrays
    ("audio") or views of the packed byte tensor ("device")."""
    if results not in ("audio", "stats", "device"):
        raise ValueError("results must be 'audio', 'stats' or 'device'")
    if out_bits is not None:
        from .pcm import check_bits, dither_code
        check_bits(out_bits)
        dither_code(out_dither)
        if results == "stats":
            raise ValueError("out_bits applies to results 'audio' or 'device'")
    if out_true_peak is not None and out_peak is not None:
        raise ValueError("out_true_peak and out_peak are two level rules: give one")
    if out_true_peak is not None and results == "stats":
        raise ValueError("out_true_peak applies to results 'audio' or 'device'")
    if out_sr is None and out_peak is not None:
        raise ValueError("out_peak needs out_sr")
    if out_sr is not None and results == "stats":
        raise ValueError("out_sr applies to results 'audio' or 'device'")
    if out_lufs is not None and out_peak is not None:
        raise ValueError("out_lufs and out_peak are two level rules: give one")
    if out_lufs is not None and results == "stats":
        raise ValueError("out_lufs applies to results 'audio' or 'device'")
    if out_lufs is None and out_true_peak is None and out_ceiling is not None:
        raise ValueError("out_ceiling needs out_lufs")
    params_list = list(params_list)
    eng = default_engine(device)
    packed = PackedBatch(params_list)
    out = eng.render_packed(packed)
    if out_sr is None:
        _level(eng, out, packed.offsets, packed.out_n, [merged(p)["base_sr"] for p in params_list],
               out_lufs, out_ceiling, out_true_peak)
    if out_sr is not None:
        y, y_off, y_lens = resample_packed(eng, out, packed.offsets, packed.out_n,
                                           [merged(p)["base_sr"] for p in params_list], int(out_sr),
                                           _out_peaks(params_list, out_peak))
        _level(eng, y, y_off, y_lens, [int(out_sr)] * len(params_list), out_lufs, out_ceiling, out_true_peak)
        if out_bits is not None:
            return _pcm_results(eng, y, y_off, y_lens, results, out_bits, out_dither, out_dither_seed)
        parts = [y[int(o):int(o) + int(n)] for o, n in zip(y_off, y_lens)]
        if results == "device":
            return parts
        eng.torch.cuda.synchronize(eng.device)
        host = y.cpu().numpy()
        return [host[int(o):int(o) + int(n)].copy() for o, n in zip(y_off, y_lens)]
    if out_bits is not None:
        return _pcm_results(eng, out, packed.offsets, packed.out_n, results, out_bits, out_dither, out_dither_seed)
    if results == "device":
        return [out[int(o):int(o) + int(n)] for o, n in zip(packed.offsets, packed.out_n)]
    eng.torch.cuda.synchronize(eng.device)
    if results == "stats":
        from .multi import device_stats
        return device_stats(eng, out, packed.offsets, packed.out_n)
    host = out.cpu().numpy()
    return [host[o:o + n].copy() for o, n in zip(packed.offsets, packed.out_n)]
