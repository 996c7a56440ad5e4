"""The app's batch render (``AudioApp.on_batch``, MS:1524-1596) on the device.

The reference loops seeds x base-unfold x stretch-factor (outer to inner),
renders each variant with ``render(p)`` and writes it with
``sf.write(path, audio.astype(np.float32), out_sr)``.  Here the whole triple
product goes to the device as batches of presets (``render_batch``; one
workgroup grid per batch, no per-variant launch sequence) and each variant is
written as a float32 WAV by a small RIFF writer (soundfile is not a
dependency).

File names: the reference builds
``f"ms_seed{sd}_unf{u:g}_st{st:g}_{out_sr}Hz.wav".replace(".", "p")`` (MS:1587),
which also turns the ``.wav`` suffix into ``pwav``; libsndfile then cannot infer
a format from that name and the reference's batch stops at its first file.
``names="reference"`` keeps that exact string (the writer here does not need
an extension); the default ``names="wav"`` applies the same replacement to the
stem and keeps a real ``.wav`` suffix.
"""
from __future__ import annotations

import os
import struct

import numpy as np

from .params import merged

# presets per device batch: bounds the output buffer (frames x 2 float32) and
# the per-batch event tables; the batch scheduler handles any mix of lengths.
MAX_BATCH_PRESETS = 1024
MAX_BATCH_FRAMES = 1 << 30      # 8 GiB of float32 stereo output


def parse_list(s, cast=float):
    """Comma-separated list, unparsable entries skipped (MS:1557-1566)."""
    out = []
    for p in str(s).split(","):
        p = p.strip()
        if not p:
            continue
        try:
            out.append(cast(p))
        except Exception:
            pass
    return out


def variant_name(sd, u, st, out_sr, names="wav"):
    if names == "reference":
        return f"ms_seed{sd}_unf{u:g}_st{st:g}_{out_sr}Hz.wav".replace(".", "p")
    if names == "wav":
        return f"ms_seed{sd}_unf{u:g}_st{st:g}_{out_sr}Hz".replace(".", "p") + ".wav"
    raise ValueError("names must be 'wav' or 'reference'")


def variants(base_params, seeds, unfolds, stretches):
    """The parameter dicts in the reference's loop order (MS:1580-1586)."""
    if isinstance(seeds, str):
        seeds = parse_list(seeds, int)
    if isinstance(unfolds, str):
        unfolds = parse_list(unfolds, float)
    if isinstance(stretches, str):
        stretches = parse_list(stretches, float)
    out = []
    for sd in seeds:
        for u in unfolds:
            for st in stretches:
                p = dict(base_params)
                p["seed"] = int(sd)
                p["time_unfold"] = float(u)
                p["partial_stretch"] = float(st)
                out.append(((sd, u, st), p))
    return out


def write_wav_float32(path, audio, sr):
    """IEEE-float WAV (format tag 3, fmt + fact + data chunks), frames x channels."""
    a = np.ascontiguousarray(audio, dtype="<f4")
    if a.ndim == 1:
        a = a[:, None]
    frames, ch = a.shape
    data_bytes = a.nbytes
    if data_bytes + 64 > 0xFFFFFFFF:
        raise ValueError("WAV data beyond 4 GiB")
    fmt = struct.pack("<HHIIHHH", 3, ch, int(sr), int(sr) * ch * 4, ch * 4, 32, 0)
    fact = struct.pack("<I", frames)
    riff_size = 4 + (8 + len(fmt)) + (8 + len(fact)) + (8 + data_bytes)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", riff_size) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"fact" + struct.pack("<I", len(fact)) + fact)
        f.write(b"data" + struct.pack("<I", data_bytes))
        a.tofile(f)


def read_wav_float32(path):
    """Reader for the files write_wav_float32 makes: (frames x channels float32, sr)."""
    with open(path, "rb") as f:
        b = f.read()
    if b[:4] != b"RIFF" or b[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    pos, ch, sr, data = 12, None, None, None
    while pos + 8 <= len(b):
        tag, size = b[pos:pos + 4], struct.unpack("<I", b[pos + 4:pos + 8])[0]
        body = b[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            tagv, ch, sr = struct.unpack("<HHI", body[:8])
            if tagv != 3:
                raise ValueError("not an IEEE-float WAV")
        elif tag == b"data":
            data = np.frombuffer(body, dtype="<f4")
        pos += 8 + size + (size & 1)
    if ch is None or data is None:
        raise ValueError("missing fmt or data chunk")
    return data.reshape(-1, ch).copy(), sr


def _chunks(items, frames_of):
    cur, tot = [], 0
    for it in items:
        fr = frames_of(it)
        if cur and (len(cur) >= MAX_BATCH_PRESETS or tot + fr > MAX_BATCH_FRAMES):
            yield cur
            cur, tot = [], 0
        cur.append(it)
        tot += fr
    if cur:
        yield cur


def render_variations(base_params, seeds, unfolds, stretches, folder=None, device: int = 0,
                      names="wav", progress=None, devices=None, export_sr=None, export_peak=None,
                      export_lufs=None, export_ceiling=None, export_true_peak=None, export_bits=None,
                      export_dither="tpdf", export_dither_seed=0, export_records=None, export_limiter=None,
                      export_report=None, export_shape=None, export_flac_records=None, export_flac=None, export_gate=None,
                      export_dynamics=None, export_stereo=None, export_filter=None, export_edges=None):
    """Render every (seed, unfold, stretch) variant of ``base_params`` on the device
    (or, with ``devices``, sharded across those GPUs, multi.py).

    Returns a list of ``(name, audio, out_sr)`` in the reference's order (audio
    (out_n, 2) float32); with ``folder``, also writes each as a float32 WAV
    (with ``export_bits``: integer audio and integer-PCM WAVs, see below).
    ``progress(percent, text)`` gets the reference's status line per file.

    ``export_sr``: deliver the variants at that rate instead of ``base_sr``: each
    batch is resampled in HBM (resample.py) before it is copied to the host, and
    the file names, WAV headers and the returned out_sr carry ``export_sr``.
    ``export_peak="preset"`` rescales each resampled variant so that max|y| is the
    preset's ``peak`` again (resampling moves the peak); None leaves the samples
    as resampled.  One device only.

    ``export_lufs``: deliver every variant at that BS.1770-4 integrated loudness
    (LUFS; -23 for EBU R 128): each is measured at the rate it is delivered at
    (after the resampling when ``export_sr`` is given) and scaled in HBM before the
    copy (loudness.py); ``export_ceiling``: a linear sample peak no scaled variant
    may exceed (None: no limit).  Not together with ``export_peak``.  One device only.

    ``export_true_peak``: a ceiling in dBTP (-1 for EBU R 128) on every variant's
    BS.1770-4 true peak, measured at the rate it is delivered at and held in HBM before
    the copy (truepeak.py); alone, or with ``export_lufs`` / ``export_ceiling``, one
    gain per variant from all of them.  Not together with ``export_peak``.  One device only.

    ``export_bits``: 16 or 24, deliver fixed-point PCM: each variant is quantised on the
    device after every level rule (pcm.py), with ``export_dither`` "tpdf" (or "none") from
    the stream (``export_dither_seed``, the variant's index in the full seed x unfold x
    stretch order, so the bits do not depend on how the batch is cut); the packed bytes
    are what is copied to the host, the files are plain integer-PCM WAVs under the same
    names, and the returned audio is the integer array in the file (int16, or int32 at
    24 bits).  ``export_records``: a list that gets every variant's msg_pcm_rec
    (pcm.PCM_DTYPE: clipped, nan, q_min, q_max, bits, dither) appended.  One device only.

    ``export_limiter``: hold ``export_true_peak`` with the look-ahead true-peak limiter
    (limit.py) instead of one static gain: only the frames around a peak over the ceiling
    are turned down, so a variant with a stray peak is delivered at ``export_lufs`` and not
    below it by that peak's excess.  None off, True a 5 ms look-ahead, a positive number
    that many milliseconds; a static trim after it holds the ceiling on dense material.
    Needs ``export_true_peak``.  One device only.

    ``export_report``: a list that gets one row per variant (export.REPORT_DTYPE: lufs, lra,
    lo, hi, max_momentary, max_short, peak, true_peak, dbtp, frames, rate), the EBU R 128
    meters of the float32 variant as it is delivered, measured on the device after every level
    rule and before the quantiser (lrange.py, truepeak.py); with ``folder``, the rows are also
    written to ``loudness_report.csv`` there, one line per file name.  One device only.

    ``export_shape``: with ``export_bits``, noise-shaped dither: "e3", "lipshitz5" or "f9"
    (pcm.py, psychoacoustic curves for 44.1 / 48 kHz).  The streams and keys are those of
    ``export_dither``; the total error of every word is fed back along its channel, one
    chain per channel of each variant, so the bits still do not depend on how the batch is cut.

    ``export_edges``: an edges.Edges: every variant's ends are shaped after the resampler and
    before the level rules (edges.py): trimmed to the span that holds sound (``trim_db``,
    ``pad_ms``), faded in and out (``fade_ms``, ``curve``) or its tail crossfaded into its head
    as a seamless loop (``loop_ms``).  The files, the returned audio, the report's ``frames`` and
    ``loudness_report.csv`` carry the delivered span; the meters and the ceiling hold on it, and
    the dither counts from its first word.  One device only.

    ``export_filter``: a filter.Filter: every variant is run through its biquad cascade (a rumble
    high-pass, shelves, peaks, a low-pass, or raw sections; ``zero_phase`` for no phase shift) in
    float64 in HBM, after the resampler and before ``export_edges`` and the level rules, so the
    meters, the ceiling and the trim see what is delivered (filter.py).  One device only.

    ``export_stereo``: a stereo.Stereo: every variant is metered for phase correlation (``meter``: a
    list that gets one row per variant), given a width, balance, swap or polarity matrix
    (``invert="auto"``: the right channel inverted where the correlation is negative) or folded to
    mono (``channels=1``) in HBM, after ``export_filter`` and before ``export_edges`` and the level
    rules, which then level, hold and report the mono render; the files are then one-channel WAVs
    and the returned audio is (n, 1) (stereo.py).  One device only.

    ``export_dynamics``: a dynamics.Dynamics: every variant is compressed in HBM (threshold, ratio,
    soft knee, linear-in-dB attack, hold and release, makeup; dynamics.py), after ``export_stereo`` and
    before ``export_edges`` and the level rules, which then level, hold and report what is delivered.
    One device only.

    ``export_gate``: a gate.Gate: every variant is gated in HBM (threshold, hysteresis, ratio, range,
    linear-in-dB attack and release, hold; gate.py), after ``export_stereo`` and before
    ``export_dynamics`` and ``export_edges``, so a trim sees the gated tail.  One device only.

    ``export_flac``: a flac.Flac, with ``export_bits``: the quantised PCM of every variant is encoded as
    FLAC frames in HBM (flac.py) and only the encoded bytes cross to the host; each result's audio is the
    complete .flac file as a uint8 array and, with a folder, ``<name>.flac`` is written instead of the
    WAV.  ``export_records`` keeps receiving the PCM records; ``export_flac_records``: a list that gets
    every variant's msg_flac_rec (flac.FLAC_DTYPE).  One device only.
    """
    from .pack import PackedBatch, out_frames

    from .export import Delivery, deliver, unpack_all

    delivery = Delivery(sr=export_sr, peak=export_peak, lufs=export_lufs, ceiling=export_ceiling,
                        true_peak=export_true_peak, bits=export_bits, dither=export_dither,
                        dither_seed=export_dither_seed, limiter=export_limiter, report=export_report,
                        shape=export_shape, edges=export_edges, filter=export_filter, stereo=export_stereo,
                        gate=export_gate, dynamics=export_dynamics, flac=export_flac)
    delivery.check("export_", n_devices=len(list(devices)) if devices is not None else 1, numeric_peak=False,
                   rates=[merged(base_params)["base_sr"]])
    first_row = len(export_report) if export_report is not None else 0
    if export_bits is not None:
        from .pcm import records, write_wav_pcm
    base = merged(base_params)
    pairs = variants(base, seeds, unfolds, stretches)
    keys = [key for key, _ in pairs]
    total = max(1, len(keys))
    base_sr = int(base["base_sr"])                # every variant has the template's out_n and base_sr
    out_sr = base_sr if export_sr is None else int(export_sr)
    results = []

    def emit(key, audio):
        name = variant_name(*key, out_sr, names)
        if export_flac is not None:
            name = name[:-4] + ".flac"                # "….wav" and the reference's "…pwav" alike
            if folder is not None:
                audio.tofile(os.path.join(folder, name))
        elif folder is not None and export_bits is not None:
            write_wav_pcm(os.path.join(folder, name), audio, out_sr, export_bits)
        elif folder is not None:
            write_wav_float32(os.path.join(folder, name), audio, out_sr)
        results.append((name, audio, out_sr))
        if progress:
            progress(int(100 * len(results) / total), f"Batch: {len(results)}/{total} → {name}")

    if devices is not None and len(list(devices)) > 1:
        from .multi import pool_for
        for key, audio in zip(keys, pool_for(devices).render_batch([p for _, p in pairs])):
            emit(key, audio)
        return results
    if devices is not None:
        device = int(list(devices)[0])
    from .engine import default_engine
    eng = default_engine(device)
    frames = out_frames(base)
    done = 0                                         # variants before this chunk: the dither key's base
    for chunk in _chunks(keys, lambda k: frames):
        packed = PackedBatch.variants(base, chunk)   # the template packed once (MS:1578-1584)
        out = eng.render_packed(packed)
        # resampled, levelled and quantised where it lies; the copy below is what is delivered
        peaks = [float(base["peak"])] * len(chunk) if export_peak == "preset" else None
        out, offsets, lens, rec = deliver(eng, out, packed.offsets, packed.out_n, [base_sr] * len(chunk), delivery,
                                          peaks, range(done, done + len(chunk)))
        done += len(chunk)
        eng.torch.cuda.synchronize(eng.device)
        host = (out if export_flac is None else out[:rec.total()]).cpu().numpy()
        delivery.flush_report()
        if export_flac is not None:
            if export_records is not None:
                export_records.extend(records(rec.pcm))
            if export_flac_records is not None:
                export_flac_records.extend(rec.flac)
            audio = rec.files(host)
        elif export_bits is not None:
            if export_records is not None:
                export_records.extend(records(rec))
            audio = unpack_all(host, offsets, lens, export_bits, delivery.channels())
        else:
            audio = [host[int(off):int(off) + int(n)].copy() for off, n in zip(offsets, lens)]
        for key, a in zip(chunk, audio):
            emit(key, a)
    if export_report is not None and folder is not None:
        from .export import write_report_csv
        write_report_csv(os.path.join(folder, "loudness_report.csv"), [name for name, _, _ in results],
                         export_report[first_row:])
    return results
