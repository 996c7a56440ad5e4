"""msgpu — MI355X-native Microsound render engine.

Drop-in for ``microsound_0.2.1/main_v2.py:render``::

    import msgpu
    audio, meta = msgpu.render(params)           # same signature as the reference

The compute path is libmsgpu.so (HIP kernels for gfx950) bound by ctypes; there
is no CPU fallback.
"""
from .params import DEFAULTS, CONFIGS, config_params, merged  # noqa: F401
# the submodule first: importing it later would rebind the name ``msgpu.resample``
# from the function below to the module (reach the module's names with
# ``from msgpu.resample import design, ...``)
from . import resample as _resample  # noqa: F401
from . import loudness as _loudness  # noqa: F401  (the same for ``msgpu.loudness``)
from . import lrange as _lrange  # noqa: F401
from . import truepeak as _truepeak  # noqa: F401
from . import pcm as _pcm  # noqa: F401
from . import limit as _limit  # noqa: F401
from . import edges as _edges  # noqa: F401
from .edges import Edges  # noqa: F401
from . import filter as _filter  # noqa: F401
from .filter import Filter  # noqa: F401
from . import stereo as _stereo  # noqa: F401
from .stereo import Stereo  # noqa: F401
from . import dynamics as _dynamics  # noqa: F401
from .dynamics import Dynamics  # noqa: F401
from . import gate as _gate  # noqa: F401
from .gate import Gate  # noqa: F401
from . import flac as _flac  # noqa: F401
from .flac import Flac  # noqa: F401


def render(params, progress=None, device: int = 0):
    from .dropin import render as _render
    return _render(params, progress, device)


def render_batch(params_list, device: int = 0, devices=None, results: str = "audio", out_sr=None, out_peak=None,
                 out_lufs=None, out_ceiling=None, out_true_peak=None, out_bits=None, out_dither="tpdf",
                 out_dither_seed=0, out_limiter=None, out_report=None, out_shape=None, out_flac=None, out_gate=None,
                 out_dynamics=None, out_stereo=None, out_filter=None, out_edges=None):
    """Render many presets; ``devices`` (e.g. range(8)) shards them across GPUs,
    one worker process per GPU (multi.py; call before this process touches the GPU).
    ``results``: "audio" ((out_n, 2) float32 arrays), "stats" (a summary per
    preset, multi.audio_stats) or "device" (the renders stay in HBM: device
    tensors on one GPU, multi.DeviceResult handles across several).
    ``out_sr``: deliver "audio" / "device" results at that rate, resampled in HBM
    before any copy (resample.py; one device only); ``out_peak``: None, "preset"
    or a number, the peak each resampled render is rescaled to.  ``out_lufs``:
    deliver each render at that BS.1770 integrated loudness (LUFS), measured at the
    delivered rate and scaled in HBM (loudness.py; one device only), with
    ``out_ceiling`` a linear sample peak it may not exceed.  ``out_true_peak``: a
    ceiling in dBTP (BS.1770 true peak at the delivered rate, truepeak.py; one device
    only), alone or with ``out_lufs`` / ``out_ceiling``; not with ``out_peak``.
    ``out_bits``: 16 or 24, deliver fixed-point PCM quantised on the device after every
    other rule (pcm.py; one device only): "audio" gives int16 / int32 arrays, "device"
    views of the packed byte tensor; ``out_dither`` "tpdf" or "none", from the stream
    (``out_dither_seed``, the preset's index in ``params_list``).  ``out_limiter``: hold
    ``out_true_peak`` with the look-ahead true-peak limiter (limit.py; one device only)
    instead of one static gain: None off, True a 5 ms look-ahead, a number of milliseconds.
    ``out_report``: a list that gets one row per render with the EBU R 128 meters of what is
    delivered (export.REPORT_DTYPE: lufs, lra, lo, hi, max_momentary, max_short, peak, true_peak,
    dbtp, frames, rate; lrange.py; one device only, "audio" or "device").  ``out_shape``: with
    ``out_bits``, noise-shaped dither: "e3", "lipshitz5" or "f9" (pcm.py).  ``out_edges``: an
    edges.Edges, every render trimmed to the span that holds sound, faded, or looped before the
    level rules (edges.py; one device only).  ``out_filter``: a filter.Filter, every render run
    through its biquad cascade (a rumble high-pass, shelves, peaks, a low-pass) after the resampler
    and before the edges and the level rules, which then see what is delivered (filter.py; one
    device only).  ``out_stereo``: a stereo.Stereo, after the filter and before the edges and the
    level rules: a phase-correlation meter, a width / balance / swap / polarity matrix, or
    ``channels=1``, the fold to mono in HBM, so that a mono delivery is levelled, held, reported and
    quantised as delivered and comes back as (n, 1) arrays (stereo.py; one device only).
    ``out_dynamics``: a dynamics.Dynamics, after the stereo rule and before the edges and the level
    rules: every render compressed in HBM (dynamics.py; one device only).  ``out_gate``: a gate.Gate,
    after the stereo rule and before ``out_dynamics``: every render gated in HBM (gate.py; one device
    only).  ``out_flac``: a flac.Flac, with ``out_bits``: every result is the complete .flac file as a
    uint8 array, encoded in HBM from the quantised PCM (flac.py; one device only)."""
    if devices is not None and len(list(devices)) > 1:
        from .export import Delivery
        Delivery(sr=out_sr, peak=out_peak, lufs=out_lufs, ceiling=out_ceiling, true_peak=out_true_peak, bits=out_bits,
                 limiter=out_limiter, report=out_report, edges=out_edges, filter=out_filter,
                 stereo=out_stereo, gate=out_gate, dynamics=out_dynamics, flac=out_flac).one_device(
            "out_", len(list(devices)), companions=True)
        # an option of out_bits and no rule of one_device's: with out_bits it was refused above
        if out_shape is not None:
            raise ValueError("out_shape needs out_bits")
        from .multi import pool_for
        return pool_for(devices).render_batch(params_list, results=results)
    if devices is not None:
        device = int(list(devices)[0])
    from .dropin import render_batch as _rb
    return _rb(params_list, device, results, out_sr=out_sr, out_peak=out_peak, out_lufs=out_lufs,
               out_ceiling=out_ceiling, out_true_peak=out_true_peak, out_bits=out_bits, out_dither=out_dither,
               out_dither_seed=out_dither_seed, out_limiter=out_limiter, out_report=out_report, out_shape=out_shape,
               out_edges=out_edges, out_filter=out_filter, out_stereo=out_stereo, out_gate=out_gate,
               out_dynamics=out_dynamics, out_flac=out_flac)


def DevicePool(devices, stub: bool = False, share_devices: bool = False):
    """One render worker per GPU (multi.py); create it before any GPU call."""
    from .multi import DevicePool as _P
    return _P(devices, stub, share_devices)


def stft_mag_db(x, sr=None, win=2048, hop=256, max_frames=3000, device: int = 0):
    """The app's spectrogram (MS:197-212) on the device; see spectrum.py."""
    from .spectrum import stft_mag_db as _s
    return _s(x, sr, win, hop, max_frames, device)


def fir(x, h, device: int = 0):
    """Standalone causal FIR np.convolve(x, h)[:len(x)] on the device (MS:444 arithmetic, any tap count)."""
    from .engine import default_engine
    import numpy as np
    eng = default_engine(device)
    torch = eng.torch
    if isinstance(x, torch.Tensor):
        return eng.fir(x.contiguous(), h)[0]
    a = np.ascontiguousarray(x, dtype=np.float32)
    y, _ = eng.fir(torch.from_numpy(a).to(f"cuda:{eng.device}"), h)
    torch.cuda.synchronize(eng.device)
    return y.cpu().numpy()


def resample(x, sr_in, sr_out, device: int = 0, **design):
    """Sample-rate conversion of x, (n,) or (n, 2), on the device (polyphase FIR,
    Kaiser-windowed sinc; see resample.py).  NumPy in, float32 NumPy out; a device
    tensor in, a device tensor out with no host synchronise."""
    return _resample.resample(x, sr_in, sr_out, device, **design)


def loudness(x, sr, device: int = 0):
    """BS.1770-4 integrated loudness of x, (n,) or (n, 2), at sr Hz, measured on the device
    in float64 (see loudness.py).  NumPy in, a float (LUFS) out; a device tensor in, a
    one-element device tensor out with no host synchronise."""
    return _loudness.loudness(x, sr, device)


def loudness_range(x, sr, device: int = 0):
    """The EBU R 128 delivery meters of x, (n,) or (n, 2), at sr Hz from one measurement on the
    device (see lrange.py): a dict with lufs, lra (EBU Tech 3342), lo, hi, max_momentary,
    max_short (EBU Tech 3341) and gate.  NumPy in, floats out; a device tensor in,
    one-element device tensors out with no host synchronise."""
    return _lrange.loudness_range(x, sr, device)


def loudness_curves(x, sr, device: int = 0):
    """(momentary, short_term) loudness of x in LUFS at ten values per second, from the hop
    sums the device measures (see lrange.py).  NumPy in, NumPy out; a device tensor in,
    device tensors out with no host synchronise."""
    return _lrange.loudness_curves(x, sr, device)


def true_peak(x, sr, device: int = 0, db: bool = False):
    """BS.1770-4 true peak of x, (n,) or (n, 2), at sr Hz, measured on the device (see
    truepeak.py): linear, or dBTP with ``db``.  NumPy in, a float out; a device tensor in,
    a one-element device tensor out with no host synchronise."""
    return _truepeak.true_peak(x, sr, device, db)


def limit(x, sr, ceiling_dbtp=-1.0, lookahead_ms=5.0, device: int = 0):
    """Hold x, (n,) or (n, 2), at sr Hz under ``ceiling_dbtp`` dBTP with the look-ahead
    true-peak limiter on the device (see limit.py).  NumPy in: a limited float32 copy and
    its record out; a device tensor in: limited in place with no host synchronise, the
    device record tensor out."""
    return _limit.limit(x, sr, ceiling_dbtp, lookahead_ms, device)


def edges(x, sr, edges, device: int = 0):
    """Shape the ends of x, (n,) or (n, 2), at sr Hz on the device with an edges.Edges: silence
    trim, fades or a loop crossfade (see edges.py).  NumPy in: the shaped span as a new float32
    array and its record out; a device tensor in: shaped in place with no host synchronise,
    the device record tensor out."""
    return _edges.edges(x, sr, edges, device)


def filter(x, sr, flt, device: int = 0, reverse=False):
    """Run x, (n,) or (n, 2), at sr Hz through the biquad cascade of a filter.Filter on the device
    (see filter.py): high- and low-pass, shelves, peaks or raw sections, in float64, optionally
    zero-phase.  NumPy in: a filtered float32 copy out; a device tensor in: filtered in place with
    no host synchronise and returned."""
    return _filter.filter(x, sr, flt, device, reverse)


def stereo_meter(x, sr, device: int = 0):
    """The stereo meter of x, (n, 2), at sr Hz, measured on the device (see stereo.py): the float64
    sums of L^2, R^2 and L R, the phase correlation, the smallest correlation of a 400 ms block and
    its index, and from the sums the channel balance, the level a mono fold-down loses and the
    side-to-mid ratio.  NumPy in, a record out; a device tensor in, the device record out (no host
    synchronise)."""
    return _stereo.stereo_meter(x, sr, device)


def stereo(x, sr, stereo, device: int = 0):
    """Apply a stereo.Stereo to x, (n, 2) at sr Hz, on the device (see stereo.py): width, balance,
    swap, polarity (``"auto"``: from the measured correlation) as one matrix over every frame, or
    the fold to mono.  Returns (n, 2) or (n, 1); NumPy in, a float32 array out; a device tensor in,
    shaped in place (or folded into a new tensor) with no host synchronise."""
    return _stereo.stereo(x, sr, stereo, device)


def dynamics(x, sr, dyn, device: int = 0):
    """Compress x, (n,) or (n, 2), at sr Hz on the device with a dynamics.Dynamics: threshold, ratio,
    soft knee, linear-in-dB attack, hold and release, makeup (see dynamics.py).  NumPy in: a
    compressed float32 copy and its record out; a device tensor in: compressed in place with no
    host synchronise, the device record tensor out."""
    return _dynamics.dynamics(x, sr, dyn, device)


def gate(x, sr, gate, device: int = 0):
    """Gate x, (n,) or (n, 2), at sr Hz on the device with a gate.Gate: threshold, hysteresis, ratio,
    range, linear-in-dB attack and release, hold (see gate.py).  NumPy in: a gated float32 copy and
    its record out; a device tensor in: gated in place with no host synchronise, the device record
    tensor out."""
    return _gate.gate(x, sr, gate, device)


def flac(q, sr, bits, flac=None, channels=None, device: int = 0):
    """The complete .flac file (uint8, 1-D) of integer audio q, (n,) or (n, channels), or of the packed
    device bytes msg_quantize wrote (give ``channels``), encoded on the device with a flac.Flac
    (block size, MD5; see flac.py): fixed predictors, Rice codes, the four stereo assignments."""
    return _flac.encode(q, sr, bits, flac, channels, device)


def quantize(x, bits=16, dither="tpdf", seed=0, key=0, device: int = 0, shape=None):
    """x, (n,) or (n, 2) float32, as 16- or 24-bit PCM quantised on the device with TPDF
    dither (or "none") from the stream (seed, key); see pcm.py.  NumPy in, int16 (or
    int32 at 24 bits, sign-extended) out in x's shape; a device tensor in, the packed
    device bytes out with no host synchronise.  ``shape``: None, or "e3", "lipshitz5" or
    "f9" for noise-shaped dither."""
    return _pcm.quantize(x, bits, dither, seed, key, device, shape)


def render_variations(base_params, seeds, unfolds, stretches, folder=None, device: int = 0, devices=None, **kw):
    """The app's batch render (on_batch, MS:1524-1596); see batch.py.  ``devices``
    shards the variants across GPUs as render_batch does; ``export_sr`` /
    ``export_peak`` deliver the variants at another sample rate, ``export_lufs`` /
    ``export_ceiling`` at a BS.1770 integrated loudness, ``export_true_peak`` under a
    ceiling in dBTP, ``export_bits`` as 16- or 24-bit PCM with TPDF dither (``export_shape``: noise-shaped), ``export_limiter`` holding
    that ceiling with the look-ahead limiter, ``export_report`` with the EBU R 128 meters of every
    delivered variant in a list and, with a folder, in loudness_report.csv, ``export_edges`` trimming,
    fading or looping every variant's ends, ``export_filter`` running every variant through a
    filter.Filter before them, ``export_stereo`` metering, shaping or folding to mono every variant's
    image with a stereo.Stereo between the two, ``export_gate`` gating every variant with a gate.Gate
    after that and ``export_dynamics`` compressing it with a dynamics.Dynamics after that, ``export_flac``
    writing FLAC files encoded on the device instead of WAVs (one device)."""
    from .batch import render_variations as _rv
    return _rv(base_params, seeds, unfolds, stretches, folder, device, devices=devices, **kw)
