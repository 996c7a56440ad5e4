"""Loudness range and maximum momentary / short-term loudness on the device
(msg_loudness_range, DESIGN.md "Loudness range").

EBU Tech 3341 / 3342 on top of loudness.py's K-weighting: the 100 ms hop sums of the
K-weighted signal give momentary blocks (400 ms, msg_loudness's own) and short-term
windows (3 s, one per 100 ms); the loudness range is the 95th minus the 10th percentile
(nearest rank) of the short-term windows above -70 LUFS and above 20 LU under their
mean.  csrc/lrange.h states the definition; :func:`lrange_reference` restates it in
float64 NumPy for the tests, and nothing on the product path uses it.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records
from .loudness import LOUDNESS_DTYPE, _biquad, _check_rate, kweight

BLOCK_HOPS = 4          # momentary: 400 ms
WINDOW_HOPS = 30        # short-term: 3 s
ABS_GATE = -70.0
REL_GATE = 20.0

# msg_lrange_rec as a numpy record
LRANGE_DTYPE = np.dtype([(k, "<f8") for k in ("lra", "lo", "hi", "max_momentary", "max_short", "gate", "z_lo", "z_hi",
                                              "z_max_m", "z_max_s")] +
                        [(k, "<i4") for k in ("n_momentary", "n_short", "n_abs", "n_kept")])


def _level(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def _fold(H, width, hop):
    """Every window of ``width`` (> 1) hop sums as the left fold of shifted slices, over width * hop
    frames; H a NumPy array or a tensor."""
    n = int(H.shape[0]) - (width - 1)
    if n <= 0:
        return H[:0]
    w = H[0:n] + H[1:n + 1]
    for k in range(2, width):
        w = w + H[k:k + n]
    return w / (float(width) * float(hop))


def hop_sums_reference(x, sr):
    """The K-weighted energy of every complete 100 ms hop of x, (n,) or (n, channels), in float64 NumPy."""
    sr = _check_rate(sr)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    hop = sr // 10
    hops = x.shape[0] // hop
    if hops == 0:
        return np.zeros(0)
    (b1, a1), (b2, a2) = kweight(sr)
    e = np.zeros(hops * hop)
    for c in range(x.shape[1]):
        y = _biquad(b2, a2, _biquad(b1, a1, x[:hops * hop, c]))
        e += y * y
    return e.reshape(hops, hop).sum(axis=1)


def hops_reference(H, hop):
    """The definition from given hop sums in float64 NumPy: a dict with msg_lrange_rec's fields
    and ``margin``, the smallest distance in LU of a short-term level to either gate (inf
    when there is no finite level)."""
    H = np.asarray(H, dtype=np.float64)
    zm = _fold(H, BLOCK_HOPS, hop)
    zs = _fold(H, WINDOW_HOPS, hop)
    S = _level(zs)
    k1 = S > ABS_GATE
    c1 = int(k1.sum())
    gate = float(_level(zs[k1].mean())) - REL_GATE if c1 else -math.inf
    k2 = k1 & (S > gate)
    c2 = int(k2.sum())
    fin = S[np.isfinite(S)]
    margin = math.inf
    if fin.size:
        margin = float(np.min(np.abs(fin - ABS_GATE)))
        if c1:
            margin = min(margin, float(np.min(np.abs(fin - gate))))
    r = {"z_max_m": float(zm.max()) if zm.size else 0.0, "z_max_s": float(zs.max()) if zs.size else 0.0,
         "gate": gate, "n_momentary": int(zm.size), "n_short": int(zs.size), "n_abs": c1, "n_kept": c2,
         "margin": margin}
    r["max_momentary"] = float(_level(r["z_max_m"])) if zm.size else -math.inf
    r["max_short"] = float(_level(r["z_max_s"])) if zs.size else -math.inf
    if c2:
        kept = np.sort(zs[k2])
        r["z_lo"] = float(kept[((c2 - 1) * 10 + 50) // 100])
        r["z_hi"] = float(kept[((c2 - 1) * 95 + 50) // 100])
        r["lo"], r["hi"] = float(_level(r["z_lo"])), float(_level(r["z_hi"]))
        r["lra"] = r["hi"] - r["lo"]
    else:
        r.update(z_lo=0.0, z_hi=0.0, lo=-math.inf, hi=-math.inf, lra=0.0)
    return r


def lrange_reference(x, sr):
    """The definition in float64 NumPy over x, (n,) or (n, channels): hops_reference of its hop sums."""
    return hops_reference(hop_sums_reference(x, sr), _check_rate(sr) // 10)


def curves_reference(x, sr):
    """(momentary, short_term) levels of x at ten per second, in float64 NumPy."""
    H, hop = hop_sums_reference(x, sr), int(sr) // 10
    return _level(_fold(H, BLOCK_HOPS, hop)), _level(_fold(H, WINDOW_HOPS, hop))


def _signal(x):
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
        raise ValueError("x must be (n,) or (n, 2)")
    return a, (1 if a.ndim == 1 else int(a.shape[1]))


def lrange_hops_host(hops, hop):
    """msg_lrange_hops_host: the library's plain C++ over given hop sums of ``hop`` frames each
    (no device); returns the record (a LRANGE_DTYPE scalar)."""
    H = np.ascontiguousarray(hops, dtype=np.float64)
    if H.ndim != 1:
        raise ValueError("hops must be 1-D")
    rec = np.zeros(1, dtype=LRANGE_DTYPE)
    L.check(L.lib().msg_lrange_hops_host(H.ctypes.data_as(C.c_void_p), int(H.size), int(hop),
                                         rec.ctypes.data_as(C.c_void_p)), None)
    return rec[0]


def lrange_host(x, sr, loudness=False):
    """msg_loudness_range_host: msg_loudness_host's loop and the hop sums' record on the host
    (no device); returns the LRANGE_DTYPE record, with ``loudness`` the LOUDNESS_DTYPE one too."""
    a, channels = _signal(x)
    rec = np.zeros(1, dtype=LRANGE_DTYPE)
    loud = np.zeros(1, dtype=LOUDNESS_DTYPE)
    L.check(L.lib().msg_loudness_range_host(a.ctypes.data_as(C.c_void_p), channels, int(a.shape[0]), int(sr),
                                            loud.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)), None)
    return (rec[0], loud[0]) if loudness else rec[0]


def records(rec):
    """Device records (Engine.loudness_range's second tensor) as a LRANGE_DTYPE array on the
    host; waits for them."""
    return read_records(rec, LRANGE_DTYPE)


def loudness_range(x, sr, device: int = 0):
    """The delivery meters of x, (n,) mono or (n, 2) stereo, at ``sr`` Hz, measured on the
    device: a dict with ``lufs`` (integrated loudness), ``lra``, ``lo``, ``hi``,
    ``max_momentary``, ``max_short`` and ``gate``.  NumPy in, floats out (and the counts
    n_momentary, n_short, n_abs, n_kept as ints); a device tensor in, one-element device
    tensors out, views of the device records, enqueued on the current stream (no host
    synchronise)."""
    from .engine import default_engine
    from .loudness import records as loud_records

    sr = _check_rate(sr)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x)
    loud, rng = eng.loudness_range(t, [0], [int(t.shape[0])], channels, sr)
    names = ("lra", "lo", "hi", "max_momentary", "max_short", "gate")
    if not on_host:
        out = {"lufs": loud[0, :1]}
        out.update({k: rng[0, i:i + 1] for i, k in enumerate(names)})
        return out
    r = records(rng)[0]
    out = {"lufs": float(loud_records(loud)["lufs"][0])}
    out.update({k: float(r[k]) for k in names})
    out.update({k: int(r[k]) for k in ("n_momentary", "n_short", "n_abs", "n_kept")})
    return out


def loudness_curves(x, sr, device: int = 0):
    """(momentary, short_term): the levels in LUFS of every 400 ms block and of every 3 s
    window of x, ten per second, from the hop sums the device measures, each the left fold
    of shifted slices the record's maxima are formed from.  NumPy in, float64 NumPy out; a
    device tensor in, float64 device tensors out with no host synchronise."""
    from .engine import default_engine

    sr = _check_rate(sr)
    eng = default_engine(device)
    torch = eng.torch
    t, channels, on_host = device_signal(eng, x)
    H = eng.loudness_range(t, [0], [int(t.shape[0])], channels, sr, hops=True)[2]
    hop = sr // 10
    if on_host:
        H = H.cpu().numpy()
        return _level(_fold(H, BLOCK_HOPS, hop)), _level(_fold(H, WINDOW_HOPS, hop))
    return tuple(-0.691 + 10.0 * torch.log10(_fold(H, w, hop)) for w in (BLOCK_HOPS, WINDOW_HOPS))
