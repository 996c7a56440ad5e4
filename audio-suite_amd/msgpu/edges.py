"""Silence trim, fades and loop crossfade on the device (msg_edges, DESIGN.md "4i. Edges").

Per signal: the span from the first to the last frame whose level max|x| over the channels
reaches ``trim_db`` dBFS, widened by the pads; a fade-in and a fade-out over the span's ends,
or a crossfade of the span's tail into its head for a seamless loop.  The samples are shaped
where they lie and nothing is moved: the record says which frames are delivered.  The device
and ``msg_edges_host`` agree to the bit; :func:`edges_reference` restates the definition in
float64 NumPy for the tests, and nothing on the product path uses it.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records

# csrc/edges.h
TILE = 4096              # frames per workgroup of the find kernel
APPLY_TILE = 1024        # frames per workgroup of the apply kernel
HEAD, TAIL = 1, 2
SILENT = 1
CURVES = {"linear": 0, "hann": 1, "qsin": 2}
SIDES = {"both": HEAD | TAIL, "head": HEAD, "tail": TAIL}

# msg_edges_rec as a numpy record
EDGES_DTYPE = np.dtype([(k, "<i8") for k in ("first", "last", "start", "end", "fade_in", "fade_out", "loop", "flags")])


def frames(ms, sr):
    """llround(ms sr / 1000): milliseconds as frames at ``sr`` Hz, halves away from zero."""
    v = float(ms) * float(sr) / 1000.0
    f = math.floor(v)
    return int(f) + (1 if v - f >= 0.5 else 0)


def threshold(trim_db):
    """The level a sound frame reaches: (float32)10^(trim_db / 20), formed in float64."""
    return np.float32(10.0 ** (float(trim_db) / 20.0))


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(float(v))


def _pair(v, what):
    if _number(v):
        v = (v, v)
    if not isinstance(v, (tuple, list)) or len(v) != 2 or not all(_number(a) and float(a) >= 0.0 for a in v):
        raise ValueError(f"{what} must be a number of milliseconds from 0 up, or two of them (head, tail)")
    return float(v[0]), float(v[1])


@dataclass
class Edges:
    trim_db: object = None        # dBFS a frame must reach to count as sound, finite and <= 0 (None: no trim)
    sides: str = "both"           # the ends that are trimmed: "both", "head" or "tail"
    pad_ms: object = (0, 0)       # silence kept before the first and after the last sound frame
    fade_ms: object = (0, 0)      # fade-in and fade-out over the span's ends; one number: both
    curve: str = "hann"           # "linear", "hann" or "qsin"
    loop_ms: object = None        # crossfade the span's tail into its head; excludes fades

    def check(self):
        """ValueError for a value out of range; returns self."""
        if self.trim_db is not None and (not _number(self.trim_db) or float(self.trim_db) > 0.0):
            raise ValueError("trim_db must be None or a finite number of dB, at most 0")
        if self.sides not in SIDES:
            raise ValueError("sides must be 'both', 'head' or 'tail'")
        _pair(self.pad_ms, "pad_ms")
        fi, fo = _pair(self.fade_ms, "fade_ms")
        if self.curve not in CURVES:
            raise ValueError("curve must be 'linear', 'hann' or 'qsin'")
        if self.loop_ms is not None:
            if not _number(self.loop_ms) or float(self.loop_ms) < 0.0:
                raise ValueError("loop_ms must be None or a number of milliseconds from 0 up")
            if fi > 0.0 or fo > 0.0:
                raise ValueError("loop_ms and fade_ms exclude each other: give one")
        return self

    def moves_span(self):
        """Whether the delivered span can differ from the whole signal (a trim or a loop)."""
        return self.trim_db is not None or self.loop_ms is not None

    def counts(self, sr):
        """(sides, pre, post, fade_in, fade_out, loop) in frames at ``sr`` Hz, as msg_edges_opts
        takes them: sides 0 without a trim, loop -1 without a crossfade."""
        self.check()
        sr = int(sr)
        if sr < 1:
            raise ValueError("the sample rate must be positive")
        pre, post = (frames(v, sr) for v in _pair(self.pad_ms, "pad_ms"))
        fi, fo = (frames(v, sr) for v in _pair(self.fade_ms, "fade_ms"))
        return (SIDES[self.sides] if self.trim_db is not None else 0, pre, post, fi, fo,
                -1 if self.loop_ms is None else frames(self.loop_ms, sr))

    def opts(self, sr):
        """The msg_edges_opts of these edges at ``sr`` Hz."""
        return _opts(self, self.counts(sr))


def _opts(edges, counts):
    return L.MsgEdgesOpts(0.0 if edges.trim_db is None else float(edges.trim_db), counts[0], CURVES[edges.curve], *counts[1:])


def curve_reference(curve, t):
    """c(t) of the definition in float64 NumPy."""
    t = np.asarray(t, dtype=np.float64)
    if curve == "linear":
        return t
    if curve == "hann":
        return 0.5 - 0.5 * np.cos(np.pi * t)
    if curve == "qsin":
        return np.sin(np.pi * t / 2.0)
    raise ValueError("curve must be 'linear', 'hann' or 'qsin'")


def gains_reference(curve, n):
    """(fade-in, fade-out) gains of an ``n``-frame fade as the definition has them: float64
    NumPy rounded once to float32."""
    k = np.arange(int(n), dtype=np.float64)
    t = (2.0 * k + 1.0) / (2.0 * n) if n else k
    return (curve_reference(curve, t).astype(np.float32),
            curve_reference(curve, (2.0 * (n - k) - 1.0) / (2.0 * n) if n else k).astype(np.float32))


def loop_gains_reference(curve, n):
    """(c(t), c(1 - t)) of an ``n``-frame crossfade, float64 NumPy rounded once to float32."""
    k = np.arange(int(n), dtype=np.float64)
    t = (2.0 * k + 1.0) / (2.0 * n) if n else k
    return curve_reference(curve, t).astype(np.float32), curve_reference(curve, 1.0 - t).astype(np.float32)


def gains(curve, n):
    """The library's own (fade-in, fade-out) float32 gains of an ``n``-frame fade: msg_edges_host
    over ones, whose product with a gain is the gain."""
    n = int(n)
    one = np.ones(n, dtype=np.float32)
    return (_host(one.copy(), 1, Edges(curve=curve), (0, 0, 0, n, 0, -1))[0],
            _host(one.copy(), 1, Edges(curve=curve), (0, 0, 0, 0, n, -1))[0])


def loop_gains(curve, n):
    """The library's own (c(t), c(1 - t)) float32 gains of an ``n``-frame crossfade: msg_edges_host
    over ones against zeros."""
    n = int(n)
    one, zero = np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    return (_host(np.concatenate([one, zero]), 1, Edges(curve=curve), (0, 0, 0, 0, 0, n))[0][:n],
            _host(np.concatenate([zero, one]), 1, Edges(curve=curve), (0, 0, 0, 0, 0, n))[0][:n])


def span_reference(m, thr, counts):
    """Steps 2 to 4's record from the level per frame ``m`` (the largest |x| that is a number; NaN: silence), the threshold and
    the frame counts of Edges.counts: an EDGES_DTYPE scalar."""
    sides, pre, post, fi, fo, loop = counts
    n = len(m)
    rec = np.zeros(1, dtype=EDGES_DTYPE)[0]
    if n == 0:
        return rec
    start, end = 0, n
    if not sides:
        rec["first"], rec["last"] = 0, n - 1
    else:
        with np.errstate(invalid="ignore"):
            sound = np.flatnonzero(np.asarray(m) >= thr)
        if sound.size == 0:
            rec["first"] = rec["last"] = -1
            rec["flags"] = SILENT
        else:
            first, last = int(sound[0]), int(sound[-1])
            rec["first"], rec["last"] = first, last
            if sides & HEAD:
                start = max(0, first - pre)
            if sides & TAIL:
                end = min(n, last + 1 + post)
    length = end - start
    if loop >= 0:
        x = min(loop, length // 2)
        rec["loop"] = x
        end -= x
    else:
        if fi + fo > length:
            fi = (length * fi) // (fi + fo)
            fo = length - fi
        rec["fade_in"], rec["fade_out"] = fi, fo
    rec["start"], rec["end"] = start, end
    return rec


def edges_reference(x, sr, edges, gains=gains_reference, loop_gains=loop_gains_reference):
    """The definition in NumPy: returns (y, rec), a shaped float32 copy of x (whole length:
    the span is y[rec.start:rec.end]) and the record.  ``gains`` / ``loop_gains``: where the
    float32 gains come from, the float64 definition unless the library's own are passed."""
    a, channels = _signal(x)
    y = a.copy()
    v = y.reshape(len(y), channels)
    counts = edges.counts(sr)
    thr = threshold(edges.trim_db) if counts[0] else np.float32(0)
    rec = span_reference(np.fmax.reduce(np.abs(v), axis=1) if len(v) else np.zeros(0, np.float32), thr, counts)
    s, e = int(rec["start"]), int(rec["end"])
    if rec["loop"]:
        n = int(rec["loop"])
        ga, gb = loop_gains(edges.curve, n)
        v[s:s + n] = (v[s:s + n].astype(np.float64) * ga.astype(np.float64)[:, None] +
                      v[e:e + n].astype(np.float64) * gb.astype(np.float64)[:, None]).astype(np.float32)
    if rec["fade_in"]:
        n = int(rec["fade_in"])
        v[s:s + n] = (v[s:s + n].astype(np.float64) * gains(edges.curve, n)[0].astype(np.float64)[:, None]).astype(np.float32)
    if rec["fade_out"]:
        n = int(rec["fade_out"])
        v[e - n:e] = (v[e - n:e].astype(np.float64) * gains(edges.curve, n)[1].astype(np.float64)[:, None]).astype(np.float32)
    return y, rec


def _signal(x):
    a = np.array(x, dtype=np.float32, order="C")
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
        raise ValueError("x must be (n,) or (n, 2)")
    return a, 1 if a.ndim == 1 else int(a.shape[1])


def _host(y, channels, edges, counts):
    """msg_edges_host over y in place with the frame counts given; returns (y, rec)."""
    opts = _opts(edges, counts)
    rec = np.zeros(1, dtype=EDGES_DTYPE)
    L.check(L.lib().msg_edges_host(y.ctypes.data_as(C.c_void_p), channels, int(y.shape[0]), C.byref(opts),
                                   rec.ctypes.data_as(C.c_void_p)), None)
    return y, rec[0]


def edges_host(x, sr, edges):
    """msg_edges_host: the library's loop on the host (no device), the device's arithmetic to
    the bit.  Returns (y, rec): a shaped float32 copy of x (whole length: the span is
    y[rec.start:rec.end]) and the record (an EDGES_DTYPE scalar)."""
    a, channels = _signal(x)
    return _host(a.copy(), channels, edges, edges.counts(sr))


def records(rec):
    """Device records (Engine.edges) as an EDGES_DTYPE array on the host; waits for them."""
    return read_records(rec, EDGES_DTYPE)


def edges(x, sr, edges, device: int = 0):
    """Shape the ends of x, (n,) mono or (n, 2) stereo at ``sr`` Hz, on the device.  NumPy in:
    (the shaped span as a new float32 array, its record).  A device tensor in: shaped in
    place where it lies, enqueued on the current stream (no host synchronise); returns the
    device record tensor (edges.records reads it), whose start and end say what is delivered."""
    from .engine import default_engine

    edges.check()
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x, in_place=True)
    rec = eng.edges(t, [0], [int(t.shape[0])], channels, int(sr), edges)
    if not on_host:
        return rec
    r = records(rec)[0]
    return t.cpu().numpy()[int(r["start"]):int(r["end"])].copy(), r
