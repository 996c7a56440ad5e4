"""The stereo image of renders on the device (msg_stereo_meter, msg_stereo; DESIGN.md "4k. Stereo").

The meter is the phase-correlation meter of broadcast QC: over the L/R frames of a signal, in
float64, ``sll = sum L^2``, ``srr = sum R^2``, ``slr = sum L R`` and ``corr = slr / sqrt(sll srr)``,
then the same correlation over every 400 ms block (the loudness meter's blocks, hop = sr / 10)
whose mean square per channel lies above -70 dBFS, of which the smallest and its index are kept.
From the three sums follow what a fold-down to mono costs (``mono_db``), the channel balance
(``balance_db``) and the side-to-mid ratio (``side_db``).

The image is one 2 x 2 matrix over every frame, in place, or one row that folds the two channels
into a mono buffer.  A ``Stereo`` says what is wanted: a width (0 mono, 1 as it is, 2 the side
doubled), a balance in dB, a channel swap, a polarity inversion, and mono delivery.
``invert="auto"`` inverts the right channel of exactly those signals whose measured correlation
is negative, on the device, from the meter's record.  The arithmetic is csrc/image.h's: the
product ``m01 R`` rounded to float32, then one fused multiply-add, the same bits on host and device.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records
from .loudness import _check_rate

TILE = 4096              # csrc/image.h: frames per workgroup; a tile never straddles a hop
WIDTH_MAX = 4.0
GATE = 1e-7              # a kept block's mean square per channel lies above this (-70 dBFS)

# msg_stereo_rec as a numpy record (the counts and the index are float64 too)
STEREO_DTYPE = np.dtype([(k, "<f8") for k in ("sll", "srr", "slr", "corr", "corr_min", "corr_min_block", "blocks_kept",
                                              "blocks")])
# records(): the record and what follows from its three sums
STEREO_ROW_DTYPE = np.dtype(STEREO_DTYPE.descr + [(k, "<f8") for k in ("balance_db", "mono_db", "side_db")])


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(float(v))


def _db(num, den):
    """10 log10(num / den) of arrays: -inf for 0 / x, +inf for x / 0, nan for 0 / 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(np.maximum(num, 0.0) / den)


def derive(rec):
    """A STEREO_DTYPE array with the derived columns, computed on the host from the three sums:
    ``balance_db = 10 log10(srr / sll)``, ``mono_db = 10 log10((sll + srr + 2 slr) / (2 (sll + srr)))``
    (0 for L = R, -3.01 for uncorrelated channels, -inf for L = -R) and
    ``side_db = 10 log10((sll + srr - 2 slr) / (sll + srr + 2 slr))``."""
    rec = np.asarray(rec, dtype=STEREO_DTYPE)
    out = np.zeros(rec.shape, dtype=STEREO_ROW_DTYPE)
    for k in STEREO_DTYPE.names:
        out[k] = rec[k]
    sll, srr, slr = rec["sll"], rec["srr"], rec["slr"]
    out["balance_db"] = _db(srr, sll)
    out["mono_db"] = _db(sll + srr + 2.0 * slr, 2.0 * (sll + srr))
    out["side_db"] = _db(sll + srr - 2.0 * slr, sll + srr + 2.0 * slr)
    return out


def records(rec):
    """Device records (Engine.stereo_meter) as a STEREO_ROW_DTYPE array on the host, the derived
    columns added; waits for them."""
    return derive(read_records(rec, STEREO_DTYPE))


@dataclass
class Stereo:
    width: object = 1.0           # 0 .. 4: [[a, b], [b, a]], a = (1 + w) / 2, b = (1 - w) / 2
    balance_db: object = 0.0      # positive turns the left channel down by that many dB, negative the right
    swap: bool = False            # exchange the channels
    invert: object = None         # None, "left", "right" or "auto" (the right channel where corr < 0)
    channels: int = 2             # 2, or 1: fold to mono, 0.5 (row0 + row1)
    matrix: object = None         # a raw 2 x 2 instead of width, balance_db, swap and invert
    meter: object = None          # None, or a list that gets one records() row per render

    def check(self):
        """ValueError for a value out of range.  Returns self."""
        if not _number(self.width) or not 0.0 <= float(self.width) <= WIDTH_MAX:
            raise ValueError(f"width must be a number from 0 to {WIDTH_MAX:g}")
        if not _number(self.balance_db):
            raise ValueError("balance_db must be a finite number of dB")
        if not isinstance(self.swap, (bool, np.bool_)):
            raise ValueError("swap must be True or False")
        if self.invert not in (None, "left", "right", "auto"):
            raise ValueError("invert must be None, 'left', 'right' or 'auto'")
        if isinstance(self.channels, bool) or self.channels not in (1, 2):
            raise ValueError("channels must be 2 or 1")
        if self.matrix is not None:
            try:
                m = np.array(self.matrix, dtype=np.float64)
            except (TypeError, ValueError):
                m = None
            if m is None or m.shape != (2, 2) or not np.all(np.isfinite(m)) or \
                    np.max(np.abs(m)) > float(np.finfo(np.float32).max):
                raise ValueError("matrix must be a finite 2 x 2")
            if float(self.width) != 1.0 or float(self.balance_db) != 0.0 or self.swap or self.invert is not None:
                raise ValueError("matrix stands instead of width, balance_db, swap and invert: give one")
        if self.meter is not None and not isinstance(self.meter, list):
            raise ValueError("meter must be None or a list")
        return self

    def metering(self):
        """Whether the rule measures before it applies: a meter list, or the polarity taken from the record."""
        return self.meter is not None or self.invert == "auto"

    def matrix64(self):
        """The 2 x 2 in float64: ``matrix``, or M = G W P D, where the input meets D, the polarity
        inversion, first, then P, the swap, W, the width, and G, the balance ("auto": D is the
        device's, from each signal's record)."""
        self.check()
        if self.matrix is not None:
            return np.array(self.matrix, dtype=np.float64)
        D = np.diag([-1.0 if self.invert == "left" else 1.0, -1.0 if self.invert == "right" else 1.0])
        P = np.array([[0.0, 1.0], [1.0, 0.0]]) if self.swap else np.eye(2)
        w = float(self.width)
        a, b = (1.0 + w) / 2.0, (1.0 - w) / 2.0
        W = np.array([[a, b], [b, a]])
        bal = float(self.balance_db)
        G = np.diag([10.0 ** (-bal / 20.0) if bal > 0.0 else 1.0, 10.0 ** (bal / 20.0) if bal < 0.0 else 1.0])
        return G @ W @ P @ D

    def matrix_at(self):
        """(M, fold): the float32 2 x 2 the library takes, rounded once from float64, and the fold
        row 0.5 (row0 + row1) of the float64 matrix, rounded once, that ``channels=1`` delivers."""
        m = self.matrix64()
        return m.astype(np.float32), (0.5 * (m[0] + m[1])).astype(np.float32)


def _stereo_signal(x):
    a = np.array(x, dtype=np.float32, order="C")
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("x must be (n, 2)")
    return a


def _rec_arg(rec):
    if rec is None:
        return None, None
    r = np.zeros(1, dtype=STEREO_DTYPE)
    for k in STEREO_DTYPE.names:
        r[k] = rec[k]
    return r, r.ctypes.data_as(C.c_void_p)


def stereo_meter_host(x, sr):
    """msg_stereo_meter_host: the library's sequential float64 loop on the host (no device);
    returns the record (a STEREO_DTYPE scalar)."""
    a = _stereo_signal(x)
    rec = np.zeros(1, dtype=STEREO_DTYPE)
    L.check(L.lib().msg_stereo_meter_host(a.ctypes.data_as(C.c_void_p), 2, int(a.shape[0]), int(sr),
                                          rec.ctypes.data_as(C.c_void_p)), None)
    return rec[0]


def stereo_host(x, stereo, rec=None):
    """msg_stereo_host: the image on the host (no device), the device's bits.  Returns a float32
    copy, (n, 2), or (n, 1) for ``channels=1``; ``rec``: the signal's meter record, whose
    ``corr < 0`` inverts the right channel first (what ``invert="auto"`` does on the device)."""
    a = _stereo_signal(x)
    m, fold = stereo.matrix_at()
    m = np.ascontiguousarray(m.reshape(4))
    keep, rp = _rec_arg(rec)
    if stereo.channels == 1:
        y = np.zeros((a.shape[0], 1), dtype=np.float32)
        L.check(L.lib().msg_stereo_host(a.ctypes.data_as(C.c_void_p), 2, int(a.shape[0]), m.ctypes.data_as(C.c_void_p),
                                        fold.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), rp), None)
        return y
    L.check(L.lib().msg_stereo_host(a.ctypes.data_as(C.c_void_p), 2, int(a.shape[0]), m.ctypes.data_as(C.c_void_p), None,
                                    None, rp), None)
    return a


def meter_reference(x, sr):
    """The definition in float64 with ``math.fsum`` on the exact products, for the tests: a dict
    of the record's fields and ``rho``, ``energy``, the kept-or-not blocks' correlations and
    SLL + SRR.  Nothing on the product path uses it."""
    sr = _check_rate(sr)
    v = _stereo_signal(x).astype(np.float64)
    n, hop = v.shape[0], sr // 10
    ll, rr, lr = v[:, 0] * v[:, 0], v[:, 1] * v[:, 1], v[:, 0] * v[:, 1]
    sll, srr, slr = math.fsum(ll), math.fsum(rr), math.fsum(lr)
    nb = 0 if n < 4 * hop else (n - 4 * hop) // hop + 1
    rho, energy = np.full(nb, np.nan), np.zeros(nb)
    for j in range(nb):
        s = slice(j * hop, j * hop + 4 * hop)
        bll, brr, blr = math.fsum(ll[s]), math.fsum(rr[s]), math.fsum(lr[s])
        energy[j] = bll + brr
        if bll > 0.0 and brr > 0.0 and bll + brr > 8.0 * hop * GATE:
            rho[j] = blr / math.sqrt(bll * brr)
    kept = ~np.isnan(rho)
    corr = slr / math.sqrt(sll * srr) if sll > 0.0 and srr > 0.0 else 0.0
    at = int(np.nanargmin(rho)) if kept.any() else -1
    return dict(sll=sll, srr=srr, slr=slr, corr=corr, corr_min=float(rho[at]) if at >= 0 else corr, corr_min_block=at,
                blocks_kept=int(kept.sum()), blocks=nb, rho=rho, energy=energy)


def stereo_meter(x, sr, device: int = 0):
    """The stereo meter of x, (n, 2), at ``sr`` Hz, measured on the device.  NumPy in: the record
    with the derived columns (a STEREO_ROW_DTYPE scalar) out; a device tensor in: the (1, 8)
    float64 device record out, enqueued on the current stream (no host synchronise)."""
    from .engine import default_engine

    sr = _check_rate(sr)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x)
    if channels != 2:
        raise ValueError("x must be (n, 2)")
    rec = eng.stereo_meter(t, [0], [int(t.shape[0])], sr)
    return records(rec)[0] if on_host else rec


def stereo(x, sr, stereo, device: int = 0):
    """Apply a ``Stereo`` to x, (n, 2) at ``sr`` Hz, on the device: (n, 2), or (n, 1) for
    ``channels=1``.  NumPy in: a float32 array out.  A device tensor in: shaped in place where it
    lies (a fold: into a new tensor), enqueued on the current stream and returned.  The signal is
    metered first when ``stereo.meter`` is a list (it gets the row; that waits for it) or
    ``invert="auto"`` (nothing returns to the host between measuring and repairing)."""
    from .engine import default_engine

    stereo.check()
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x, in_place=True)
    if channels != 2:
        raise ValueError("x must be (n, 2)")
    rec = None
    if stereo.metering():
        rec = eng.stereo_meter(t, [0], [int(t.shape[0])], _check_rate(sr))
    y, _ = eng.stereo(t, [0], [int(t.shape[0])], stereo, rec=rec if stereo.invert == "auto" else None)
    if stereo.meter is not None:
        stereo.meter.extend(records(rec))
    return y.cpu().numpy() if on_host else y
