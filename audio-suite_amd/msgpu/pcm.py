"""Fixed-point PCM export with TPDF dither (msg_quantize).

A float32 render becomes 16- or 24-bit PCM where it lies in HBM: word ``w`` of a signal
(``w = frame * channels + c``) is scaled by ``S = 2**(bits - 1)`` in float64, gets one
triangular dither value ``d(seed, key, w)`` in (-1, 1) LSB, is rounded to nearest (ties to
even) and clamped to ``[-S, S - 1]``; the words are packed little-endian with no padding.
The dither is a counter-based hash of ``(seed, key, w)`` alone, so a signal's bytes do
not depend on the batch it is quantised in.  The device and ``msg_quantize_host`` agree
to the bit; :func:`quantize_reference` restates the definition in NumPy for the tests,
and nothing on the product path uses it.

``shape`` ("e3", "lipshitz5", "f9") adds noise shaping (msg_quantize_shaped):
the total error of each word, dither included, is fed back through the shape's taps, one
chain per channel from the signal's first word to its last, which moves the 16-bit floor
out of the band where the ear is most sensitive.  :func:`quantize_shaped_host` and
:func:`quantize_shaped_reference` are its host loop and its NumPy restatement.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _lib as L
from ._signal import device_signal, read_records

# csrc/pcm.h
G = 0x9E3779B97F4A7C15
TILE = 4096
DITHER = {"none": 0, "tpdf": 1}
# csrc/pcm_shape.h: a shape's code (MSG_SHAPE_*) and its integer taps H_k = -llround(c_k 65536)
SHAPES = {
    "e3": (1, (-106365, 64356, -7143)),
    "lipshitz5": (2, (-133235, 141885, -128385, 104202, -40298)),
    "f9": (3, (-158073, 220856, -258015, 273547, -219742, 144507, -83952, 37290, -5551)),
}
SHAPE_CHUNK = 32

# msg_pcm_rec as a numpy record
PCM_DTYPE = np.dtype([("clipped", "<i8"), ("nan", "<i8"), ("q_min", "<i4"), ("q_max", "<i4"),
                      ("bits", "<i4"), ("dither", "<i4")])

_M64 = (1 << 64) - 1


def dither_code(dither):
    """"none" / "tpdf" (or MSG_DITHER_NONE / MSG_DITHER_TPDF) as the ABI's code."""
    if isinstance(dither, str) and dither in DITHER:
        return DITHER[dither]
    if not isinstance(dither, (str, bool)) and dither in (0, 1):
        return int(dither)
    raise ValueError("dither must be 'tpdf' or 'none'")


def shape_code(shape):
    """"e3" / "lipshitz5" / "f9" (or MSG_SHAPE_E3 / _LIPSHITZ5 / _F9) as the ABI's code."""
    if isinstance(shape, str) and shape in SHAPES:
        return SHAPES[shape][0]
    if not isinstance(shape, (str, bool)) and shape in (1, 2, 3):
        return int(shape)
    raise ValueError("shape must be 'e3', 'lipshitz5' or 'f9'")


def shape_taps(shape):
    """The integer taps H_1 .. H_K of a shape (int64)."""
    code = shape_code(shape)
    return np.array(next(h for c, h in SHAPES.values() if c == code), dtype=np.int64)


def check_bits(bits):
    if bits not in (16, 24) or isinstance(bits, bool):
        raise ValueError("bits must be 16 or 24")
    return int(bits)


def _fmix64(h):
    """MurmurHash3's finaliser on a uint64 array (dg_fmix64 of csrc/digest.h)."""
    h = np.array(h, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    return h


def stream_key(seed, key):
    """k = fmix64(seed ^ fmix64(key + G)), as a Python int."""
    inner = int(_fmix64([(int(key) + G) & _M64])[0])
    return int(_fmix64([(int(seed) & _M64) ^ inner])[0])


def dither_int(seed, key, w):
    """a - b of the dither stream at the word indices ``w`` (int64, |a - b| < 2^24): the
    dither in units of 2^-24 LSB."""
    w = np.asarray(w).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = _fmix64(np.uint64(stream_key(seed, key)) + (w + np.uint64(1)) * np.uint64(G))
    a = (h & np.uint64(0xFFFFFF)).astype(np.int64)
    b = ((h >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.int64)
    return a - b


def dither(seed, key, w):
    """The dither values d(seed, key, w) of the word indices ``w`` (float64, exact
    multiples of 2^-24 in (-1, 1))."""
    return dither_int(seed, key, w).astype(np.float64) * 2.0 ** -24


_dither_values = dither          # the functions below take a parameter named ``dither``


def _signal(x):
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
        raise ValueError("x must be (n,) or (n, 2)")
    return a, (1 if a.ndim == 1 else int(a.shape[1]))


def int_dtype(bits):
    """The integer type quantised audio is returned in: int16, or int32 (sign-extended) at 24 bits."""
    return np.int16 if check_bits(bits) == 16 else np.int32


def quantize_reference(x, bits, dither="tpdf", seed=0, key=0):
    """The definition in NumPy: ``(q, rec)`` with q in x's shape (int16, or int32 at 24
    bits) and rec a PCM_DTYPE scalar."""
    bits = check_bits(bits)
    code = dither_code(dither)
    a, _ = _signal(x)
    S = float(1 << (bits - 1))
    flat = a.reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = flat.astype(np.float64) * S
        if code:
            v = v + _dither_values(seed, key, np.arange(flat.size, dtype=np.uint64))
        nan = np.isnan(v)
        r = np.rint(v)
        clipped = (r < -S) | (r > S - 1)
        q = np.where(nan, 0.0, np.clip(r, -S, S - 1)).astype(np.int64)
    rec = np.zeros(1, dtype=PCM_DTYPE)
    rec["clipped"], rec["nan"] = int(clipped.sum()), int(nan.sum())
    if flat.size:
        rec["q_min"], rec["q_max"] = int(q.min()), int(q.max())
    rec["bits"], rec["dither"] = bits, code
    return q.astype(int_dtype(bits)).reshape(a.shape), rec[0]


def pack24(q):
    """int32 values in [-2^23, 2^23) as packed little-endian 3-byte words (uint8, 3 x size)."""
    q = np.ascontiguousarray(q, dtype="<i4")
    return np.ascontiguousarray(q.reshape(-1, 1).view(np.uint8)[:, :3]).reshape(-1)


def unpack24(b):
    """Packed little-endian 3-byte words as sign-extended int32."""
    b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, 3)
    out = np.zeros((b.shape[0], 4), dtype=np.uint8)
    out[:, 1:] = b
    return out.view("<i4").reshape(-1) >> 8


def pack(q, bits):
    """Integer audio as the bytes of its file (uint8, 1-D)."""
    if check_bits(bits) == 16:
        return np.ascontiguousarray(q, dtype="<i2").reshape(-1).view(np.uint8)
    return pack24(q)


def unpack(b, bits, shape=None):
    """Packed bytes as integer audio (int16, or int32 at 24 bits), reshaped to ``shape``."""
    b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
    q = b.view("<i2").copy() if check_bits(bits) == 16 else unpack24(b)
    return q if shape is None else q.reshape(shape)


def quantize_host(x, bits, dither="tpdf", seed=0, key=0):
    """msg_quantize_host: the library's loop on the host (no device), the device's bytes
    to the bit; returns ``(q, rec)`` as quantize_reference does."""
    bits = check_bits(bits)
    code = dither_code(dither)
    a, channels = _signal(x)
    out = np.zeros(a.size * (bits // 8), dtype=np.uint8)
    rec = np.zeros(1, dtype=PCM_DTYPE)
    L.check(L.lib().msg_quantize_host(a.ctypes.data_as(C.c_void_p), channels, int(a.shape[0]), bits, code,
                                      C.c_uint64(int(seed) & _M64), C.c_uint64(int(key) & _M64),
                                      out.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)), None)
    return unpack(out, bits, a.shape), rec[0]


def quantize_shaped_reference(xs, bits, dither="tpdf", shape="f9", seed=0, keys=None):
    """The noise-shaped quantiser's definition (csrc/pcm_shape.h) in NumPy, for the tests:
    a Python loop over the frames, vectorised over the channel runs of the signals ``xs``
    (a list; signal i takes the stream (seed, keys[i]), keys None: key = i).  Returns
    ``(qs, recs, max_e)``: per signal q and rec as quantize_reference gives them, and the
    largest |E| fed back in any run."""
    bits = check_bits(bits)
    code = dither_code(dither)
    H = shape_taps(shape)
    K = H.size
    S = float(1 << (bits - 1))
    sig = [_signal(x) for x in xs]
    keys = list(range(len(sig))) if keys is None else list(keys)
    runs = [(i, c) for i, (a, ch) in enumerate(sig) for c in range(ch)]
    nf = max([a.shape[0] for a, _ in sig], default=0)
    V = np.zeros((len(runs), nf), dtype=np.float64)           # v = x S, exact
    D = np.zeros((len(runs), nf), dtype=np.int64)
    n = np.zeros(len(runs), dtype=np.int64)
    for row, (i, c) in enumerate(runs):
        a, ch = sig[i]
        f = a.shape[0]
        n[row] = f
        V[row, :f] = a.reshape(f, ch)[:, c].astype(np.float64) * S
        if code:
            D[row, :f] = dither_int(seed, keys[i], np.arange(f, dtype=np.uint64) * np.uint64(ch) + np.uint64(c))
    Rr = np.zeros((len(runs), nf), dtype=np.float64)           # r of every word
    E = np.zeros((len(runs), K), dtype=np.int64)
    max_e = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(nf):
            A = E @ H
            F = (A + 32768) >> 16
            d = D[:, f]
            y = V[:, f] + (F + d).astype(np.float64) * 2.0 ** -24
            r = np.rint(y)
            none = np.isnan(y) | (r < -S) | (r > S - 1)
            t = np.where(none, 0.0, (r - y) * 2.0 ** 24)
            e = np.where(f < n, np.rint(t).astype(np.int64) + np.where(none, 0, d), 0)
            E[:, 1:] = E[:, :-1].copy()
            E[:, 0] = e
            max_e = max(max_e, int(np.abs(e).max()))
            Rr[:, f] = r
        nan = np.isnan(Rr)
        clipped = (Rr < -S) | (Rr > S - 1)
        Q = np.where(nan, 0.0, np.clip(Rr, -S, S - 1)).astype(np.int64)
    qs, recs = [], []
    for i, (a, ch) in enumerate(sig):
        rows = [row for row, (j, _) in enumerate(runs) if j == i]
        f = a.shape[0]
        q = np.stack([Q[row, :f] for row in rows], axis=1)
        rec = np.zeros(1, dtype=PCM_DTYPE)
        rec["clipped"] = sum(int(clipped[row, :f].sum()) for row in rows)
        rec["nan"] = sum(int(nan[row, :f].sum()) for row in rows)
        if q.size:
            rec["q_min"], rec["q_max"] = int(q.min()), int(q.max())
        rec["bits"], rec["dither"] = bits, code
        qs.append(q.astype(int_dtype(bits)).reshape(a.shape))
        recs.append(rec[0])
    return qs, recs, max_e


def quantize_shaped_host(x, bits, dither="tpdf", shape="f9", seed=0, key=0):
    """msg_quantize_shaped_host: the library's error-feedback loop on the host (no device),
    the device's bytes to the bit; returns ``(q, rec)`` as quantize_host does."""
    bits = check_bits(bits)
    code = dither_code(dither)
    scode = shape_code(shape)
    a, channels = _signal(x)
    out = np.zeros(a.size * (bits // 8), dtype=np.uint8)
    rec = np.zeros(1, dtype=PCM_DTYPE)
    L.check(L.lib().msg_quantize_shaped_host(a.ctypes.data_as(C.c_void_p), channels, int(a.shape[0]), bits, code, scode,
                                             C.c_uint64(int(seed) & _M64), C.c_uint64(int(key) & _M64),
                                             out.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)), None)
    return unpack(out, bits, a.shape), rec[0]


def records(rec):
    """Device records (Engine.quantize) as a PCM_DTYPE array on the host; waits for them."""
    return read_records(rec, PCM_DTYPE)


def write_wav_pcm(path, q, sr, bits):
    """Integer-PCM WAV (WAVE_FORMAT_PCM, tag 1, a 16-byte fmt chunk, no fact chunk: what
    libsndfile writes for PCM_16 / PCM_24), frames x channels; an odd-sized data chunk is
    followed by its pad byte."""
    bits = check_bits(bits)
    a = np.asarray(q)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.dtype.kind != "i":
        raise ValueError("q must be integer audio, (n,) or (n, channels)")
    frames, ch = a.shape
    by = bits // 8
    data_bytes = frames * ch * by
    pad = data_bytes & 1
    riff_size = 4 + (8 + 16) + (8 + data_bytes + pad)
    if riff_size > 0xFFFFFFFF:
        raise ValueError("WAV data beyond 4 GiB")
    S = 1 << (bits - 1)
    if a.size and (int(a.min()) < -S or int(a.max()) > S - 1):
        raise ValueError(f"q exceeds {bits} bits")
    fmt = struct.pack("<HHIIHH", 1, ch, int(sr), int(sr) * ch * by, ch * by, bits)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", riff_size) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", data_bytes))
        pack(a, bits).tofile(f)
        if pad:
            f.write(b"\0")


def read_wav_pcm(path):
    """Reader for the files write_wav_pcm makes: (frames x channels int16 or int32, sr, bits)."""
    with open(path, "rb") as f:
        b = f.read()
    if b[:4] != b"RIFF" or b[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    pos, ch, sr, bits, data = 12, None, None, None, None
    while pos + 8 <= len(b):
        tag, size = b[pos:pos + 4], struct.unpack("<I", b[pos + 4:pos + 8])[0]
        body = b[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            tagv, ch, sr, _, _, bits = struct.unpack("<HHIIHH", body[:16])
            if tagv != 1 or bits not in (16, 24):
                raise ValueError("not a 16- or 24-bit integer PCM WAV")
        elif tag == b"data":
            data = np.frombuffer(body, dtype=np.uint8)
        pos += 8 + size + (size & 1)
    if ch is None or data is None:
        raise ValueError("missing fmt or data chunk")
    return unpack(data, bits).reshape(-1, ch), sr, bits


def quantize(x, bits=16, dither="tpdf", seed=0, key=0, device: int = 0, shape=None):
    """x, (n,) mono or (n, 2) stereo float32, as ``bits``-bit PCM quantised on the device.
    NumPy in: int16 (16 bits) or int32 (24 bits, sign-extended) out, in x's shape.  A
    device tensor in: the packed device bytes (uint8, n * channels * bits / 8) out,
    enqueued on the current stream (no host synchronise).  ``shape``: None, or "e3",
    "lipshitz5" or "f9" for noise-shaped dither (msg_quantize_shaped)."""
    from .engine import default_engine

    bits = check_bits(bits)
    dither_code(dither)
    if shape is not None:
        shape_code(shape)
    eng = default_engine(device)
    t, channels, on_host = device_signal(eng, x)
    out, _, _ = eng.quantize(t, [0], [int(t.shape[0])], channels, bits, dither, seed, [key], shape=shape)
    if not on_host:
        return out
    return unpack(out.cpu().numpy(), bits, tuple(t.shape))
