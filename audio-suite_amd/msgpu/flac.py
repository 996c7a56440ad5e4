"""FLAC delivery: lossless frames encoded on the device (msg_flac, DESIGN.md "4n. FLAC").

What ``msg_quantize`` leaves in HBM, packed 16- or 24-bit PCM of one or two channels, becomes the
FLAC frames of each signal where it lies: fixed predictors of order 0 .. 4, partitioned Rice codes,
constant and verbatim subframes and the four stereo assignments, all of it integer arithmetic
(csrc/flac.h), so the device's bytes are those of ``msg_flac_host``'s sequential bit writer, alone
or in any batch.  The encoded lengths are only known on the device: reading the records is one
host wait, after which exactly the encoded bytes cross to the host.  The 42-byte stream header
(``fLaC`` and STREAMINFO) is written here from a signal's record.

:func:`read_flac` is the reader of the files this module writes and of any FLAC file inside the
same subset: fixed block size, constant, verbatim and fixed subframes without wasted bits, both
Rice methods without escape partitions, one or two channels at 16 or 24 bits.  It verifies every
CRC-8, every CRC-16 and the MD5 and raises ``ValueError`` on anything else.  It is written from
the format and shares nothing with the encoder.
"""
from __future__ import annotations

import ctypes as C
import hashlib
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from ._signal import read_records
from .pcm import check_bits, pack

BLOCKS = (256, 512, 1024, 2048, 4096)
RATE_MAX = 655350

# msg_flac_rec as a numpy record
FLAC_DTYPE = np.dtype([("byte_off", "<i8"), ("bytes", "<i8"), ("frames", "<i8"), ("samples", "<i8"), ("min_frame", "<i4"),
                       ("max_frame", "<i4"), ("md5", "u1", (16,)), ("constant", "<i4"), ("verbatim", "<i4"),
                       ("fixed", "<i4"), ("flags", "<i4"), ("assign", "<i4", (4,))])
REC_WORDS = FLAC_DTYPE.itemsize // 8


@dataclass
class Flac:
    block: object = 4096           # frames per block: 256, 512, 1024, 2048 or 4096
    md5: object = True             # the MD5 of the PCM in STREAMINFO (a launch of its own on the device)

    def check(self, rate=None):
        """ValueError for a value out of range.  Returns self."""
        if isinstance(self.block, bool) or self.block not in BLOCKS:
            raise ValueError("block must be 256, 512, 1024, 2048 or 4096")
        if not isinstance(self.md5, (bool, np.bool_)):
            raise ValueError("md5 must be True or False")
        if rate is not None:
            check_rate(rate)
        return self


def check_rate(rate):
    if isinstance(rate, bool) or int(rate) != rate or not 1 <= int(rate) <= RATE_MAX:
        raise ValueError(f"the sample rate must be a whole number of Hz from 1 to {RATE_MAX}")
    return int(rate)


def bound(frames, channels, bits, block=4096):
    """msg_flac_bound: the most bytes the FLAC frames of ``frames`` frames can take."""
    b = int(L.lib().msg_flac_bound(int(frames), int(channels), int(bits), int(block)))
    if b < 0:
        raise ValueError("frames, channels, bits or block out of range")
    return b


def _integers(q, bits):
    a = np.asarray(q)
    if a.dtype.kind != "i" or a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
        raise ValueError("q must be integer audio, (n,), (n, 1) or (n, 2)")
    S = 1 << (check_bits(bits) - 1)
    if a.size and (int(a.min()) < -S or int(a.max()) > S - 1):
        raise ValueError(f"q exceeds {bits} bits")
    return a, (1 if a.ndim == 1 else int(a.shape[1]))


def stream_header(rec, sr, channels, bits, block):
    """``fLaC``, the header of the one metadata block and STREAMINFO, 42 bytes (uint8), from a
    signal's record (a FLAC_DTYPE scalar, or anything with its fields)."""
    sr, bits, channels, block = check_rate(sr), check_bits(bits), int(channels), int(block)
    samples = int(rec["samples"])
    if channels not in (1, 2) or block not in BLOCKS or not 0 <= samples < 1 << 36:
        raise ValueError("channels, block or samples out of range")
    v = (sr << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | samples
    head = b"fLaC" + bytes([0x80, 0, 0, 34]) + block.to_bytes(2, "big") * 2 + int(rec["min_frame"]).to_bytes(3, "big") + \
        int(rec["max_frame"]).to_bytes(3, "big") + v.to_bytes(8, "big") + bytes(np.asarray(rec["md5"], dtype=np.uint8))
    return np.frombuffer(head, dtype=np.uint8).copy()


def frames_host(q, sr, bits, flac=None):
    """msg_flac_host over integer audio ``q``: (the frames' bytes, the record), no device."""
    flac = (flac or Flac()).check(sr)
    a, channels = _integers(q, bits)
    pcm = np.ascontiguousarray(pack(a, bits))
    out = np.zeros(max(bound(a.shape[0], channels, bits, flac.block), 1), dtype=np.uint8)
    rec = np.zeros(1, dtype=FLAC_DTYPE)
    L.check(L.lib().msg_flac_host(pcm.ctypes.data_as(C.c_void_p), channels, int(a.shape[0]), bits, int(sr), int(flac.block),
                                  int(bool(flac.md5)), out.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p)), None)
    return out[:int(rec[0]["bytes"])].copy(), rec[0]


def encode_host(q, sr, bits, flac=None):
    """The complete .flac file of integer audio ``q`` (uint8, 1-D) by the library's host loop."""
    flac = flac or Flac()
    body, rec = frames_host(q, sr, bits, flac)
    return np.concatenate([stream_header(rec, sr, _integers(q, bits)[1], bits, flac.block), body])


def records(rec):
    """Device records (Engine.flac) as a FLAC_DTYPE array on the host; waits for them."""
    return read_records(rec, FLAC_DTYPE)


def files(host, rec, sr, channels, bits, block):
    """The complete files of a batch: ``host`` holds the frames' bytes (at least up to the last
    record's end), ``rec`` the FLAC_DTYPE records."""
    return [np.concatenate([stream_header(r, sr, channels, bits, block), host[int(r["byte_off"]):int(r["byte_off"] + r["bytes"])]])
            for r in rec]


def total_bytes(rec):
    """The bytes of the output the records' frames take."""
    return int((rec["byte_off"] + rec["bytes"]).max()) if len(rec) else 0


def encode(q, sr, bits, flac=None, channels=None, device: int = 0):
    """The complete .flac file (uint8, 1-D) of ``q`` encoded on the device: integer audio, (n,) or
    (n, channels) NumPy, or the packed device bytes of one signal as msg_quantize wrote them (uint8
    tensor; give ``channels``)."""
    from .engine import default_engine

    flac = (flac or Flac()).check(sr)
    bits = check_bits(bits)
    eng = default_engine(device)
    if isinstance(q, eng.torch.Tensor):
        if channels not in (1, 2):
            raise ValueError("channels must be 1 or 2 for packed device bytes")
        t, channels = q, int(channels)
        if t.dtype != eng.torch.uint8 or t.dim() != 1 or t.numel() % (channels * (bits // 8)):
            raise ValueError("q must be a 1-D uint8 tensor of whole frames")
        n = t.numel() // (channels * (bits // 8))
    else:
        a, channels = _integers(q, bits)
        n = int(a.shape[0])
        t = eng.torch.from_numpy(np.ascontiguousarray(pack(a, bits)).copy()).to(f"cuda:{eng.device}")
    out, rec = eng.flac(t, [0], [n], channels, bits, sr, flac.block, flac.md5)
    r = records(rec)
    return files(out[:total_bytes(r)].cpu().numpy(), r, sr, channels, bits, flac.block)[0]


def write_flac(path, q, sr=None, bits=None, flac=None, host=False, device: int = 0):
    """Write ``q`` as a .flac file: a complete file already (uint8, 1-D, as :func:`encode` returns)
    or integer audio with ``sr`` and ``bits``, encoded on the device (``host``: by the host loop)."""
    a = np.asarray(q) if not hasattr(q, "device") else q
    if isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 1 and sr is None:
        data = a
    else:
        data = encode_host(a, sr, bits, flac) if host else encode(a, sr, bits, flac, device=device)
    if bytes(data[:4]) != b"fLaC":
        raise ValueError("not a FLAC stream")
    with open(path, "wb") as f:
        data.tofile(f)


# ---- the reader: written from the format, nothing shared with the encoder ----

def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    tab = []
    for b in range(256):
        r = b << (width - 8)
        for _ in range(8):
            r = ((r << 1) ^ poly) & mask if r & top else (r << 1) & mask
        tab.append(r)
    return tab


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data):
    r = 0
    for b in bytes(data):
        r = _T8[r ^ b]
    return r


def crc16(data):
    r = 0
    for b in bytes(data):
        r = ((r << 8) & 0xFFFF) ^ _T16[(r >> 8) ^ b]
    return r


_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}


class _Bits:
    """The bits of one frame, MSB first."""

    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8))
        self.pos = 0
        self._next = None

    def uint(self, n):
        if self.pos + n > self.bits.size:
            raise ValueError("truncated frame")
        v = 0
        for b in self.bits[self.pos:self.pos + n].tolist():
            v = (v << 1) | b
        self.pos += n
        return v

    def signed(self, count, depth):
        """``count`` two's-complement numbers of ``depth`` bits as int64."""
        end = self.pos + count * depth
        if end > self.bits.size:
            raise ValueError("truncated frame")
        w = (np.int64(1) << np.arange(depth - 1, -1, -1, dtype=np.int64))
        v = self.bits[self.pos:end].reshape(count, depth).astype(np.int64) @ w
        self.pos = end
        return v - ((v >> (depth - 1)) << depth)

    def rice(self, count, k):
        """``count`` Rice codes of parameter k, unfolded to signed int64."""
        if self._next is None:               # for every bit the index of the next one bit at or after it
            n = self.bits.size
            idx = np.where(self.bits != 0, np.arange(n, dtype=np.int64), n)
            self._next = np.minimum.accumulate(idx[::-1])[::-1].tolist() + [n, n]
        nxt, n, pos = self._next, self.bits.size, self.pos
        start = [0] * count
        stop = [0] * count
        for i in range(count):
            start[i] = pos
            s = nxt[pos] if pos < n else n
            stop[i] = s
            pos = s + 1 + k
        if count and pos > n:
            raise ValueError("truncated residual")
        self.pos = pos
        start, stop = np.asarray(start, dtype=np.int64), np.asarray(stop, dtype=np.int64)
        u = stop - start
        if k:
            w = (np.int64(1) << np.arange(k - 1, -1, -1, dtype=np.int64))
            low = self.bits[(stop + 1)[:, None] + np.arange(k)[None, :]].astype(np.int64) @ w
            u = (u << k) | low
        return np.where(u & 1, -((u + 1) >> 1), u >> 1)


def _subframe(br, n, depth, counts):
    if br.uint(1):
        raise ValueError("subframe padding bit set")
    kind = br.uint(6)
    if br.uint(1):
        raise ValueError("wasted bits are outside the subset")
    if kind == 0:
        counts["constant"] += 1
        return np.full(n, br.signed(1, depth)[0], dtype=np.int64)
    if kind == 1:
        counts["verbatim"] += 1
        return br.signed(n, depth)
    if not 8 <= kind <= 12:
        raise ValueError(f"subframe type {kind:06b} is outside the subset")
    counts["fixed"] += 1
    order = kind - 8
    if order > n:
        raise ValueError("predictor order above the block size")
    warm = br.signed(order, depth) if order else np.zeros(0, dtype=np.int64)
    method = br.uint(2)
    if method > 1:
        raise ValueError("reserved residual coding method")
    pbits, escape = (4, 15) if method == 0 else (5, 31)
    porder = br.uint(4)
    if n % (1 << porder) or (n >> porder) < order:
        raise ValueError("partition order does not fit the block")
    parts = []
    counts["params"] = counts.get("params", [])
    for q in range(1 << porder):
        k = br.uint(pbits)
        if k == escape:
            raise ValueError("escape partitions are outside the subset")
        counts["params"].append(k)
        parts.append(br.rice((n >> porder) - (order if q == 0 else 0), k))
    counts["method"] = method
    counts["order"], counts["porder"] = order, porder
    res = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    # undo the order-th difference: one running sum per order, each started from the warm-up's own differences
    diffs = [warm]
    for _ in range(order):
        diffs.append(np.diff(diffs[-1]))
    seq = res
    for j in range(order - 1, -1, -1):
        seq = diffs[j][-1] + np.cumsum(seq)
    return np.concatenate([warm, seq])


def read_frame(data, pos, channels=None, bits=None):
    """One frame of ``data`` (bytes) at byte ``pos``: (samples (n, channels) int64, the position
    after it, info), every check made.  ``channels`` and ``bits``: what STREAMINFO said, if known."""
    b = data
    if len(b) < pos + 6 or b[pos] != 0xFF or b[pos + 1] != 0xF8:
        raise ValueError("no fixed-block frame sync")
    bs_code, rate_code = b[pos + 2] >> 4, b[pos + 2] & 15
    assign, size_code = b[pos + 3] >> 4, (b[pos + 3] >> 1) & 7
    if b[pos + 3] & 1:
        raise ValueError("reserved header bit set")
    if assign not in (0, 1, 8, 9, 10):
        raise ValueError("channel assignment outside the subset")
    if size_code not in (4, 6):
        raise ValueError("sample size outside the subset")
    depth = 16 if size_code == 4 else 24
    ch = 1 if assign == 0 else 2
    if (channels is not None and ch != channels) or (bits is not None and depth != bits):
        raise ValueError("frame disagrees with STREAMINFO")
    at = pos + 4
    first = b[at]
    at += 1
    if first < 0x80:
        number = first
    else:
        cont = 0
        while first & (0x80 >> cont):
            cont += 1
        if cont < 2 or cont > 6:
            raise ValueError("bad frame number")
        number = first & (0x7F >> cont)
        for _ in range(cont - 1):
            if b[at] & 0xC0 != 0x80:
                raise ValueError("bad frame number")
            number = (number << 6) | (b[at] & 0x3F)
            at += 1
    if bs_code == 6:
        n = b[at] + 1
        at += 1
    elif bs_code == 7:
        n = ((b[at] << 8) | b[at + 1]) + 1
        at += 2
    elif 8 <= bs_code <= 12:
        n = 256 << (bs_code - 8)
    else:
        raise ValueError("block size outside the subset")
    if rate_code in _RATES:
        rate = _RATES[rate_code]
    elif rate_code == 12:
        rate = b[at] * 1000
        at += 1
    elif rate_code in (13, 14):
        rate = ((b[at] << 8) | b[at + 1]) * (1 if rate_code == 13 else 10)
        at += 2
    elif rate_code == 0:
        rate = None
    else:
        raise ValueError("reserved sample-rate code")
    if crc8(b[pos:at]) != b[at]:
        raise ValueError("frame header CRC-8 mismatch")
    at += 1
    most = at + ch * (2 + (n * (depth + 1) + 7) // 8) + 2
    br = _Bits(b[at:most])
    counts = {"constant": 0, "verbatim": 0, "fixed": 0}
    subs = []
    for s in range(ch):
        side = (assign == 8 and s == 1) or (assign == 9 and s == 0) or (assign == 10 and s == 1)
        c = {"constant": 0, "verbatim": 0, "fixed": 0}
        subs.append(_subframe(br, n, depth + (1 if side else 0), c))
        for k in ("constant", "verbatim", "fixed"):
            counts[k] += c[k]
        counts.setdefault("subframes", []).append(c)
    if br.pos % 8 and br.uint(8 - br.pos % 8):
        raise ValueError("nonzero padding")
    end = at + br.pos // 8
    if len(b) < end + 2 or crc16(b[pos:end]) != ((b[end] << 8) | b[end + 1]):
        raise ValueError("frame CRC-16 mismatch")
    if assign == 8:
        left, right = subs[0], subs[0] - subs[1]
    elif assign == 9:
        left, right = subs[0] + subs[1], subs[1]
    elif assign == 10:
        m = (subs[0] << 1) | (subs[1] & 1)
        left, right = (m + subs[1]) >> 1, (m - subs[1]) >> 1
    else:
        left, right = subs[0], subs[-1]
    x = left[:, None] if ch == 1 else np.stack([left, right], axis=1)
    info = {"number": number, "samples": n, "rate": rate, "assign": assign, "bits": depth, "bytes": end + 2 - pos,
            "block_code": bs_code, "rate_code": rate_code, **counts}
    return x, end + 2, info


def read_streaminfo(data):
    """The stream header of ``data`` (bytes): a dict of STREAMINFO's fields and where the frames begin."""
    b = data
    if len(b) < 42 or b[:4] != b"fLaC":
        raise ValueError("not a FLAC stream")
    if b[4] & 0x7F != 0 or int.from_bytes(b[5:8], "big") != 34:
        raise ValueError("the first metadata block must be STREAMINFO")
    pos = 8
    last = bool(b[4] & 0x80)
    si = b[8:42]
    pos = 42
    while not last:                              # other metadata blocks are skipped
        if len(b) < pos + 4:
            raise ValueError("truncated metadata")
        last = bool(b[pos] & 0x80)
        pos += 4 + int.from_bytes(b[pos + 1:pos + 4], "big")
    v = int.from_bytes(si[10:18], "big")
    return {"min_block": int.from_bytes(si[0:2], "big"), "max_block": int.from_bytes(si[2:4], "big"),
            "min_frame": int.from_bytes(si[4:7], "big"), "max_frame": int.from_bytes(si[7:10], "big"),
            "rate": v >> 44, "channels": ((v >> 41) & 7) + 1, "bits": ((v >> 36) & 31) + 1, "samples": v & ((1 << 36) - 1),
            "md5": bytes(si[18:34]), "first_frame": pos}


def read_flac(path_or_bytes):
    """A .flac file of the subset this module writes: (frames x channels integers, int16 or int32,
    sr, bits, info).  Every CRC-8 and CRC-16 is verified, and the MD5 when STREAMINFO holds one.
    ``info``: STREAMINFO's fields and, as walked, ``frames``, ``frame_bytes`` (a list), ``smallest`` and
    ``largest`` frame, the subframe counts and ``assign`` (frames per channel assignment code)."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview, np.ndarray)):
        b = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            b = f.read()
    si = read_streaminfo(b)
    if si["min_block"] != si["max_block"] or si["channels"] not in (1, 2) or si["bits"] not in (16, 24):
        raise ValueError("stream outside the subset: one block size, 1 or 2 channels, 16 or 24 bits")
    pos, got, number = si["first_frame"], 0, 0
    parts, sizes = [], []
    info = dict(si, constant=0, verbatim=0, fixed=0, assign={}, frame_info=[])
    while pos < len(b):
        x, nxt, fi = read_frame(b, pos, si["channels"], si["bits"])
        if fi["number"] != number:
            raise ValueError("frame numbers out of order")
        if fi["rate"] is not None and fi["rate"] != si["rate"]:
            raise ValueError("frame rate disagrees with STREAMINFO")
        if fi["samples"] > si["max_block"] or (fi["samples"] != si["max_block"] and got + fi["samples"] != si["samples"]):
            raise ValueError("only the last block may be short")
        parts.append(x)
        sizes.append(nxt - pos)
        for k in ("constant", "verbatim", "fixed"):
            info[k] += fi[k]
        info["assign"][fi["assign"]] = info["assign"].get(fi["assign"], 0) + 1
        info["frame_info"].append(fi)
        got += fi["samples"]
        number += 1
        pos = nxt
    if got != si["samples"]:
        raise ValueError("STREAMINFO's sample count does not match the frames")
    info.update(frames=number, frame_bytes=sizes, smallest=min(sizes, default=0), largest=max(sizes, default=0))
    dtype = np.int16 if si["bits"] == 16 else np.int32
    q = (np.concatenate(parts) if parts else np.zeros((0, si["channels"]), dtype=np.int64)).astype(dtype)
    if si["md5"] != bytes(16) and hashlib.md5(pack(q, si["bits"]).tobytes()).digest() != si["md5"]:
        raise ValueError("MD5 mismatch")
    return q, si["rate"], si["bits"], info
