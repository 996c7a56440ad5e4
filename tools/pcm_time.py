#!/usr/bin/env python3
"""PCM quantiser timing: msg_quantize at 16 and 24 bits, with and without TPDF dither, on
S stereo signals of 48 000, 96 000 and 384 000 frames, timed with device events on the
call's stream after a warm-up.  The yardstick is msg_truepeak_gain's scale sweep alone
(it reads and writes 8 B per frame; the quantiser reads 8 and writes 4 or 6) on the same
buffer in the same session, timed before and after; msg_digest (one read of the same
bytes) is a second column.  Also the device-to-host copy of one S x 48 000 batch as
float32, 24-bit and 16-bit bytes (host clock around a synchronised copy).

    python tools/pcm_time.py [--batch 1024] [--steps 10] [--out profiles/pcm_time.json]

Writes one JSON document: per shape and variant the milliseconds per call, the ratio to
the yardstick, the bytes per second counting 8 B read and bits / 4 B written per frame,
and the box.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-suite_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", default="48000,96000,384000", help="frames per signal, comma-separated")
    ap.add_argument("--shift", type=int, default=0,
                    help="start every signal that many frames into the buffer (1: every span lies 8 bytes off a "
                         "16-byte address and takes the kernel's piecewise path)")
    ap.add_argument("--note", default="", help="a label for the document (e.g. the store shape built)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pcm_time.json"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    from msgpu import _lib as L
    from msgpu.engine import default_engine
    from msgpu.pcm import records

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    S = a.batch

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    rows = []
    for n in (int(v) for v in a.frames.split(",")):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        x = torch.randn((S * n + a.shift, 2), generator=g, device=dev, dtype=torch.float32) * 0.1
        offs, lens = np.arange(S, dtype=np.int64) * n + a.shift, np.full(S, n, dtype=np.int64)
        tp = eng.true_peak(x, offs, lens, 2, 384000)                  # the plain max sweep: the records the gain reads
        out = torch.empty(S * n * 6, dtype=torch.uint8, device=dev)   # n * 4 and n * 6 are multiples of 16 here
        drec = torch.empty((S, 6), dtype=torch.float64, device=dev)
        po, pn = offs.ctypes.data_as(C.POINTER(C.c_int64)), lens.ctypes.data_as(C.POINTER(C.c_int64))

        def gain():                        # never binds: g = 1, x keeps its bits
            eng.true_peak_gain(x, offs, lens, 2, tp, ceiling_tp=1e6)

        def digest():                      # msg_digest alone: Engine.digest also copies the records back
            L.check(L.lib().msg_digest(eng._ctx, C.c_void_p(x.data_ptr()), po, pn, S, C.c_void_p(drec.data_ptr()),
                                       C.c_void_p(stream.cuda_stream)), eng._ctx)

        # one session; the yardsticks are timed before and after the quantiser
        g0, d0 = timed(gain), timed(digest)
        ms = {}
        for bits in (16, 24):
            for mode in ("tpdf", "none"):
                ms[(bits, mode)] = timed(lambda: eng.quantize(x, offs, lens, 2, bits, mode, 0, None, out=out))
        g1, d1 = timed(gain), timed(digest)
        gm, dm = 0.5 * (g0 + g1), 0.5 * (d0 + d1)
        first = records(eng.quantize(x, offs, lens, 2, 16, "tpdf", 0, None, out=out)[2])[0]
        row = {"signals": S, "frames": n, "shift": a.shift, "gain_ms": round(gm, 4), "gain_ms_before_after": [round(g0, 4), round(g1, 4)],
               "gain_GBs": round(16.0 * S * n / (gm * 1e-3) / 1e9, 1),
               "digest_ms": round(dm, 4), "digest_ms_before_after": [round(d0, 4), round(d1, 4)],
               "clipped_first": int(first["clipped"]), "q_max_first": int(first["q_max"])}
        for (bits, mode), t in ms.items():
            moved = (8.0 + bits / 4.0) * S * n
            row[f"pcm{bits}_{mode}_ms"] = round(t, 4)
            row[f"pcm{bits}_{mode}_ratio_to_gain"] = round(t / gm, 3)
            row[f"pcm{bits}_{mode}_ratio_to_digest"] = round(t / dm, 3)
            row[f"pcm{bits}_{mode}_GBs"] = round(moved / (t * 1e-3) / 1e9, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, out

    # what crosses to the host: one S x 48 000 batch as float32, then as the quantiser's bytes
    n = 48000
    x = torch.randn((S * n, 2), device=dev, dtype=torch.float32) * 0.1
    offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)
    copies = {}

    def copy_ms(t):
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.cpu()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        return round(best, 2)

    copies["float32_ms"] = copy_ms(x)
    for bits in (24, 16):
        copies[f"pcm{bits}_ms"] = copy_ms(eng.quantize(x, offs, lens, 2, bits)[0])
    copies["bytes"] = {"float32": 8 * S * n, "pcm24": 6 * S * n, "pcm16": 4 * S * n}
    print(json.dumps(copies), flush=True)

    doc = {"bench": "pcm_time", "steps": a.steps, "warmup": a.warmup, "note": a.note,
           "box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "hip": getattr(torch.version, "hip", None)},
           "rows": rows, "d2h_copy_1024x48000": copies}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
