#!/usr/bin/env python3
"""True-peak timing: msg_truepeak, then msg_truepeak + msg_truepeak_gain, on S stereo
signals of 48 000 frames at 48 kHz (oversampled by 4), 96 000 at 96 kHz (by 2) and
384 000 at 384 kHz (the plain max sweep), timed with device events on the call's stream
after a warm-up.  The yardstick is msg_digest on the same buffer in the same session,
timed before and after: the one-read reduction over the same bytes.

    python tools/truepeak_time.py [--batch 1024] [--steps 10] [--out profiles/truepeak_time.json]

Writes one JSON document: per shape the milliseconds per call, the ratio to msg_digest,
the fused multiply-adds per second of the interpolator (frames x channels x 24 taps x
(OS - 1) phases) and the bytes per second counting 8 B per frame per HBM sweep
(msg_truepeak reads a signal once; the gain pass reads and writes it once more), and
the box.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-suite_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

SWEEPS_MEASURE, SWEEPS_GAIN = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="48000:48000,96000:96000,384000:384000",
                    help="sr:frames per signal, comma-separated")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "truepeak_time.json"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    from msgpu import _lib as L
    from msgpu.engine import default_engine
    from msgpu.truepeak import TAPS, oversampling, records

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
    for shape in a.shapes.split(","):
        sr, n = (int(v) for v in shape.split(":"))
        os_ = oversampling(sr)
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        x = torch.randn((S * n, 2), generator=g, device=dev, dtype=torch.float32) * 0.1
        offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)
        first = records(eng.true_peak(x, offs, lens, 2, sr))[0]

        def measure_and_gain():
            r = eng.true_peak(x, offs, lens, 2, sr)
            eng.true_peak_gain(x, offs, lens, 2, r, ceiling_tp=1e6)      # never binds: g = 1, x keeps its bits

        drec = torch.empty((S, 6), dtype=torch.float64, device=dev)
        po, pn = offs.ctypes.data_as(C.POINTER(C.c_int64)), lens.ctypes.data_as(C.POINTER(C.c_int64))

        def digest():                      # msg_digest alone: Engine.digest also copies the records back
            L.check(L.lib().msg_digest(eng._ctx, C.c_void_p(x.data_ptr()), po, pn, S, C.c_void_p(drec.data_ptr()),
                                       C.c_void_p(stream.cuda_stream)), eng._ctx)

        # one session; the digest is timed before and after the true-peak calls
        dg0 = timed(digest)
        ms = timed(lambda: eng.true_peak(x, offs, lens, 2, sr))
        ms_gain = timed(measure_and_gain)
        dg1 = timed(digest)
        dg = 0.5 * (dg0 + dg1)
        sweep = 8.0 * S * n
        fma = 2.0 * S * n * TAPS * (os_ - 1)
        rows.append({"sr": sr, "os": os_, "signals": S, "frames": n, "sweep_bytes": sweep, "fma": fma,
                     "digest_ms": round(dg, 4), "digest_ms_before_after": [round(dg0, 4), round(dg1, 4)],
                     "truepeak_ms": round(ms, 4), "truepeak_gain_ms": round(ms_gain, 4),
                     "ratio_to_digest": round(ms / dg, 3), "ratio_with_gain_to_digest": round(ms_gain / dg, 3),
                     "hbm_sweeps": SWEEPS_MEASURE, "hbm_sweeps_with_gain": SWEEPS_MEASURE + SWEEPS_GAIN,
                     "digest_GBs": round(sweep / (dg * 1e-3) / 1e9, 1),
                     "truepeak_GBs": round(SWEEPS_MEASURE * sweep / (ms * 1e-3) / 1e9, 1),
                     "truepeak_TFMAs": round(fma / (ms * 1e-3) / 1e12, 2),
                     "truepeak_gain_GBs": round((SWEEPS_MEASURE + SWEEPS_GAIN) * sweep / (ms_gain * 1e-3) / 1e9, 1),
                     "true_peak_first": float(first["true_peak"]), "peak_first": float(first["peak"])})
        print(json.dumps(rows[-1]), flush=True)
        del x
    doc = {"bench": "truepeak_time", "steps": a.steps, "warmup": a.warmup,
           "box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "hip": getattr(torch.version, "hip", None)},
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
