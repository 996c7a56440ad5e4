#!/usr/bin/env python3
"""Resampler benchmark: S x n stereo frames at 384 kHz (one C3-shaped batch) to 48 kHz
(integer decimation kernel) and to 44.1 kHz (general kernel, 147/1280) through
msg_resample, timed with HIP events on the call's stream after warm-up.

    python tools/resample_bench.py [--batch 1024] [--n 384000] [--steps 10] [--export 64]

Prints one JSON line per target rate: device ms per call, the algorithmic bytes
S * 8 * (n + n_out) against 8 TB/s, the FMA rate, and the device-to-host copy time of
the full-rate and of the resampled buffer (torch's .cpu(), as batch.py copies).
With --export V, also the end-to-end export comparison on V variants of the C3
preset: render_variations as it was (full-rate copy) against export_sr=48000.
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
    ap.add_argument("--n", type=int, default=384000)
    ap.add_argument("--sr", type=int, default=384000)
    ap.add_argument("--rates", default="48000,44100")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--export", type=int, default=0, help="variants of the C3 preset for the export comparison")
    a = ap.parse_args()
    import torch
    import msgpu
    from msgpu.engine import default_engine
    from msgpu.resample import design, ratio, resample_len

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    S, n = a.batch, a.n
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x = torch.randn((S * n, 2), generator=g, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev)
    offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)

    def d2h_ms(t):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.cpu()
        return (time.perf_counter() - t0) * 1e3

    full_copy = None
    for sr_out in (int(r) for r in a.rates.split(",")):
        up, down = ratio(a.sr, sr_out)
        h = design(up, down)
        n_out = resample_len(n, up, down)
        y = torch.empty((S * n_out, 2), device=dev, dtype=torch.float32)
        for _ in range(a.warmup):
            eng.resample(x, offs, lens, 2, up, down, h, out=y)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        for _ in range(a.steps):
            eng.resample(x, offs, lens, 2, up, down, h, out=y)
        e1.record(stream)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.steps
        dev_ms = e0.elapsed_time(e1) / a.steps
        alg = S * 8.0 * (n + n_out)
        fma = 2.0 * S * n_out * (-(-h.size // up))          # taps per output x 2 channels
        if full_copy is None:
            d2h_ms(y)                                       # warm the copy path
            full_copy = d2h_ms(x)
        print(json.dumps({"bench": "resample", "sr_in": a.sr, "sr_out": sr_out, "up": up, "down": down,
                          "taps": int(h.size), "signals": S, "n": n, "n_out": n_out,
                          "device_ms_per_call": round(dev_ms, 4), "ms_per_call": round(wall * 1e3, 4),
                          "algorithmic_bytes": alg, "achieved_GBs": round(alg / (dev_ms * 1e-3) / 1e9, 1),
                          "peak_GBs": 8000.0, "frac": round(alg / (dev_ms * 1e-3) / 8e12, 4),
                          "fma": fma, "tfma_per_s": round(fma / (dev_ms * 1e-3) / 1e12, 2),
                          "d2h_full_rate_ms": round(full_copy, 1), "d2h_resampled_ms": round(d2h_ms(y), 1)}),
              flush=True)
        del y
    del x
    if a.export > 0:
        irs = dict(np.load(os.path.join(REPO, "tests", "golden", "irs.npz")))
        base = msgpu.config_params("C3", seed=1000, irs=irs)
        seeds = list(range(1000, 1000 + a.export))
        times = {"plain": [], "export_48000": []}
        for rep in range(3):                                # alternating; the first pair warms up
            for key, kw in (("plain", {}), ("export_48000", {"export_sr": 48000})):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                msgpu.render_variations(base, seeds, [base["time_unfold"]], [base["partial_stretch"]], **kw)
                if rep:
                    times[key].append(round((time.perf_counter() - t0) * 1e3, 1))
        print(json.dumps({"bench": "export", "config": "C3", "variants": a.export, "ms": times}), flush=True)


if __name__ == "__main__":
    main()
