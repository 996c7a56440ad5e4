#!/usr/bin/env python3
"""Stereo timing on S x 48 000 stereo frames at 48 kHz: the meter beside msg_loudness on the same
buffer (the meter reads once and filters nothing), the in-place image beside the msg_truepeak_gain
sweep (the same traffic: every sample read once and written once), the fold to mono, and the
delivery chain (-23 LUFS, -1 dBTP, 16 bits) with Stereo(channels=1) against the same chain without it.

    python tools/stereo_time.py [--batch 1024] [--steps 10] [--out profiles/stereo_time.json]

Every signal is noise at 0.1 whose right channel is half the left plus noise, and is restored
before each timed call, outside the timed window.  The passes alternate call by call, each between
device events on the stream; the chains alternate too, each timed by the host clock from the call
to the end of a device synchronise.

Writes one JSON document: mean, spread (max - min) and every call in milliseconds, the bytes each
pass moves and the rate that makes, and the box.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stereo_time.json"))
    a = ap.parse_args()
    import torch
    from msgpu.engine import default_engine
    from msgpu.export import Delivery, deliver
    from msgpu.stereo import Stereo

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    S, n, sr = a.batch, 48000, 48000
    wide, mono = Stereo(width=1.5, balance_db=1.0), Stereo(channels=1)

    def stat(ms):
        return {"mean_ms": round(float(np.mean(ms)), 4), "spread_ms": round(float(max(ms) - min(ms)), 4),
                "calls_ms": [round(float(v), 4) for v in ms]}

    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x0 = torch.randn((S * n, 2), generator=g, device=dev, dtype=torch.float32) * 0.1
    x0[:, 1] = 0.5 * x0[:, 0] + 0.5 * x0[:, 1]
    x0 = x0.contiguous()
    x = x0.clone()
    y = torch.empty((S * n, 1), dtype=torch.float32, device=dev)
    offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)
    tp = eng.true_peak(x, offs, lens, 2, sr)                 # the gain sweep's record, measured once

    # ---- the passes, alternating, device events around each call ----------------------------------
    nbytes = S * n * 2 * 4
    passes = {"stereo_meter": (lambda: eng.stereo_meter(x, offs, lens, sr), nbytes),
              "loudness": (lambda: eng.loudness(x, offs, lens, 2, sr), 2 * nbytes),
              "image_in_place": (lambda: eng.stereo(x, offs, lens, wide), 2 * nbytes),
              "truepeak_gain_sweep": (lambda: eng.true_peak_gain(x, offs, lens, 2, tp, None, None, 0.5, None), 2 * nbytes),
              "fold_to_mono": (lambda: eng.stereo(x, offs, lens, mono, out=y), nbytes + nbytes // 2)}
    ms = {k: [] for k in passes}
    evs = []
    for step in range(a.warmup + a.steps):
        for k, (fn, _) in passes.items():
            x.copy_(x0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            if step >= a.warmup:
                evs.append((k, e0, e1))
    torch.cuda.synchronize()
    for k, e0, e1 in evs:
        ms[k].append(e0.elapsed_time(e1))
    rows = {k: stat(v) for k, v in ms.items()}
    for k, r in rows.items():
        r["bytes"] = passes[k][1]
        r["gb_per_s"] = round(r["bytes"] / (r["mean_ms"] * 1e-3) / 1e9, 1)
    doc = {"bench": "stereo_time", "steps": a.steps, "warmup": a.warmup, "signals": S, "frames": n, "sr": sr,
           "bytes_note": "meter: one read; loudness: two reads; image and gain sweep: one read, one write; "
                         "fold: one read, half a write",
           "passes": rows,
           "meter_over_loudness": round(rows["stereo_meter"]["mean_ms"] / rows["loudness"]["mean_ms"], 4),
           "image_over_gain_sweep": round(rows["image_in_place"]["mean_ms"] / rows["truepeak_gain_sweep"]["mean_ms"], 4)}

    # ---- the chain, alternating, host clock to the end of a synchronise ----------------------------
    chains = {"stereo_delivery": None, "mono_delivery": mono}
    wall = {k: [] for k in chains}
    out_bytes = {}
    for step in range(a.warmup + a.steps):
        for k, st in chains.items():
            x.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q, _, nb, _ = deliver(eng, x, offs, lens, [sr] * S, Delivery(lufs=-23.0, true_peak=-1.0, bits=16, stereo=st), None,
                                  range(S))
            torch.cuda.synchronize()
            if step >= a.warmup:
                wall[k].append((time.perf_counter() - t0) * 1e3)
            out_bytes[k] = int(np.sum(nb))
            del q
    doc["deliver_lufs_tp_16bit"] = {k: dict(stat(v), pcm_bytes=out_bytes[k]) for k, v in wall.items()}
    doc["box"] = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": getattr(torch.version, "hip", None)}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
