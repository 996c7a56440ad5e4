#!/usr/bin/env python3
"""Edges timing: msg_edges (find + span + apply) with a trim and 2 / 20 ms fades on S x 48 000
stereo frames at 48 kHz, beside msg_truepeak_gain on the same buffer, which also reads every
sample once and writes it; then the delivery chain (-23 LUFS, -1 dBTP, 16 bits) without
edges, with fades alone (no host wait) and with trim and fades (the spans are read: one wait).

    python tools/edges_time.py [--batch 1024] [--steps 10] [--out profiles/edges_time.json]

Every signal is noise at 0.1 between 100 ms and 800 ms and digital silence around it, and is
restored before each timed call, outside the timed window.  The two passes alternate call by
call, each between device events on the stream; the chains alternate too, each timed by the
host clock from the call to the end of a device synchronise, since one of them waits.

Writes one JSON document: mean, spread (max - min) and every call in milliseconds, the bytes
each pass moves and the rate that makes, and the box.
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
    ap.add_argument("--frames", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "edges_time.json"))
    a = ap.parse_args()
    import torch
    from msgpu.edges import Edges, records
    from msgpu.engine import default_engine
    from msgpu.export import Delivery, deliver

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    S, n, sr = a.batch, a.frames, 48000
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x0 = torch.randn((S, n, 2), generator=g, device=dev, dtype=torch.float32) * 0.1
    x0[:, :n // 10] = 0.0
    x0[:, n * 8 // 10:] = 0.0
    x0 = x0.reshape(S * n, 2).contiguous()
    x = x0.clone()
    offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)
    trim = Edges(trim_db=-60, pad_ms=5, fade_ms=(2, 20))
    fades = Edges(fade_ms=(2, 20))
    tp = eng.true_peak(x, offs, lens, 2, sr)
    first = records(eng.edges(x, offs, lens, 2, sr, trim))[0]

    def stat(ms):
        return {"mean_ms": round(float(np.mean(ms)), 4), "spread_ms": round(float(max(ms) - min(ms)), 4),
                "calls_ms": [round(float(v), 4) for v in ms]}

    # ---- the passes, alternating, device events around each call --------------------------------
    passes = {"edges_trim_fades": lambda: eng.edges(x, offs, lens, 2, sr, trim),
              "edges_fades_only": lambda: eng.edges(x, offs, lens, 2, sr, fades),
              "truepeak_gain": lambda: eng.true_peak_gain(x, offs, lens, 2, tp, None, None, 0.5, None)}
    ms = {k: [] for k in passes}
    evs = []
    for step in range(a.warmup + a.steps):
        for k, fn in passes.items():
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
    nbytes = S * n * 2 * 4
    fade_bytes = 2 * S * (96 + 960) * 2 * 4
    rows = {k: stat(v) for k, v in ms.items()}
    rows["edges_trim_fades"]["bytes"] = nbytes + fade_bytes                 # one read of every sample, the fades read and written
    rows["edges_fades_only"]["bytes"] = fade_bytes
    rows["truepeak_gain"]["bytes"] = 2 * nbytes                             # every sample read and written
    for r in rows.values():
        r["gb_per_s"] = round(r["bytes"] / (r["mean_ms"] * 1e-3) / 1e9, 1)

    # ---- the chain, alternating, host clock to the end of a synchronise ------------------------
    chains = {"no_edges": None, "fades_only": fades, "trim_fades": trim}
    wall = {k: [] for k in chains}
    delivered = {}
    for step in range(a.warmup + a.steps):
        for k, e in chains.items():
            x.copy_(x0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y, off, nb, _ = deliver(eng, x, offs, lens, [sr] * S, Delivery(lufs=-23.0, true_peak=-1.0, bits=16, edges=e),
                                    None, range(S))
            torch.cuda.synchronize()
            if step >= a.warmup:
                wall[k].append((time.perf_counter() - t0) * 1e3)
            delivered[k] = int(np.asarray(nb).sum())
    chain_rows = {k: dict(stat(v), delivered_bytes=delivered[k]) for k, v in wall.items()}
    doc = {"bench": "edges_time", "steps": a.steps, "warmup": a.warmup, "signals": S, "frames": n, "sr": sr,
           "first_record": {k: int(first[k]) for k in first.dtype.names},
           "passes": rows, "deliver_lufs_tp_16bit": chain_rows,
           "wait_cost_ms": round(chain_rows["trim_fades"]["mean_ms"] - chain_rows["fades_only"]["mean_ms"], 4),
           "box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "hip": getattr(torch.version, "hip", None)}}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
