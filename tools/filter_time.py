#!/usr/bin/env python3
"""Filter timing: msg_filter with 2 and 8 sections on S x 48 000 stereo frames at 48 kHz and on
S x 384 000 at 384 kHz, beside the yardstick msg_loudness + msg_loudness_gain on the same buffer
(the same three sweeps plus one read, with two sections); then the delivery chain (-23 LUFS,
-1 dBTP, 16 bits) at 48 kHz with and without the filter.

    python tools/filter_time.py [--batch 1024] [--steps 10] [--out profiles/filter_time.json]

Every signal is noise at 0.1 on a DC offset of 0.05 and is restored before each timed call,
outside the timed window.  The passes alternate call by call, each between device events on the
stream; the chains alternate too, each timed by the host clock from the call to the end of a
device synchronise.

Writes one JSON document: mean, spread (max - min) and every call in milliseconds, the bytes each
pass moves (every sample read twice and written once for the filter; read three times and written
once for the yardstick) and the rate that makes, and the box.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "filter_time.json"))
    a = ap.parse_args()
    import torch
    from msgpu.engine import default_engine
    from msgpu.export import Delivery, deliver
    from msgpu.filter import Filter

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    S = a.batch
    two = Filter(highpass=(20, 4))
    eight = Filter(highpass=(20, 4), low_shelf=(120, 3.0, 0.7), peaks=[(400, -4.0, 1.4), (3000, 2.5, 2.0)],
                   high_shelf=(9000, -2.0, 0.7), lowpass=(18000, 4))
    assert two.n_sections() == 2 and eight.n_sections() == 8

    def stat(ms):
        return {"mean_ms": round(float(np.mean(ms)), 4), "spread_ms": round(float(max(ms) - min(ms)), 4),
                "calls_ms": [round(float(v), 4) for v in ms]}

    doc = {"bench": "filter_time", "steps": a.steps, "warmup": a.warmup, "signals": S, "sizes": {}}
    for n, sr in ((48000, 48000), (384000, 384000)):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        x0 = (torch.randn((S * n, 2), generator=g, device=dev, dtype=torch.float32) * 0.1 + 0.05).contiguous()
        x = x0.clone()
        offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)

        def yardstick():
            r = eng.loudness(x, offs, lens, 2, sr)
            eng.loudness_gain(x, offs, lens, 2, r, -23.0, None)

        # ---- the passes, alternating, device events around each call ------------------------------
        passes = {"filter_2_sections": lambda: eng.filter(x, offs, lens, 2, sr, two),
                  "filter_8_sections": lambda: eng.filter(x, offs, lens, 2, sr, eight),
                  "loudness_plus_gain": yardstick}
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
        rows = {k: stat(v) for k, v in ms.items()}
        for k, r in rows.items():
            r["bytes"] = (4 if k == "loudness_plus_gain" else 3) * nbytes
            r["gb_per_s"] = round(r["bytes"] / (r["mean_ms"] * 1e-3) / 1e9, 1)
        size = {"frames": n, "sr": sr, "passes": rows,
                "filter_2_over_yardstick": round(rows["filter_2_sections"]["mean_ms"] / rows["loudness_plus_gain"]["mean_ms"], 4)}

        # ---- the chain, alternating, host clock to the end of a synchronise ----------------------
        if sr == 48000:
            chains = {"no_filter": None, "highpass_2_sections": two, "eight_sections": eight}
            wall = {k: [] for k in chains}
            for step in range(a.warmup + a.steps):
                for k, f in chains.items():
                    x.copy_(x0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    deliver(eng, x, offs, lens, [sr] * S, Delivery(lufs=-23.0, true_peak=-1.0, bits=16, filter=f), None, range(S))
                    torch.cuda.synchronize()
                    if step >= a.warmup:
                        wall[k].append((time.perf_counter() - t0) * 1e3)
            size["deliver_lufs_tp_16bit"] = {k: stat(v) for k, v in wall.items()}
        doc["sizes"][f"{S}x{n}"] = size
        del x, x0
        torch.cuda.empty_cache()
    doc["box"] = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": getattr(torch.version, "hip", None)}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
