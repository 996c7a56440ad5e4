#!/usr/bin/env python3
"""Gate timing: msg_gate_apply on S x 48 000 stereo frames at 48 kHz beside, in the same session and
on the same buffer, msg_dynamics without a hold (the same two sweeps and a scan over tiles) and the
true-peak gain sweep (msg_truepeak_gain from records measured once: one read and one write of every
sample).

    python tools/gate_time.py [--batch 1024] [--steps 10] [--out profiles/gate_time.json]

The inputs are tools/dynamics_time.py's, and the threshold is its -6 dB: ``quiet`` is noise at 0.1,
the gate opens for some tens of frames in 49 million and every other frame is written 60 dB down; ``dense`` is noise at 0.5 clipped to full
scale, the state changes all the time; ``grains`` is noise at 0.1 with seeded Hann grains over full
scale on about 2 % of the frames, the gate opens for each.  The gate is timed in three
configurations: ``gate_local`` without hysteresis and without a hold (three launches, the state is a
frame's own), ``gate_hysteresis`` with 6 dB of hysteresis (the state sweep and its scan in front:
five launches and a third read of the samples) and ``gate_hysteresis_hold`` with a 10 ms hold on top.
The passes alternate call by call, each between device events on the stream, every call on a fresh
copy of the input (the copy is outside the timed span).

Writes one JSON document: per input and pass the mean, the spread (max - min) and every call in
milliseconds, the bytes the pass must move (24 per stereo frame for the local gate and the
compressor: two reads and one write; 32 with the state sweep) and the rate that makes, the share of
reduced and of open frames from the records, and the box.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-suite_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

GRAIN = 64


def measure(a):
    import torch
    from msgpu.dynamics import Dynamics
    from msgpu.engine import default_engine
    from msgpu.gate import Gate, records

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    S, n, sr = a.batch, 48000, 48000
    offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)
    c = 10.0 ** (-1.0 / 20.0)
    gates = {"gate_local": Gate(threshold_db=-6.0, hysteresis_db=0.0, hold_ms=0.0),
             "gate_hysteresis": Gate(threshold_db=-6.0, hysteresis_db=6.0, hold_ms=0.0),
             "gate_hysteresis_hold": Gate(threshold_db=-6.0, hysteresis_db=6.0, hold_ms=10.0)}
    comp = Dynamics(threshold_db=-6.0, ratio=3.0, knee_db=0.0)

    def inputs():
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        noise = torch.randn((S * n, 2), generator=g, device=dev, dtype=torch.float32)
        yield "quiet", noise * 0.1
        yield "dense", (noise * 0.5).clamp_(-1.0, 1.0)
        x0 = noise * 0.1
        per = max(1, int(round(0.02 * n / GRAIN)))
        at = torch.randint(0, n - GRAIN, (S, per), generator=g, device=dev) + (torch.arange(S, device=dev) * n).unsqueeze(1)
        idx = (at.unsqueeze(2) + torch.arange(GRAIN, device=dev)).reshape(-1)
        hann = 0.5 - 0.5 * torch.cos(2 * np.pi * (torch.arange(GRAIN, device=dev) + 0.5) / GRAIN)
        burst = (1.5 * hann * torch.cos(0.9 * torch.arange(GRAIN, device=dev))).to(torch.float32)
        x0.index_put_((idx,), burst.repeat(S * per).unsqueeze(1).expand(-1, 2), accumulate=True)
        yield "grains", x0

    def stat(ms, nbytes):
        mean = float(np.mean(ms))
        return {"mean_ms": round(mean, 4), "spread_ms": round(float(max(ms) - min(ms)), 4),
                "calls_ms": [round(float(v), 4) for v in ms], "bytes": nbytes,
                "gb_per_s": round(nbytes / (mean * 1e-3) / 1e9, 1)}

    frame_bytes = S * n * 8
    out = {}
    for name, x0 in inputs():
        x = x0.clone()
        tp = eng.true_peak(x, offs, lens, 2, sr)                  # measured once: the gain sweep alone is timed
        state = {}

        def gate_pass(g):
            def run():
                state["rec"] = eng.gate_apply(x, offs, lens, 2, sr, g)
            return run

        passes = {k: gate_pass(g) for k, g in gates.items()}
        passes.update({"dynamics": lambda: eng.dynamics(x, offs, lens, 2, sr, comp),
                       "truepeak_gain_sweep": lambda: eng.true_peak_gain(x, offs, lens, 2, tp.clone(), None, None,
                                                                         0.25 * c, None)})
        moved = {"gate_local": 3, "gate_hysteresis": 4, "gate_hysteresis_hold": 4, "dynamics": 3, "truepeak_gain_sweep": 2}
        ms = {k: [] for k in passes}
        evs, share = [], {}
        for step in range(a.warmup + a.steps):
            for k, fn in passes.items():
                x.copy_(x0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                if step >= a.warmup:
                    evs.append((k, e0, e1))
                if step == 0 and k in gates:
                    rec = records(state["rec"])
                    share[k] = (round(float(rec["reduced_frames"].sum()) / float(S * n), 5),
                                round(float(rec["open_frames"].sum()) / float(S * n), 5), int(rec["opens"].sum()))
        torch.cuda.synchronize()
        for k, e0, e1 in evs:
            ms[k].append(e0.elapsed_time(e1))
        rows = {k: stat(v, moved[k] * frame_bytes) for k, v in ms.items()}
        for k, v in share.items():
            rows[k]["reduced_share"], rows[k]["open_share"], rows[k]["opens"] = v
        out[name] = rows
        print(json.dumps({name: {k: r["mean_ms"] for k, r in rows.items()}}), flush=True)
        del x, x0
        torch.cuda.empty_cache()
    box = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": getattr(torch.version, "hip", None)}
    return {"signals": S, "frames": n, "sr": sr, "inputs": out, "box": box}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gate_time.json"))
    a = ap.parse_args()
    doc = {"bench": "gate_time", "steps": a.steps, "warmup": a.warmup}
    doc.update(measure(a))
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
