#!/usr/bin/env python3
"""FLAC timing: msg_flac on S x 48 000 stereo frames at 48 kHz, 16 and 24 bits, beside, in the same
session and on the same buffers, msg_quantize and the device-to-host copies an export pays: the
packed PCM bytes without the encoder, the encoded bytes with it.

    python tools/flac_time.py [--batch 1024] [--steps 10] [--out profiles/flac_time.json]

Three inputs: ``grains``, tools/gate_time.py's (noise at 0.1 with seeded Hann grains over full scale
on about 2 % of the frames); ``sine``, a -20 dBFS 440 Hz sine, the right channel at 0.7 of the left;
``noise``, full-scale uniform noise, which no predictor helps: every subframe falls back to
verbatim and the encoded bytes exceed the PCM bytes by the frame headers.

The device passes alternate call by call, each between device events on the stream: ``quantize``
(TPDF), ``flac`` with the MD5 launch and ``flac_nomd5`` without it.  The copies are timed on the
host around a synchronise, ``tensor.cpu()`` as the front ends do it: ``copy_pcm`` the quantiser's
bytes, ``copy_flac`` the encoder's bytes up to the last record's end, after the records were read.

Writes one JSON document: per bit depth and input the mean, the spread (max - min) and every call
in milliseconds, the PCM and encoded byte counts and their ratio, the subframe kinds and stereo
assignments from the records, whether encode plus the smaller copy beats the PCM copy, and the box.
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

GRAIN = 64


def measure(a):
    import torch
    from msgpu.engine import default_engine
    from msgpu.flac import records, total_bytes

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    S, n, sr = a.batch, 48000, 48000
    offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)

    def inputs():
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        x0 = torch.randn((S * n, 2), generator=g, device=dev, dtype=torch.float32) * 0.1
        per = max(1, int(round(0.02 * n / GRAIN)))
        at = torch.randint(0, n - GRAIN, (S, per), generator=g, device=dev) + (torch.arange(S, device=dev) * n).unsqueeze(1)
        idx = (at.unsqueeze(2) + torch.arange(GRAIN, device=dev)).reshape(-1)
        hann = 0.5 - 0.5 * torch.cos(2 * np.pi * (torch.arange(GRAIN, device=dev) + 0.5) / GRAIN)
        burst = (1.5 * hann * torch.cos(0.9 * torch.arange(GRAIN, device=dev))).to(torch.float32)
        x0.index_put_((idx,), burst.repeat(S * per).unsqueeze(1).expand(-1, 2), accumulate=True)
        yield "grains", x0.clamp_(-1.0, 1.0)
        del x0
        t = torch.arange(S * n, device=dev, dtype=torch.float64)
        s = (0.1 * torch.sin(2 * np.pi * 440.0 / sr * t)).to(torch.float32)
        del t
        yield "sine", torch.stack([s, 0.7 * s], dim=1).contiguous()
        del s
        yield "noise", torch.rand((S * n, 2), generator=g, device=dev, dtype=torch.float32) * 2.0 - 1.0

    def stat(ms):
        return {"mean_ms": round(float(np.mean(ms)), 4), "spread_ms": round(float(max(ms) - min(ms)), 4),
                "calls_ms": [round(float(v), 4) for v in ms]}

    out = {}
    for name, x in inputs():
        for bits in (16, 24):
            state = {}

            def quantize():
                state["q"] = eng.quantize(x, offs, lens, 2, bits, "tpdf", 1, out=state.get("q", (None,))[0])

            quantize()
            pcm, byte_off, _ = state["q"]
            frames = torch.empty(0, dtype=torch.uint8, device=dev)

            def flac(md5):
                def run():
                    state["f"] = eng.flac(pcm, byte_off, lens, 2, bits, sr, 4096, md5, out=state["f"][0] if "f" in state else None)
                return run

            passes = {"quantize": quantize, "flac": flac(True), "flac_nomd5": flac(False)}
            ms = {k: [] for k in passes}
            evs = []
            for step in range(a.warmup + a.steps):
                for k, fn in passes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    if step >= a.warmup:
                        evs.append((k, e0, e1))
            torch.cuda.synchronize()
            for k, e0, e1 in evs:
                ms[k].append(e0.elapsed_time(e1))
            passes["flac"]()
            frames, rec = state["f"]
            rec = records(rec)
            total = total_bytes(rec)
            copies = {"copy_pcm": [], "copy_flac": []}
            for step in range(a.warmup + a.steps):
                for k, t in (("copy_pcm", pcm), ("copy_flac", frames[:total])):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    host = t.cpu()
                    torch.cuda.synchronize()
                    if step >= a.warmup:
                        copies[k].append((time.perf_counter() - t0) * 1e3)
                    del host
            rows = {k: stat(v) for k, v in {**ms, **copies}.items()}
            pcm_bytes = int(S * n * 2 * (bits // 8))
            rows.update(pcm_bytes=pcm_bytes, flac_bytes=int(rec["bytes"].sum()), copied_flac_bytes=total,
                        ratio=round(float(rec["bytes"].sum()) / pcm_bytes, 4),
                        subframes={k: int(rec[k].sum()) for k in ("constant", "verbatim", "fixed")},
                        assign=[int(v) for v in rec["assign"].sum(axis=0)])
            for k in ("flac", "flac_nomd5"):
                with_copy = rows[k]["mean_ms"] + rows["copy_flac"]["mean_ms"]
                rows[k + "_plus_copy_ms"] = round(with_copy, 4)
                rows[k + "_beats_pcm_copy"] = bool(with_copy < rows["copy_pcm"]["mean_ms"])
            out.setdefault(name, {})[str(bits)] = rows
            print(json.dumps({name: {bits: {k: (r["mean_ms"] if isinstance(r, dict) and "mean_ms" in r else r)
                                            for k, r in rows.items()}}}), flush=True)
            del state, pcm, frames
        del x
        torch.cuda.empty_cache()
    box = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": getattr(torch.version, "hip", None)}
    return {"signals": S, "frames": n, "sr": sr, "block": 4096, "inputs": out, "box": box}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flac_time.json"))
    a = ap.parse_args()
    doc = {"bench": "flac_time", "steps": a.steps, "warmup": a.warmup}
    doc.update(measure(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
