#!/usr/bin/env python3
"""Noise-shaped quantiser timing (tools/pcm_time.py's method): msg_quantize_shaped at 16 bits
with TPDF dither, each shape, on S stereo signals of 48 000, 96 000 and 384 000 frames, timed
with device events on the call's stream after a warm-up.  In the same session and on the same
buffers: msg_quantize with TPDF dither, msg_truepeak_gain's scale sweep (the yardstick, timed
before and after) and the device-to-host copy of the 16-bit output bytes to pageable memory
(host clock around a synchronised copy).  The shaped call is latency-bound, frames times the
dependent path of one step, so each row also carries the time per frame in nanoseconds and in
cycles at the shader clock read from the driver while the kernel runs (null where the driver
shows none).  Last, one lone long signal: 1 x 11 520 000 stereo frames (four minutes at 48 kHz).

    python tools/pcm_shape_time.py [--batch 1024] [--steps 5] [--out profiles/pcm_shape_time.json]

Writes one JSON document.
"""
import argparse
import glob
import json
import os
import re
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-suite_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def shader_mhz():
    """The highest current shader clock the driver shows over its cards, in MHz, or None."""
    best = None
    for path in glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"):
        try:
            with open(path) as f:
                for line in f:
                    m = re.search(r"(\d+)\s*Mhz\s*\*", line, flags=re.I)
                    if m:
                        best = max(best or 0, int(m.group(1)))
        except OSError:
            pass
    return best


class ClockWatch:
    """Samples shader_mhz() every few milliseconds while a block runs; .mhz: the largest seen."""

    def __enter__(self):
        self.mhz, self._stop = None, False
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        return self

    def _run(self):
        while not self._stop:
            v = shader_mhz()
            if v is not None:
                self.mhz = max(self.mhz or 0, v)
            time.sleep(0.005)

    def __exit__(self, *exc):
        self._stop = True
        self._t.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", default="48000,96000,384000", help="frames per signal, comma-separated")
    ap.add_argument("--long", type=int, default=11520000, help="frames of the lone long signal (0: skip)")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pcm_shape_time.json"))
    a = ap.parse_args()
    import torch
    from msgpu.engine import default_engine
    from msgpu.pcm import SHAPES, records

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    S = a.batch

    def timed(fn, steps=None):
        steps = a.steps if steps is None else steps
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with ClockWatch() as watch:
            e0.record(stream)
            for _ in range(steps):
                fn()
            e1.record(stream)
            torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps, watch.mhz

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

    def per_frame(ms, n, mhz):
        ns = ms * 1e6 / n
        return round(ns, 2), (None if mhz is None else round(ns * mhz * 1e-3, 1))

    rows = []
    for n in (int(v) for v in a.frames.split(",")):
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        x = torch.randn((S * n, 2), generator=g, device=dev, dtype=torch.float32) * 0.1
        offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)
        tp = eng.true_peak(x, offs, lens, 2, 384000)
        out = torch.empty(S * n * 4, dtype=torch.uint8, device=dev)   # n * 4 is a multiple of 16 here

        def gain():                        # never binds: g = 1, x keeps its bits
            eng.true_peak_gain(x, offs, lens, 2, tp, ceiling_tp=1e6)

        g0, _ = timed(gain)
        tpdf, _ = timed(lambda: eng.quantize(x, offs, lens, 2, 16, "tpdf", 0, None, out=out))
        row = {"signals": S, "frames": n, "pcm16_tpdf_ms": round(tpdf, 4)}
        for shape in SHAPES:
            ms, mhz = timed(lambda: eng.quantize(x, offs, lens, 2, 16, "tpdf", 0, None, out=out, shape=shape))
            ns, cyc = per_frame(ms, n, mhz)
            row[f"{shape}_ms"] = round(ms, 4)
            row[f"{shape}_ns_per_frame"], row[f"{shape}_cycles_per_frame"], row[f"{shape}_mhz"] = ns, cyc, mhz
            row[f"{shape}_ratio_to_tpdf"] = round(ms / tpdf, 2)
        g1, _ = timed(gain)
        gm = 0.5 * (g0 + g1)
        row["gain_ms"], row["gain_ms_before_after"] = round(gm, 4), [round(g0, 4), round(g1, 4)]
        first = records(eng.quantize(x, offs, lens, 2, 16, "tpdf", 0, None, out=out, shape="f9")[2])[0]
        row["clipped_first"], row["q_max_first"] = int(first["clipped"]), int(first["q_max"])
        row["d2h_copy_pcm16_ms"] = copy_ms(out)
        for shape in SHAPES:
            row[f"{shape}_ratio_to_gain"] = round(row[f"{shape}_ms"] / gm, 2)
            row[f"{shape}_ratio_to_copy"] = round(row[f"{shape}_ms"] / row["d2h_copy_pcm16_ms"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, out

    lone = None
    if a.long > 0:
        n = a.long
        x = torch.randn((n, 2), device=dev, dtype=torch.float32) * 0.1
        out = torch.empty(n * 4, dtype=torch.uint8, device=dev)
        lone = {"signals": 1, "frames": n}
        for shape in SHAPES:
            ms, mhz = timed(lambda: eng.quantize(x, [0], [n], 2, 16, "tpdf", 0, None, out=out, shape=shape), steps=1)
            ns, cyc = per_frame(ms, n, mhz)
            lone[f"{shape}_ms"] = round(ms, 2)
            lone[f"{shape}_ns_per_frame"], lone[f"{shape}_cycles_per_frame"], lone[f"{shape}_mhz"] = ns, cyc, mhz
        lone["pcm16_tpdf_ms"] = round(timed(lambda: eng.quantize(x, [0], [n], 2, 16, "tpdf", 0, None, out=out))[0], 4)
        print(json.dumps(lone), flush=True)

    doc = {"bench": "pcm_shape_time", "steps": a.steps, "warmup": a.warmup, "note": a.note,
           "box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "hip": getattr(torch.version, "hip", None)},
           "rows": rows, "lone_long_signal": lone}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
