#!/usr/bin/env python3
"""Limiter timing: the ceiling steps of the export chain with the look-ahead limiter
(msg_truepeak, msg_limit with the measured records, msg_truepeak, msg_truepeak_gain) on S
stereo signals of 48 000 frames at 48 kHz, 96 000 at 96 kHz and 384 000 at 384 kHz, at the
5 ms default look-ahead.  Every signal is noise at 0.1 with a few seeded Hann grains over the
ceiling, placed so that about 3 % of the frames are limited; one more case at 48 kHz has
nothing over the ceiling.  The yardstick is the gain-only path the limiter replaces,
msg_truepeak + msg_truepeak_gain at the same ceiling, in the same session, timed before and
after; msg_digest on the same buffer is timed too, as tools/truepeak_time.py does.

    python tools/limit_time.py [--batch 1024] [--steps 10] [--out profiles/limit_time.json]

Both paths change the buffer, so every step starts from a fresh copy of the signals; the copy
is outside the timed span (device events around the calls alone, summed over the steps).
Writes one JSON document: per case the milliseconds per call of each path and of msg_limit
alone, the ratios, the share of limited frames from the records, and the box.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "audio-suite_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

GRAIN = 64          # frames of one over-ceiling grain
CEILING_DB = -1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="48000:48000,96000:96000,384000:384000",
                    help="sr:frames per signal, comma-separated")
    ap.add_argument("--lookahead-ms", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "limit_time.json"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    from msgpu import _lib as L
    from msgpu.engine import default_engine
    from msgpu.limit import lookahead_frames, records, tile
    from msgpu.truepeak import Z

    eng = default_engine(0)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    S = a.batch
    c = 10.0 ** (CEILING_DB / 20.0)

    def timed(fn, x, x0):
        """ms per call of fn, each call on a fresh copy of x0 in x, the copies not timed."""
        total = 0.0
        for k in range(a.warmup + a.steps):
            x.copy_(x0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            if k >= a.warmup:
                total += e0.elapsed_time(e1)
        return total / a.steps

    cases = [(int(s.split(":")[0]), int(s.split(":")[1]), True) for s in a.shapes.split(",")]
    cases.append((cases[0][0], cases[0][1], False))
    rows = []
    for sr, n, grains in cases:
        la = lookahead_frames(sr, a.lookahead_ms)
        g = torch.Generator(device=dev)
        g.manual_seed(0)
        x0 = torch.randn((S * n, 2), generator=g, device=dev, dtype=torch.float32) * 0.1
        if grains:
            # one grain limits GRAIN + 2 (2 L + Z) frames and a bit: as many grains as 3 % of the signal takes
            per = max(1, int(round(0.03 * n / (GRAIN + 2 * (2 * la + Z)))))
            at = torch.randint(0, n - GRAIN, (S, per), generator=g, device=dev) + \
                (torch.arange(S, device=dev) * n).unsqueeze(1)
            idx = (at.unsqueeze(2) + torch.arange(GRAIN, device=dev)).reshape(-1)
            hann = 0.5 - 0.5 * torch.cos(2 * np.pi * (torch.arange(GRAIN, device=dev) + 0.5) / GRAIN)
            burst = (1.5 * hann * torch.cos(0.9 * torch.arange(GRAIN, device=dev))).to(torch.float32)
            x0.index_put_((idx,), burst.repeat(S * per).unsqueeze(1).expand(-1, 2), accumulate=True)
        x = torch.empty_like(x0)
        offs, lens = np.arange(S, dtype=np.int64) * n, np.full(S, n, dtype=np.int64)
        state = {}

        def limiter_path():
            t = eng.true_peak(x, offs, lens, 2, sr)
            state["rec"] = eng.limit(x, offs, lens, 2, sr, c, la, tp_rec=t)
            t2 = eng.true_peak(x, offs, lens, 2, sr)
            eng.true_peak_gain(x, offs, lens, 2, t2, None, None, c, None)

        def limit_alone():
            eng.limit(x, offs, lens, 2, sr, c, la)

        def gain_only():
            t = eng.true_peak(x, offs, lens, 2, sr)
            eng.true_peak_gain(x, offs, lens, 2, t, None, None, c, None)

        drec = torch.empty((S, 6), dtype=torch.float64, device=dev)
        po, pn = offs.ctypes.data_as(C.POINTER(C.c_int64)), lens.ctypes.data_as(C.POINTER(C.c_int64))

        def digest():                      # msg_digest alone: Engine.digest also copies the records back
            L.check(L.lib().msg_digest(eng._ctx, C.c_void_p(x.data_ptr()), po, pn, S, C.c_void_p(drec.data_ptr()),
                                       C.c_void_p(stream.cuda_stream)), eng._ctx)

        # one session; the yardsticks are timed before and after the limiter's calls
        g0, d0 = timed(gain_only, x, x0), timed(digest, x, x0)
        ms = timed(limiter_path, x, x0)
        rec = records(state["rec"])
        ms_alone = timed(limit_alone, x, x0)
        g1, d1 = timed(gain_only, x, x0), timed(digest, x, x0)
        gain, dg = 0.5 * (g0 + g1), 0.5 * (d0 + d1)
        limited = int(rec["limited_frames"].sum())
        rows.append({"sr": sr, "signals": S, "frames": n, "lookahead": la, "tile": tile(la), "grains": bool(grains),
                     "limited_share": round(limited / float(S * n), 5),
                     "signals_limited": int((rec["state"] == 1).sum()),
                     "min_gain": float(rec["min_gain"].min()),
                     "limiter_path_ms": round(ms, 4), "limit_alone_ms": round(ms_alone, 4),
                     "gain_only_ms": round(gain, 4), "gain_only_ms_before_after": [round(g0, 4), round(g1, 4)],
                     "digest_ms": round(dg, 4), "digest_ms_before_after": [round(d0, 4), round(d1, 4)],
                     "ratio_to_gain_only": round(ms / gain, 3), "limit_alone_ratio_to_gain_only": round(ms_alone / gain, 3),
                     "ratio_to_digest": round(ms / dg, 3)})
        print(json.dumps(rows[-1]), flush=True)
        del x, x0
    doc = {"bench": "limit_time", "steps": a.steps, "warmup": a.warmup, "ceiling_dbtp": CEILING_DB,
           "lookahead_ms": a.lookahead_ms,
           "box": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "hip": getattr(torch.version, "hip", None)},
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
