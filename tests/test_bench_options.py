"""bench.py's run modes: the plain run (headline only), ``--full`` and ``--dump-outputs``.

CPU: the frames --dump-outputs keeps of a buffer above its budget (fixed by the
seed, inside the buffer, first and last block included), and both options on the
launcher's dry-run path.  GPU: one small plain run end to end -- the line holds
the headline fields and none of the ``--full`` parts, and the dumped buffers are
the render of the same presets by msgpu.render_batch's engine.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

FULL_ONLY = ("roofline", "roofline_isolated", "checked", "from_dicts", "cpu_baseline", "dropin_latency", "points",
             "points_summary")


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True,
                       timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    return json.loads(lines[0])


def test_dump_rows_fixed_sample():
    total, budget = 10 * bench.DUMP_BLOCK + 17, 4 * bench.DUMP_BLOCK
    assert bench.dump_rows(budget, budget, 1) is None                 # fits: the whole buffer
    rows = bench.dump_rows(total, budget, 1)
    assert rows.dtype == np.int64 and np.all(np.diff(rows) > 0)
    assert rows[0] == 0 and rows[-1] == total - 1                     # first and last block are in
    assert 8 * len(rows) <= 8 * budget
    assert len(rows) >= budget - bench.DUMP_BLOCK                     # the budget is used (last block is short)
    assert np.array_equal(rows, bench.dump_rows(total, budget, 1))    # same seed, same frames
    assert not np.array_equal(rows, bench.dump_rows(total, budget, 2))
    # whole blocks of consecutive frames
    starts = rows[np.concatenate(([True], np.diff(rows) > 1))]
    assert np.all(starts % bench.DUMP_BLOCK == 0)


def test_headline_dump_fits_its_budget():
    """C3's three sub-batch buffers (341 / 342 presets of 384 000 frames) sampled under 64 MB in all."""
    n = 0
    for i, presets in enumerate((341, 341, 342)):
        rows = bench.dump_rows(presets * 384000, bench.DUMP_BYTES // (8 * 3), bench.DUMP_SEED + i)
        assert rows[-1] == presets * 384000 - 1
        n += 8 * len(rows)
    assert n <= bench.DUMP_BYTES <= 64 << 20


def test_options_on_dry_run(tmp_path):
    """--full and --dump-outputs parse on the launcher path; a dry run renders nothing, so it dumps nothing."""
    d = _run("--gpus", "1", "--steps", "2", "--warmup", "0", "--batch", "2", "--config", "C2", "--dry-run", "5",
             "--full", "--dump-outputs", str(tmp_path / "dump"))
    assert d["dry_run"] is True and not (tmp_path / "dump").exists()


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, irs):
    import msgpu
    steps = 3
    d = _run("--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", "4", "--config", "C2",
             "--dump-outputs", str(tmp_path))
    assert d["steps"] == steps and d["full"] is False and d["n_gpus"] == 1
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    frames = 4 * 192000                                               # C2: 1 s at 192 kHz
    assert d["config"]["frames_per_gpu_step"] == frames
    assert d["value"] == pytest.approx(frames / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert not [k for k in FULL_ONLY if k in d]
    files = sorted(os.listdir(tmp_path))
    assert files == [f"out_sub{i}.npy" for i in range(d["config"]["sub_batches_per_gpu"])]
    outs = [np.load(os.path.join(tmp_path, f)) for f in files]
    assert all(o.dtype == np.float32 and o.ndim == 2 and o.shape[1] == 2 for o in outs)
    got = np.concatenate(outs)
    assert got.shape == (frames, 2)                                   # under the budget: whole buffers
    # the presets the run rendered (seeds 1000..1003), by the drop-in call
    for j in (0, 3):
        ref, _ = msgpu.render(msgpu.config_params("C2", seed=1000 + j, irs=irs))
        mine = got[j * 192000:(j + 1) * 192000]
        print(f"dumped preset {j} vs msgpu.render: max abs diff {float(np.abs(mine - ref).max()):.3e}")
        assert np.array_equal(mine, ref)            # batching and streams do not change results (test_gpu_parity)
