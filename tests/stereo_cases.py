"""What tests/test_stereo_host.py and tests/test_gpu_stereo.py share: the meter's tolerances and the
check against a reference record, the samples of the bit-exact image tests, and signals whose
smallest block correlation cannot tie.

Meter tolerances: sll and srr relative 1e-9, slr within 1e-9 sqrt(sll srr), corr and corr_min within
1e-9.  A sequential float64 sum of n <= 2^20 terms is within n 2^-53 = 1.2e-10 of sum |terms|, and
|sum L R| <= sqrt(sll srr), so 1e-9 covers it fourfold; the device's fixed-order tree of float64
partial sums obeys the same bound."""
import math

import numpy as np

TOL = 1e-9
SEPARATION = 1e-6


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_meter(what, got, ref):
    """A record against meter_reference's, at the tolerances of the module's docstring."""
    scale = math.sqrt(ref["sll"] * ref["srr"])
    line = (f"{what}: sll {abs(got['sll'] - ref['sll']) / ref['sll'] if ref['sll'] else 0.0:.2e} srr "
            f"{abs(got['srr'] - ref['srr']) / ref['srr'] if ref['srr'] else 0.0:.2e} slr "
            f"{abs(got['slr'] - ref['slr']) / scale if scale else 0.0:.2e} corr {abs(got['corr'] - ref['corr']):.2e} "
            f"corr_min {abs(got['corr_min'] - ref['corr_min']):.2e} at {int(got['corr_min_block'])} "
            f"kept {int(got['blocks_kept'])}/{int(got['blocks'])}")
    print(line)
    assert abs(got["sll"] - ref["sll"]) <= TOL * ref["sll"] and abs(got["srr"] - ref["srr"]) <= TOL * ref["srr"], what
    assert abs(got["slr"] - ref["slr"]) <= TOL * scale, what
    assert abs(got["corr"] - ref["corr"]) <= TOL and abs(got["corr_min"] - ref["corr_min"]) <= TOL, what
    assert int(got["blocks"]) == ref["blocks"] and int(got["blocks_kept"]) == ref["blocks_kept"], what
    assert int(got["corr_min_block"]) == ref["corr_min_block"], what
    return line


def separated(ref, by=SEPARATION):
    """The reference's own blocks: the minimum lies ``by`` below every other kept block's, so no tie."""
    rho = ref["rho"][~np.isnan(ref["rho"])]
    return len(rho) < 2 or np.sort(rho)[1] - np.sort(rho)[0] >= by


def samples():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((300, 2)).astype(np.float32)
    x[:8] = [[0.0, -0.0], [-0.0, 0.0], [-0.0, -0.0], [1e-45, -1e-45], [3e-39, 1.0], [1e30, -1e30], [1e30, 1e-40],
             [-1.0, 1.0]]
    x[8:16] *= np.float32(1e-38)                                                    # products that land on subnormals
    x[16:24] *= np.float32(1e30)
    return x


def hop_noise(n, hop, seed, scale=0.25):
    """n stereo frames of noise whose correlation is drawn anew for every hop from [-0.9, 0.9], so that no
    two blocks share a correlation: R = c L + sqrt(1 - c^2) N."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 2)) * scale
    c = np.repeat(rng.uniform(-0.9, 0.9, n // hop + 1), hop)[:n]
    return np.stack([a[:, 0], c * a[:, 0] + np.sqrt(1.0 - c * c) * a[:, 1]], axis=1).astype(np.float32)
