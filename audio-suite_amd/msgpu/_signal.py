"""What the per-pass modules' device entry points share (loudness.py, truepeak.py, lrange.py,
limit.py, edges.py, pcm.py, resample.py): one signal onto the device, its records back."""
from __future__ import annotations

import numpy as np


def device_signal(eng, x, in_place=False):
    """x, a host array or a device tensor, (n,) or (n, 2), as (tensor, channels, on_host) for
    the engine's per-signal calls.  A host array is copied as float32 and uploaded.  A device
    tensor is made contiguous, but never for a pass that works ``in_place``: a copy would
    swallow its result, so Engine._signals refuses a non-contiguous one instead."""
    torch = eng.torch
    on_host = not isinstance(x, torch.Tensor)
    if on_host:
        t = torch.from_numpy(np.array(x, dtype=np.float32, order="C")).to(f"cuda:{eng.device}")
    else:
        t = x if in_place else x.contiguous()
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] not in (1, 2)):
        raise ValueError("x must be (n,) or (n, 2)")
    return t, (1 if t.dim() == 1 else int(t.shape[1])), on_host


def read_records(rec, dtype):
    """A device record tensor (one row per signal) as an array of ``dtype`` on the host; waits for it."""
    host = rec.cpu().numpy()
    return host.copy().view(dtype).reshape(host.shape[0])
