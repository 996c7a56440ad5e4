"""Life cycle of a context (csrc/ctx.h, csrc/dev_own.h): whatever a context
allocates -- device memory, pinned memory, events -- is released by
msg_destroy.  msg_debug_live reports the owners' process-wide counts of what
is live: device allocations, their bytes, pinned allocations, events.  The
counts are compared with their values before the context was created, so
other contexts alive in the process do not matter."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def msgpu():
    import msgpu as m
    return m


def live():
    from msgpu import _lib as L
    fn = L.lib().msg_debug_live
    fn.argtypes = [C.POINTER(C.c_int64)]
    fn.restype = C.c_int
    out = (C.c_int64 * 4)()
    assert fn(out) == 0
    return tuple(out)


def _render(eng, params):
    from msgpu.pack import PackedBatch
    packed = PackedBatch(params)
    return eng.render_packed(packed), packed


def _use_everything(msgpu, irs, monkeypatch):
    """One small batch or call per group of owners; returns the counts while
    both engines are open."""
    import torch
    from msgpu.engine import Engine
    from msgpu.resample import design
    eng = Engine(0)
    eng.set_profiling(1)                                   # the stage events record
    # ER taps + IR: the ER-gain buffers, the filter spectra, the stereo pass
    out, packed = _render(eng, [msgpu.config_params("C3", seed=1000 + s, irs=irs, out_dur_s=0.1) for s in range(2)])
    eng.stage_times()
    eng.set_profiling(False)
    # the float64 chain with its feedback state and float64 plans
    _render(eng, [msgpu.merged(out_dur_s=0.05, seed=3, event_feedback_on=True, spectral_imprint_on=True)])
    # 2205 frames, odd: the Bluestein cache and its scratch
    _, odd = _render(eng, [msgpu.merged(out_dur_s=0.05, seed=4, base_sr=44100)])
    assert int(odd.out_n[0]) % 2 == 1
    x = torch.randn((4, 4096), dtype=torch.float32, device="cuda")
    eng.fir(x, np.hanning(1000))
    eng.digest(out, packed.offsets, packed.out_n)
    eng.resample(x.reshape(-1), [0, 4096], [4096, 4096], 1, 1, 2, design(1, 2))
    eng.stft_mag_db(x.reshape(-1), win=512, hop=128)
    # the float64 FIR of every FIR preset: a switch read when the context is created
    monkeypatch.setenv("MSGPU_FIR64", "2")
    eng64 = Engine(0)
    monkeypatch.delenv("MSGPU_FIR64")
    _render(eng64, [msgpu.config_params("C3", seed=1002, irs=irs, out_dur_s=0.1)])
    torch.cuda.synchronize(0)
    during = live()
    eng.close()
    eng64.close()
    return during


def test_destroy_releases_everything(msgpu, irs, monkeypatch):
    gc.collect()                                           # no stale Engine is collected half way
    base = live()
    for _ in range(2):
        during = _use_everything(msgpu, irs, monkeypatch)
        assert all(d > b for d, b in zip(during, base)), (during, base)   # the counters are alive
        assert live() == base


def test_lru_eviction_frees(msgpu):
    """The Bluestein cache (so_bp) drops least-recently-used spectra beyond
    1 GiB.  An entry is 16 B x the transform length, with a quarter of headroom."""
    import torch
    from msgpu.engine import Engine
    sr, lo, hi = 44100, 0.05, 0.1                          # this file's render sizes
    lengths = [n for n in range(int(lo * sr), int(hi * sr) + 1) if n % 2]
    entry = lambda n: 16 * (1 << (2 * n - 2).bit_length()) * 5 // 4
    if sum(entry(n) for n in lengths) <= 1 << 30:
        pytest.skip("every odd length of a %.2f-%.2f s render together holds %d MiB: the 1 GiB bound is out of reach"
                    % (lo, hi, sum(entry(n) for n in lengths) >> 20))
    eng = Engine(0)
    peak, fell = 0, False
    for n in lengths:
        _render(eng, [msgpu.merged(out_dur_s=n / sr, seed=5, base_sr=sr)])
        torch.cuda.synchronize(0)
        now = live()[1]
        fell = fell or now < peak
        peak = max(peak, now)
    eng.close()
    assert fell


@pytest.mark.parametrize("first", ["peer", "gated"])
def test_gated_contexts_destroy_in_either_order(msgpu, irs, first):
    """A waits on B's gate event.  Destroying B unlinks A; destroying A takes
    it off B's list: neither order leaves a pointer to a dead context in use."""
    import torch
    from msgpu.engine import Engine
    gc.collect()
    base = live()
    a, b = Engine(0), Engine(0)
    a.gate(b, 2, 6)
    params = [msgpu.config_params("C2", seed=2000, irs=irs, out_dur_s=0.05)]
    for e in (b, a):
        _render(e, params)
    torch.cuda.synchronize(0)
    assert all(d > s for d, s in zip(live(), base))
    order = (b, a) if first == "peer" else (a, b)
    order[0].close()
    _render(order[1], params)                              # the survivor renders on, ungated
    torch.cuda.synchronize(0)
    order[1].close()
    assert live() == base
