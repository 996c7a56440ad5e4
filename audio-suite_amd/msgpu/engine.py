"""Device engine: one libmsgpu context per (process, device).

``Engine.render_packed`` enqueues one batched render on the current torch
stream and returns the device output tensor (frames x 2, float32,
interleaved L/R).  PyTorch-ROCm is used only as the device-buffer container
and for its stream handle.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from . import _lib as L
from .loudness import _check_rate      # the one loudness-rate check
from .pack import PackedBatch


# msg_digest_rec as a numpy record
DIGEST_DTYPE = np.dtype([("sum_sq", "<f8"), ("peak", "<f8"), ("sum_l", "<f8"), ("sum_r", "<f8"),
                         ("h0", "<u8"), ("h1", "<u8")])

_I64P = C.POINTER(C.c_int64)


class Engine:
    def __init__(self, device: int = 0):
        import torch  # device buffers only

        if not torch.cuda.is_available():
            raise RuntimeError("msgpu needs a HIP device (torch.cuda.is_available() is False)")
        self.torch = torch
        self.device = int(device)
        lib = L.lib()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream()  # initialise the runtime on this device first
            ctx = lib.msg_create(self.device)
        if not ctx:
            raise RuntimeError("msg_create failed: " + lib.msg_last_error(None).decode())
        self._ctx = C.c_void_p(ctx)
        self._lock = threading.Lock()
        self._last_n = 0

    def close(self):
        if getattr(self, "_ctx", None):
            L.lib().msg_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def set_profiling(self, on):
        """False / 0 off, True / 1 every batch, k > 1 every k-th batch of this context."""
        k = 0 if not on else max(1, int(on))
        L.check(L.lib().msg_set_profiling(self._ctx, k), self._ctx)

    def gate(self, peer, wait_stage: int = 2, record_stage: int = 6):
        """Order this context's batches against ``peer``'s (msg_gate): stage
        ``wait_stage`` of each batch waits for the stage ``record_stage`` of the
        peer's latest batch to begin.  ``peer=None`` clears the gate."""
        L.check(L.lib().msg_gate(self._ctx, peer._ctx if peer is not None else None, int(wait_stage),
                                 int(record_stage)), self._ctx)
        self._gate_peer = peer      # the peer context stays alive while this one gates on it

    def stage_times(self):
        """Per profiled batch: [0..9] stage times and [10..17] host clocks in ms, [18] presets
        whose overlap-add ran inside the FIR kernel, [19] float32-chain events, [20] the grains
        the generator wrote for them (fewer when events share a generator stream), [21] the
        events among them that ran a spectral kernel (fewer when events share a spectral key)."""
        arr = (C.c_float * 22)()
        L.check(L.lib().msg_stage_times(self._ctx, arr, 22), self._ctx)
        return list(arr)

    def alloc_output(self, packed: PackedBatch):
        return self.torch.empty((packed.total_frames, 2), dtype=self.torch.float32,
                                device=f"cuda:{self.device}")

    def render_packed(self, packed: PackedBatch, out=None, stream=None):
        """Enqueue the batch; returns the output tensor (not yet synchronised)."""
        torch = self.torch
        if out is None:
            out = self.alloc_output(packed)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < 2 * packed.total_frames:
            raise ValueError("output tensor must be contiguous float32 with 2*frames elements")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        with self._lock:
            st = L.lib().msg_render_batch(
                self._ctx, packed.presets, packed.n, packed.bp_ptr, packed.bp_pairs,
                packed.ir_ptrs, packed.ir_lens, packed.n_irs,
                packed.img_ptrs, packed.img_h, packed.img_w, packed.n_images,
                C.c_void_p(out.data_ptr()), packed._offsets_c, C.c_void_p(stream.cuda_stream))
            L.check(st, self._ctx)
            self._last_n = packed.n
        return out

    def render_batch(self, params_list, out=None):
        packed = PackedBatch(params_list)
        return self.render_packed(packed, out), packed

    def stft_mag_db(self, x, win=2048, hop=256, max_frames=3000, stream=None):
        """Spectrogram of a device float32/float64 tensor (n,) mono or (n, 2) stereo (L/R
        mean): returns a device float64 tensor (frames, win//2 + 1), enqueued on ``stream``."""
        torch = self.torch
        if x.dtype not in (torch.float32, torch.float64) or not x.is_contiguous() or x.device.type != "cuda":
            raise ValueError("x must be a contiguous float32 or float64 device tensor")
        eb = x.element_size()
        channels = 1 if x.dim() == 1 else int(x.shape[1])
        if x.dim() > 2 or channels not in (1, 2):
            raise ValueError("x must be (n,) or (n, 2)")
        n = int(x.shape[0])
        frames = C.c_int32(0)
        lib = L.lib()
        L.check(lib.msg_stft_mag_db(self._ctx, None, eb, n, channels, int(win), int(hop), int(max_frames),
                                    None, C.byref(frames), None), self._ctx)
        S = torch.empty((frames.value, int(win) // 2 + 1), dtype=torch.float64, device=x.device)
        if frames.value == 0:
            return S
        if stream is None:
            stream = torch.cuda.current_stream(x.device)
        with self._lock:
            L.check(lib.msg_stft_mag_db(self._ctx, C.c_void_p(x.data_ptr()), eb, n, channels, int(win), int(hop),
                                        int(max_frames), C.c_void_p(S.data_ptr()), C.byref(frames),
                                        C.c_void_p(stream.cuda_stream)), self._ctx)
        return S

    def fir(self, x, h, out=None, stream=None):
        """Causal FIR y = np.convolve(x, h)[:n] of each row of a device float32 tensor
        (S, n) or (n,), h float64 taps (host); returns (y, (N, P, Q)) enqueued on ``stream``."""
        torch = self.torch
        if x.dtype != torch.float32 or not x.is_contiguous() or x.device.type != "cuda" or x.dim() > 2:
            raise ValueError("x must be a contiguous float32 device tensor (n,) or (S, n)")
        S, n = (1, int(x.shape[0])) if x.dim() == 1 else (int(x.shape[0]), int(x.shape[1]))
        hh = np.ascontiguousarray(h, dtype=np.float64)
        if hh.ndim != 1 or hh.size < 1:
            raise ValueError("h must be a non-empty 1-D array")
        if out is None:
            out = torch.empty_like(x)
        if out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must match x")
        if stream is None:
            stream = torch.cuda.current_stream(x.device)
        shape = (C.c_int32 * 3)()
        with self._lock:
            L.check(L.lib().msg_fir(self._ctx, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), n, S,
                                    hh.ctypes.data_as(C.c_void_p), int(hh.size), shape,
                                    C.c_void_p(stream.cuda_stream)), self._ctx)
        return out, tuple(shape)

    def _signals(self, x, offsets, lens, channels, nonneg=True, names=("x", "lens", "signal", "input")):
        """The checks every per-signal call shares; returns (channels, offsets, lens) as the
        library takes them.  ``nonneg=False`` leaves negative extents to the library;
        ``names``: the caller's words for the tensor, the lengths, one signal and the tensor's role."""
        torch = self.torch
        if x.dtype != torch.float32 or not x.is_contiguous() or x.device.type != "cuda":
            raise ValueError(f"{names[0]} must be a contiguous float32 device tensor")
        channels = int(channels)
        if channels not in (1, 2):
            raise ValueError("channels must be 1 or 2")
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        cnt = np.ascontiguousarray(lens, dtype=np.int64)
        if off.shape != cnt.shape or off.ndim != 1:
            raise ValueError(f"offsets and {names[1]} must be 1-D of one length")
        if off.size and ((nonneg and (int(off.min()) < 0 or int(cnt.min()) < 0)) or
                         int((off + cnt).max()) * channels > x.numel()):
            raise ValueError(f"a {names[2]} extends past the {names[3]} tensor")
        return channels, off, cnt

    def _record(self, rec, x, n, name, maker):
        """The check of a record tensor a caller hands back: ``maker``'s float64 rows, one per signal."""
        if rec.dtype != self.torch.float64 or not rec.is_contiguous() or rec.device != x.device or rec.numel() < 5 * n:
            raise ValueError(f"{name} must be the float64 record tensor of Engine.{maker} on x's device")

    def _signal_call(self, fn, x, channels, off, cnt, *args, stream=None):
        """One per-signal entry point of the library, fn(ctx, x, [channels,] offsets, lens, n,
        *args, stream), on ``stream`` (None: the current stream of x's device) under the
        context's lock; ``args`` as the library takes them.  Returns the stream."""
        if stream is None:
            stream = self.torch.cuda.current_stream(x.device)
        xp, op, cp = C.c_void_p(x.data_ptr()), off.ctypes.data_as(_I64P), cnt.ctypes.data_as(_I64P)
        sp = C.c_void_p(stream.cuda_stream)
        with self._lock:
            if channels is None:
                rc = fn(self._ctx, xp, op, cp, off.size, *args, sp)
            else:
                rc = fn(self._ctx, xp, channels, op, cp, off.size, *args, sp)
            L.check(rc, self._ctx)
        return stream

    def resample(self, x, offsets, lens, channels, up, down, h, out=None, stream=None):
        """msg_resample of signals lying in a device float32 tensor (mono samples or
        interleaved L/R frames, signal i at frame offsets[i] with lens[i] frames):
        each is resampled by up / down with the float64 taps h (resample.design;
        None when up == down, a copy) and the outputs are packed back to back in
        ``out`` (allocated when None; it must not alias x).  Returns (y, out_offsets,
        out_lens), y of shape (frames,) or (frames, 2), enqueued on ``stream``."""
        from .resample import resample_len
        torch = self.torch
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        up, down = int(up), int(down)
        if up < 1 or down < 1:
            raise ValueError("the ratio must be positive")
        out_cnt = np.array([resample_len(n, up, down) for n in cnt], dtype=np.int64)
        out_off = np.concatenate([[0], np.cumsum(out_cnt)[:-1]]).astype(np.int64) if off.size else out_cnt
        total = int(out_cnt.sum())
        if out is None:
            out = torch.empty((total,) if channels == 1 else (total, 2), dtype=torch.float32, device=x.device)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device or \
                out.numel() < total * channels:
            raise ValueError("out must be a contiguous float32 tensor on x's device with room for every output")
        if up != down:
            hh = np.ascontiguousarray(h, dtype=np.float64)
            if hh.ndim != 1 or hh.size % 2 == 0:
                raise ValueError("h must be 1-D with an odd number of taps")
        else:
            hh = None
        self._signal_call(L.lib().msg_resample, x, channels, off, cnt, up, down,
                          None if hh is None else hh.ctypes.data_as(C.c_void_p), 0 if hh is None else int(hh.size),
                          C.c_void_p(out.data_ptr()), out_off.ctypes.data_as(_I64P), stream=stream)
        return out, out_off, out_cnt

    def digest(self, out, offsets, out_n, stream=None):
        """msg_digest of renders lying in a device output tensor ((frames, 2)
        float32, render i at frame offsets[i], out_n[i] frames): one record per
        render reduced on the device (float64 sums, peak, the 128-bit digest);
        only the records (48 B each) are copied back.  Returns a numpy structured
        array with fields sum_sq, peak, sum_l, sum_r, h0, h1."""
        torch = self.torch
        _, off, cnt = self._signals(out, offsets, out_n, 2, False, ("out", "out_n", "render", "output"))
        n = int(off.size)
        rec = torch.empty((max(n, 1), 6), dtype=torch.float64, device=out.device)
        stream = self._signal_call(L.lib().msg_digest, out, None, off, cnt, C.c_void_p(rec.data_ptr()), stream=stream)
        with torch.cuda.stream(stream):
            host = rec.cpu().numpy()       # ordered after the digest on its stream
        return host[:n].copy().view(DIGEST_DTYPE).reshape(n)

    def loudness(self, x, offsets, lens, channels, sr, stream=None):
        """msg_loudness of signals lying in a device float32 tensor (mono samples or
        interleaved L/R frames, signal i at frame offsets[i] with lens[i] frames at sr
        Hz): BS.1770-4 integrated loudness, reduced on the device in float64.
        Returns the device records, a float64 tensor (signals, 5) whose rows are
        msg_loudness_rec (lufs, mean_sq, peak, gain, then n_blocks and n_kept as two
        int32; loudness.records reads them on the host), enqueued on ``stream``."""
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        sr = _check_rate(sr)
        rec = self.torch.empty((int(off.size), 5), dtype=self.torch.float64, device=x.device)
        self._signal_call(L.lib().msg_loudness, x, channels, off, cnt, sr, C.c_void_p(rec.data_ptr()), stream=stream)
        return rec

    def loudness_range(self, x, offsets, lens, channels, sr, hops=False, stream=None):
        """msg_loudness_range of signals lying in a device float32 tensor (as Engine.loudness):
        one measurement for the integrated loudness and for the loudness range and the
        maximum momentary / short-term loudness (lrange.py).  Returns (loud_rec, range_rec),
        float64 device tensors (signals, 5) and (signals, 12) whose rows are msg_loudness_rec
        and msg_lrange_rec (loudness.records / lrange.records read them on the host);
        ``hops``: (loud_rec, range_rec, hop_sums, hop_offsets) with every signal's K-weighted
        100 ms hop sums back to back in one float64 device tensor, signal i's lens[i] // (sr // 10)
        sums from hop_offsets[i].  Enqueued on ``stream``, no host synchronise."""
        torch = self.torch
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        sr = _check_rate(sr)
        n = int(off.size)
        loud = torch.empty((n, 5), dtype=torch.float64, device=x.device)
        rng = torch.empty((n, 12), dtype=torch.float64, device=x.device)
        n_hops = cnt // (sr // 10)
        hop_off = (np.cumsum(n_hops) - n_hops).astype(np.int64)
        buf = torch.empty(max(int(n_hops.sum()), 1), dtype=torch.float64, device=x.device) if hops else None
        self._signal_call(L.lib().msg_loudness_range, x, channels, off, cnt, sr, C.c_void_p(loud.data_ptr()),
                          C.c_void_p(rng.data_ptr()), None if buf is None else C.c_void_p(buf.data_ptr()),
                          hop_off.ctypes.data_as(_I64P), stream=stream)
        if hops:
            return loud, rng, buf[:int(n_hops.sum())], hop_off
        return loud, rng

    def loudness_gain(self, x, offsets, lens, channels, rec, target_lufs, ceiling=None, stream=None):
        """msg_loudness_gain: scale each signal of x in place to ``target_lufs`` from its
        device record (Engine.loudness), the gain formed on the device; ``ceiling``: a
        linear sample peak no scaled signal may exceed (None: no limit).  Writes the
        gains into ``rec`` and returns it; enqueued on ``stream``, no host synchronise."""
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        self._record(rec, x, int(off.size), "rec", "loudness")
        ceil = 0.0 if ceiling is None else float(ceiling)
        if ceiling is not None and not ceil > 0.0:
            raise ValueError("the ceiling must be positive")
        self._signal_call(L.lib().msg_loudness_gain, x, channels, off, cnt, C.c_void_p(rec.data_ptr()),
                          float(target_lufs), ceil, stream=stream)
        return rec

    def true_peak(self, x, offsets, lens, channels, sr, stream=None):
        """msg_truepeak of signals lying in a device float32 tensor (as Engine.loudness):
        the BS.1770-4 Annex 2 true peak at sr Hz.  Returns the device records, a float64
        tensor (signals, 5) whose rows are msg_truepeak_rec (true_peak, peak, dbtp, gain,
        then os and a pad as two int32; truepeak.records reads them on the host),
        enqueued on ``stream``."""
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        sr = int(sr)
        if sr < 1:
            raise ValueError("the sample rate must be positive")
        rec = self.torch.empty((int(off.size), 5), dtype=self.torch.float64, device=x.device)
        self._signal_call(L.lib().msg_truepeak, x, channels, off, cnt, sr, C.c_void_p(rec.data_ptr()), stream=stream)
        return rec

    def true_peak_gain(self, x, offsets, lens, channels, tp_rec, loud_rec=None, target_lufs=None, ceiling_tp=None,
                       ceiling_peak=None, stream=None):
        """msg_truepeak_gain: scale each signal of x in place from its device records, the
        gain formed on the device: to ``target_lufs`` when ``loud_rec`` (Engine.loudness)
        is given, then held under ``ceiling_tp``, a linear true peak, and ``ceiling_peak``,
        a linear sample peak (None: no limit).  Writes the gains into ``tp_rec`` (and
        ``loud_rec``) and returns ``tp_rec``; enqueued on ``stream``, no host synchronise."""
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        n = int(off.size)
        if tp_rec is not None:
            self._record(tp_rec, x, n, "tp_rec", "true_peak")
        if loud_rec is not None:
            self._record(loud_rec, x, n, "loud_rec", "loudness")
        if tp_rec is None:
            raise ValueError("tp_rec must be the float64 record tensor of Engine.true_peak on x's device")
        if (loud_rec is None) != (target_lufs is None):
            raise ValueError("loud_rec and target_lufs go together")
        ceil = []
        for c in (ceiling_tp, ceiling_peak):
            v = 0.0 if c is None else float(c)
            if c is not None and not v > 0.0:
                raise ValueError("a ceiling must be positive")
            ceil.append(v)
        self._signal_call(L.lib().msg_truepeak_gain, x, channels, off, cnt,
                          None if loud_rec is None else C.c_void_p(loud_rec.data_ptr()), C.c_void_p(tp_rec.data_ptr()),
                          0.0 if target_lufs is None else float(target_lufs), ceil[0], ceil[1], stream=stream)
        return tp_rec

    def limit(self, x, offsets, lens, channels, sr, ceiling_tp, lookahead_frames, tp_rec=None, stream=None):
        """msg_limit: the look-ahead true-peak limiter over signals lying in a device float32
        tensor (as Engine.true_peak), in place: each is held under ``ceiling_tp``, a linear
        true peak, with a look-ahead of ``lookahead_frames`` (limit.py).  ``tp_rec``: the
        signals' device records of Engine.true_peak measured on these samples; a signal
        measured under the ceiling is then skipped on the device.  Returns the device
        records, a float64 tensor (signals, 4) whose rows are msg_limit_rec (limit.records
        reads them on the host); enqueued on ``stream``, no host synchronise."""
        torch = self.torch
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        sr, la, c = int(sr), int(lookahead_frames), float(ceiling_tp)
        if sr < 1:
            raise ValueError("the sample rate must be positive")
        n = int(off.size)
        if tp_rec is not None:
            self._record(tp_rec, x, n, "tp_rec", "true_peak")
        rec = torch.empty((n, 4), dtype=torch.float64, device=x.device)
        self._signal_call(L.lib().msg_limit, x, channels, off, cnt, sr, c, la,
                          None if tp_rec is None else C.c_void_p(tp_rec.data_ptr()), C.c_void_p(rec.data_ptr()),
                          stream=stream)
        return rec

    def edges(self, x, offsets, lens, channels, sr, edges, stream=None):
        """msg_edges: silence trim, fades or loop crossfade (edges.Edges, milliseconds taken at
        ``sr`` Hz) over signals lying in a device float32 tensor (as Engine.true_peak), in
        place; nothing is moved.  Returns the device records, an int64 tensor (signals, 8)
        whose rows are msg_edges_rec (edges.records reads them on the host): signal i is
        delivered from frame offsets[i] + start, end - start frames.  Enqueued on ``stream``,
        no host synchronise."""
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        opts = edges.opts(sr)
        rec = self.torch.empty((int(off.size), 8), dtype=self.torch.int64, device=x.device)
        self._signal_call(L.lib().msg_edges, x, channels, off, cnt, C.byref(opts), C.c_void_p(rec.data_ptr()),
                          stream=stream)
        return rec

    def filter(self, x, offsets, lens, channels, sr, flt, reverse=False, stream=None):
        """msg_filter: the biquad cascade of a filter.Filter designed at ``sr`` Hz over signals lying
        in a device float32 tensor (as Engine.true_peak), in place.  ``zero_phase`` filters make the
        forward call and then the reverse call with the same cascade; otherwise ``reverse`` runs the
        one call from each signal's last frame to its first.  Returns x; enqueued on ``stream``, no
        host synchronise."""
        from .filter import _opts
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        sos = flt.design(sr)
        for rev in ((False, True) if flt.zero_phase else (bool(reverse),)):
            opts = _opts(sos, rev)
            self._signal_call(L.lib().msg_filter, x, channels, off, cnt, C.byref(opts), stream=stream)
        return x

    def stereo_meter(self, x, offsets, lens, sr, stream=None):
        """msg_stereo_meter of stereo signals lying in a device float32 tensor (interleaved L/R
        frames, signal i at frame offsets[i] with lens[i] frames at sr Hz): the three float64 sums,
        the correlation and the smallest 400 ms block correlation (stereo.py).  Returns the device
        records, a float64 tensor (signals, 8) whose rows are msg_stereo_rec (stereo.records reads
        them on the host); enqueued on ``stream``, no host synchronise."""
        channels, off, cnt = self._signals(x, offsets, lens, 2)
        sr = _check_rate(sr)
        rec = self.torch.empty((int(off.size), 8), dtype=self.torch.float64, device=x.device)
        if not off.size:                      # no signal: no record to point at
            return rec
        self._signal_call(L.lib().msg_stereo_meter, x, channels, off, cnt, sr, C.c_void_p(rec.data_ptr()), stream=stream)
        return rec

    def stereo(self, x, offsets, lens, stereo, rec=None, out=None, stream=None):
        """msg_stereo: the 2 x 2 matrix of a stereo.Stereo over stereo signals lying in a device
        float32 tensor (as Engine.stereo_meter), in place, or, ``stereo.channels == 1``, its fold row
        into ``out`` (a float32 tensor that does not overlap x; a new (frames, 1) one when None), the
        outputs packed back to back in signal order.  ``rec``: the signals' device records of
        Engine.stereo_meter; a signal with corr < 0 then has its right channel inverted first, on the
        device (``invert="auto"`` needs it).  Returns (x, offsets) or (out, out_offsets); the identity
        launches nothing.  Enqueued on ``stream``, no host synchronise."""
        torch = self.torch
        channels, off, cnt = self._signals(x, offsets, lens, 2)
        m, fold = stereo.matrix_at()
        n = int(off.size)
        if rec is not None and (rec.dtype != torch.float64 or not rec.is_contiguous() or rec.device != x.device or
                                rec.numel() < 8 * n):
            raise ValueError("rec must be the float64 record tensor of Engine.stereo_meter on x's device")
        if stereo.invert == "auto" and rec is None:
            raise ValueError("invert='auto' needs the records of Engine.stereo_meter")
        m = np.ascontiguousarray(m.reshape(4))
        rp = None if rec is None else C.c_void_p(rec.data_ptr())
        if stereo.channels == 2:
            self._signal_call(L.lib().msg_stereo, x, channels, off, cnt, m.ctypes.data_as(C.c_void_p), None, None, None,
                              rp, stream=stream)
            return x, off
        out_off = (np.cumsum(cnt) - cnt).astype(np.int64)
        total = int(cnt.sum())
        if out is None:
            out = torch.empty((total, 1), dtype=torch.float32, device=x.device)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device or out.numel() < total:
            raise ValueError("out must be a contiguous float32 tensor on x's device with room for every output")
        self._signal_call(L.lib().msg_stereo, x, channels, off, cnt, m.ctypes.data_as(C.c_void_p),
                          fold.ctypes.data_as(C.c_void_p), C.c_void_p(out.data_ptr()), out_off.ctypes.data_as(_I64P), rp,
                          stream=stream)
        return out, out_off

    def dynamics(self, x, offsets, lens, channels, sr, dyn, stream=None):
        """msg_dynamics: the compressor of a dynamics.Dynamics (milliseconds taken at ``sr`` Hz) over
        signals lying in a device float32 tensor (as Engine.true_peak), in place.  Returns the device
        records, an int64 tensor (signals, 4) whose rows are msg_dynamics_rec (dynamics.records reads
        them on the host); enqueued on ``stream``, no host synchronise."""
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        opts = dyn.opts(sr)
        rec = self.torch.empty((int(off.size), 4), dtype=self.torch.int64, device=x.device)
        if not off.size:                      # no signal: no record to point at
            return rec
        self._signal_call(L.lib().msg_dynamics, x, channels, off, cnt, C.byref(opts), C.c_void_p(rec.data_ptr()),
                          stream=stream)
        return rec

    def gate_apply(self, x, offsets, lens, channels, sr, gate, stream=None):
        """msg_gate_apply: the gate of a gate.Gate (milliseconds taken at ``sr`` Hz) over signals lying
        in a device float32 tensor (as Engine.true_peak), in place.  Returns the device records, an
        int64 tensor (signals, 6) whose rows are msg_gate_rec (gate.records reads them on the host);
        enqueued on ``stream``, no host synchronise.  (Engine.gate is the stream gate between contexts.)"""
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        opts = gate.opts(sr)
        rec = self.torch.empty((int(off.size), 6), dtype=self.torch.int64, device=x.device)
        if not off.size:                      # no signal: no record to point at
            return rec
        self._signal_call(L.lib().msg_gate_apply, x, channels, off, cnt, C.byref(opts), C.c_void_p(rec.data_ptr()),
                          stream=stream)
        return rec

    def quantize(self, x, offsets, lens, channels, bits, dither="tpdf", seed=0, keys=None, out=None, stream=None,
                 shape=None):
        """msg_quantize of signals lying in a device float32 tensor (as Engine.true_peak):
        ``bits``-bit PCM (16 or 24) with ``dither`` ("tpdf" or "none") from the stream
        (seed, keys[i]) (keys None: key = i), packed little-endian with no padding.
        Returns ``(out, byte_offsets, rec)``: the device bytes (uint8; signal i at
        byte_offsets[i], each rounded up to a multiple of 16; ``out``: a tensor to write
        into instead of a new one), and the device records, an int64 tensor (signals, 4)
        whose rows are msg_pcm_rec (pcm.records reads them on the host).  ``shape``: None,
        or "e3", "lipshitz5" or "f9": msg_quantize_shaped, the same call with noise-shaped
        dither.  Enqueued on ``stream``, no host synchronise."""
        from .pcm import check_bits, dither_code, shape_code
        torch = self.torch
        channels, off, cnt = self._signals(x, offsets, lens, channels)
        bits = check_bits(bits)
        code = dither_code(dither)
        scode = None if shape is None else shape_code(shape)
        n = int(off.size)
        nbytes = cnt * (channels * (bits // 8))
        byte_off = np.zeros(n, dtype=np.int64)
        if n > 1:
            byte_off[1:] = np.cumsum((nbytes[:-1] + 15) // 16 * 16)
        total = int(byte_off[-1] + nbytes[-1]) if n else 0
        if keys is None:
            k = None
        else:
            k = np.ascontiguousarray([int(v) & 0xFFFFFFFFFFFFFFFF for v in keys], dtype=np.uint64)
            if k.shape != off.shape:
                raise ValueError("keys must have one entry per signal")
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device=x.device)
        elif (out.dtype != torch.uint8 or not out.is_contiguous() or out.device != x.device or out.numel() < total or
              out.data_ptr() % 16):
            raise ValueError("out must be a contiguous 16-byte aligned uint8 tensor on x's device, large enough")
        rec = torch.empty((n, 4), dtype=torch.int64, device=x.device)
        tail = (C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(out.data_ptr()),
                byte_off.ctypes.data_as(_I64P), C.c_void_p(rec.data_ptr()))
        if scode is None:
            self._signal_call(L.lib().msg_quantize, x, channels, off, cnt, bits, code, *tail, stream=stream)
        else:
            self._signal_call(L.lib().msg_quantize_shaped, x, channels, off, cnt, bits, code, scode, *tail, stream=stream)
        return out, byte_off, rec

    def flac(self, pcm, byte_offsets, lens, channels, bits, sr, block=4096, md5=True, out=None, stream=None):
        """msg_flac: the FLAC frames of signals lying as packed PCM in a device uint8 tensor, as
        Engine.quantize left them (signal i at byte_offsets[i], a multiple of 16, with lens[i]
        frames of ``channels`` words of ``bits`` bits).  Returns ``(out, rec)``: a uint8 device
        tensor sized for the worst case (``out``: a tensor to write into instead of a new one) in
        which signal i's frames lie at rec[i].byte_off, compact across the batch, and the device
        records, an int64 tensor (signals, 11) whose rows are msg_flac_rec (flac.records reads them on
        the host).  Enqueued on ``stream``, no host synchronise."""
        from .flac import BLOCKS, REC_WORDS, check_rate
        from .pcm import check_bits
        torch = self.torch
        if pcm.dtype != torch.uint8 or not pcm.is_contiguous() or pcm.device.type != "cuda" or pcm.data_ptr() % 16:
            raise ValueError("pcm must be a contiguous 16-byte aligned uint8 device tensor")
        channels, bits, sr = int(channels), check_bits(bits), check_rate(sr)
        if channels not in (1, 2):
            raise ValueError("channels must be 1 or 2")
        if isinstance(block, bool) or block not in BLOCKS:
            raise ValueError("block must be 256, 512, 1024, 2048 or 4096")
        off = np.ascontiguousarray(byte_offsets, dtype=np.int64)
        cnt = np.ascontiguousarray(lens, dtype=np.int64)
        if off.shape != cnt.shape or off.ndim != 1:
            raise ValueError("byte_offsets and lens must be 1-D of one length")
        n = int(off.size)
        frame = channels * (bits // 8)
        if n and (int(off.min()) < 0 or int(cnt.min()) < 0 or int((off + cnt * frame).max()) > pcm.numel()):
            raise ValueError("a signal extends past the pcm tensor")
        if n and int((off & 15).max()):
            raise ValueError("byte_offsets must be multiples of 16")
        lib = L.lib()
        need = sum((int(lib.msg_flac_bound(int(c), channels, bits, int(block))) + 15) // 16 * 16 for c in cnt)
        if out is None:
            out = torch.empty(need, dtype=torch.uint8, device=pcm.device)
        elif (out.dtype != torch.uint8 or not out.is_contiguous() or out.device != pcm.device or out.numel() < need or
              out.data_ptr() % 16):
            raise ValueError("out must be a contiguous 16-byte aligned uint8 tensor on pcm's device, large enough")
        rec = torch.empty((n, REC_WORDS), dtype=torch.int64, device=pcm.device)
        if not n:                             # no signal: no record to point at
            return out, rec
        self._signal_call(lib.msg_flac, pcm, channels, off, cnt, bits, sr, int(block), int(bool(md5)),
                          C.c_void_p(out.data_ptr()), int(out.numel()), C.c_void_p(rec.data_ptr()), stream=stream)
        return out, rec

    # ---- last-batch inspection -----------------------------------------
    def last_plan(self):
        arr = (L.MsgPlanInfo * self._last_n)()
        L.check(L.lib().msg_last_plan(self._ctx, arr, self._last_n), self._ctx)
        return list(arr)

    def last_events(self, preset: int):
        n = C.c_int32(0)
        L.check(L.lib().msg_last_events(self._ctx, preset, None, 0, C.byref(n)), self._ctx)
        arr = (L.MsgEvent * max(n.value, 1))()
        L.check(L.lib().msg_last_events(self._ctx, preset, arr, n.value, C.byref(n)), self._ctx)
        return list(arr)[:n.value]

    def last_grain64(self, preset: int, k: int):
        """Float64 grain of event k of a float64-chain preset of the last batch."""
        n = C.c_int64(0)
        L.check(L.lib().msg_last_grain64(self._ctx, preset, k, None, 0, C.byref(n)), self._ctx)
        g = np.zeros(max(n.value, 1), dtype=np.float64)
        L.check(L.lib().msg_last_grain64(self._ctx, preset, k, g.ctypes.data_as(C.POINTER(C.c_double)), n.value,
                                         C.byref(n)), self._ctx)
        return g[:n.value].copy()

    def last_spec_routes(self):
        """Spectral runs of the last batch per kernel route: {route name: count} over
        _lib.SPEC_ROUTES (msg_last_spec_routes; host bookkeeping, no device work)."""
        arr = (C.c_int64 * len(L.SPEC_ROUTES))()
        L.check(L.lib().msg_last_spec_routes(self._ctx, arr, len(L.SPEC_ROUTES)), self._ctx)
        return dict(zip(L.SPEC_ROUTES, (int(v) for v in arr)))

    def last_meta(self, preset: int, cap: int):
        micro = np.zeros(max(cap, 1), dtype=np.float64)
        grain = np.zeros(max(cap, 1), dtype=np.float64)
        n = C.c_int64(0)
        L.check(L.lib().msg_last_meta(self._ctx, preset, micro.ctypes.data_as(C.POINTER(C.c_double)),
                                      grain.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(n)),
                self._ctx)
        if n.value == 0:
            return None, None
        return micro[:n.value].copy(), grain[:n.value].copy()


_engines: dict = {}
_engines_lock = threading.Lock()


def default_engine(device: int = 0) -> Engine:
    with _engines_lock:
        eng = _engines.get(device)
        if eng is None:
            eng = Engine(device)
            _engines[device] = eng
        return eng
