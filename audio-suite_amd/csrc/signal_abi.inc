// signal_abi.inc — the entry points of the C ABI (include/msgpu.h) that run one pass over
// a ragged batch of signals lying in a device buffer: msg_digest, msg_resample,
// msg_loudness, msg_loudness_range, msg_loudness_gain, msg_truepeak, msg_truepeak_gain, msg_quantize, msg_quantize_shaped, msg_limit,
// msg_edges, msg_filter, msg_stereo_meter, msg_stereo, msg_dynamics, msg_gate_apply, msg_flac.
// Included inside extern "C" by msgpu.hip.  DESIGN.md "Signal passes".
// Needs in scope: fail, HIPCHK, stream_handover, DoneGuard, MSG_MAX_FRAMES, ctx.h.
//
// A new pass supplies its kernels and launcher, its buffers in ctx.h, and an entry point
// here: its own value checks, SignalCall::rows with its tiles-of rule, its tables, the
// launch and finish().

extern "C++" {

// the arguments and the channel count, the first two checks of every pass over 1 or 2 channels
static int sig_args(msg_ctx* ctx, bool pointers_ok, int32_t n_signals, int32_t channels) {
    if (!ctx || !pointers_ok || n_signals < 0) return fail(ctx, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(ctx, MSG_E_VALUE, "channels must be 1 or 2");
    return MSG_OK;
}
// stereo frames are read as 8-byte pairs
static int sig_aligned(msg_ctx* ctx, int32_t channels, const void* x_dev) {
    if (channels == 2 && (reinterpret_cast<uintptr_t>(x_dev) & 7))
        return fail(ctx, MSG_E_ARG, "stereo input must be 8-byte aligned");
    return MSG_OK;
}

// One call of a pass: the meta rows on the host, then the context's device, the stream
// handover, the done guard and the rows' upload.  finish() records the call's end; every
// earlier return does too (DoneGuard) once open() has run.
struct SignalCall {
    msg_ctx* ctx;
    hipStream_t s;
    int64_t tiles = 0;
    std::vector<int64_t> meta;
    std::optional<DoneGuard> done;
    SignalCall(msg_ctx* c, void* stream) : ctx(c), s((hipStream_t)stream) {}

    // meta = [offsets | frames | n + 1 first tiles | extra words for the pass], tiles_of(frames)
    // tiles per signal; TB: the tile row's element (the digest's kernels read int32 bases packed
    // into the int64 upload).  Fails on a bad extent or on more tiles than a grid takes.  No HIP call.
    template <class TB = int64_t, class F>
    int rows(const int64_t* offsets, const int64_t* frames, int32_t n, F tiles_of, const char* unit, const char* what,
             size_t extra = 0) {
        const size_t tile_words = sizeof(TB) == 8 ? (size_t)n + 1 : (size_t)(n + 2) / 2 + 1;
        meta.assign((size_t)2 * n + tile_words + extra, 0);
        TB* tb = reinterpret_cast<TB*>(meta.data() + (size_t)2 * n);
        auto too_many = [&] { return fail(ctx, MSG_E_UNSUPPORTED, std::string("too many ") + what + " tiles"); };
        for (int i = 0; i < n; ++i) {
            if (frames[i] < 0 || frames[i] > MSG_MAX_FRAMES || offsets[i] < 0)
                return fail(ctx, MSG_E_ARG, std::string("bad ") + unit + " extent");
            meta[i] = offsets[i];
            meta[(size_t)n + i] = frames[i];
            tb[i] = (TB)tiles;
            tiles += tiles_of(frames[i]);
            if (sizeof(TB) < 8 && tiles > INT32_MAX) return too_many();   // before a base wraps
        }
        tb[n] = (TB)tiles;
        if (tiles > INT32_MAX) return too_many();
        return MSG_OK;
    }
    int64_t* extra_row(int32_t n, int k) { return meta.data() + (size_t)(3 + k) * n + 1; }   // after int64 tile bases

    int open() {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, stream_handover(ctx, s));
        done.emplace(ctx, s);
        return MSG_OK;
    }
    // a pageable source is staged before hipMemcpyAsync returns (as msg_fir's uploads)
    template <class T>
    int upload(DevBuf<T>& dev, const std::vector<T>& v) {
        HIPCHK(ctx, dev.ensure(v.size()));
        HIPCHK(ctx, hipMemcpyAsync(dev.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, s));
        return MSG_OK;
    }
    int open(DevBuf<int64_t>& dev) {
        if (const int rc = open()) return rc;
        return upload(dev, meta);
    }
    int finish() {
        HIPCHK(ctx, done->finish());
        return MSG_OK;
    }
    size_t parts() const { return (size_t)std::max<int64_t>(1, tiles); }   // per-tile partials: never an empty buffer
};

// [first, last) ranges of bytes or elements the signals' outputs take: MSG_E_VALUE when two overlap
using SigRanges = std::vector<std::pair<int64_t, int64_t>>;
static int sig_disjoint(msg_ctx* ctx, SigRanges& ranges, const char* what) {
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); ++i)
        if (ranges[i].first < ranges[i - 1].second) return fail(ctx, MSG_E_VALUE, std::string(what) + " ranges overlap");
    return MSG_OK;
}

// The quantisers' extra rows: the stream keys (formed here for both paths) and the output offsets, 16-byte
// aligned; ``ranges`` gets every signal's bytes.  The null test and sig_disjoint stay with each, in its order.
static int pcm_rows(SignalCall& c, int32_t channels, const int64_t* n, int32_t n_signals, int32_t bits, uint64_t seed,
                    const uint64_t* keys, const int64_t* out_byte_off, SigRanges& ranges) {
    ranges.reserve((size_t)n_signals);
    for (int i = 0; i < n_signals; ++i) {
        const int64_t o = out_byte_off[i], b = pcm_bytes(n[i] * channels, bits);
        if (o < 0 || (o & 15)) return fail(c.ctx, MSG_E_VALUE, "output offsets must be multiples of 16");
        c.extra_row(n_signals, 0)[i] = (int64_t)pcm_stream_key(seed, keys ? keys[i] : (uint64_t)i);
        c.extra_row(n_signals, 1)[i] = o;
        if (b > 0) ranges.emplace_back(o, o + b);
    }
    return MSG_OK;
}

}  // extern "C++"

int msg_digest(msg_ctx* ctx, const float* out_dev, const int64_t* out_offsets, const int64_t* out_n,
               int32_t n_renders, msg_digest_rec* rec_dev, void* stream) {
    if (!ctx || !out_offsets || !out_n || !rec_dev || n_renders < 0) return fail(ctx, MSG_E_ARG, "bad arguments");
    if (n_renders == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows<int32_t>(out_offsets, out_n, n_renders, digest_tiles, "render", "digest")) return rc;
    if (c.tiles > 0 && !out_dev) return fail(ctx, MSG_E_ARG, "null output buffer");
    if (const int rc = c.open(ctx->dg_meta)) return rc;
    HIPCHK(ctx, ctx->dg_part.ensure(c.parts() * sizeof(msg_digest_rec)));
    const int64_t* dm = ctx->dg_meta.p;
    HIPCHK(ctx, launch_digest(n_renders, (int)c.tiles, c.s, out_dev, dm, dm + n_renders,
                              reinterpret_cast<const int32_t*>(dm + 2 * (size_t)n_renders), ctx->dg_part.p, rec_dev));
    return c.finish();
}

int msg_resample(msg_ctx* ctx, const float* x_dev, int32_t channels, const int64_t* in_offsets, const int64_t* in_n,
                 int32_t n_signals, int32_t up, int32_t down, const double* h, int64_t K, float* y_dev,
                 const int64_t* out_offsets, void* stream) {
    if (const int rc = sig_args(ctx, x_dev && y_dev && in_offsets && in_n && out_offsets, n_signals, channels)) return rc;
    if (up < 1 || down < 1) return fail(ctx, MSG_E_VALUE, "the ratio must be positive");
    if (up != down && (!h || K < 1 || (K & 1) == 0)) return fail(ctx, MSG_E_VALUE, "the tap count must be odd");
    if (up > RS_RATIO_MAX || down > RS_RATIO_MAX)
        return fail(ctx, MSG_E_UNSUPPORTED, "ratio beyond the resampler's limits");
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    RsPlan plan{};
    if (up != down) {
        plan = rs_plan(up, down, K, channels);
        if (plan.kind < 0) return fail(ctx, MSG_E_UNSUPPORTED, "ratio beyond the resampler's tap-table or LDS limit");
    }
    // its own rows (input offsets, input frames, output offsets, first tiles): the output offsets lie
    // in front of the tile row, and the output's extent is checked signal by signal with the input's
    SignalCall c(ctx, stream);
    c.meta.resize((size_t)4 * n_signals);
    int64_t x_end = 0, y_end = 0;
    for (int i = 0; i < n_signals; ++i) {
        if (in_n[i] < 0 || in_n[i] > MSG_MAX_FRAMES || in_offsets[i] < 0 || out_offsets[i] < 0)
            return fail(ctx, MSG_E_ARG, "bad signal extent");
        const int64_t n_out = rs_out_len(in_n[i], up, down);
        if (n_out > MSG_MAX_FRAMES) return fail(ctx, MSG_E_UNSUPPORTED, "output longer than 2^31 - 2^20 frames");
        c.meta[i] = in_offsets[i];
        c.meta[(size_t)n_signals + i] = in_n[i];
        c.meta[(size_t)2 * n_signals + i] = out_offsets[i];
        c.meta[(size_t)3 * n_signals + i] = c.tiles;
        if (up != down) c.tiles += (n_out + plan.tile - 1) / plan.tile;
        x_end = std::max(x_end, in_offsets[i] + in_n[i]);
        y_end = std::max(y_end, out_offsets[i] + n_out);
    }
    if (c.tiles > INT32_MAX) return fail(ctx, MSG_E_UNSUPPORTED, "too many output tiles");
    if (x_dev < y_dev + y_end * channels && y_dev < x_dev + x_end * channels)
        return fail(ctx, MSG_E_ARG, "x and y must not alias");
    if (const int rc = c.open()) return rc;
    if (up == down) {                                       // a copy
        for (int i = 0; i < n_signals; ++i)
            if (in_n[i] > 0)
                HIPCHK(ctx, hipMemcpyAsync(y_dev + out_offsets[i] * channels, x_dev + in_offsets[i] * channels,
                                           sizeof(float) * (size_t)(in_n[i] * channels), hipMemcpyDeviceToDevice, c.s));
        return c.finish();
    }
    if (c.tiles == 0) return c.finish();
    std::vector<float> tab((size_t)plan.tab);
    rs_table(plan, up, down, h, K, tab.data());
    if (const int rc = c.upload(ctx->rs_meta, c.meta)) return rc;
    if (const int rc = c.upload(ctx->rs_tab, tab)) return rc;
    HIPCHK(ctx, launch_resample(plan, channels, (unsigned)c.tiles, c.s, x_dev, y_dev, ctx->rs_meta.p, n_signals,
                                ctx->rs_tab.p, up, down, K));
    return c.finish();
}

int msg_loudness(msg_ctx* ctx, const float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n,
                 int32_t n_signals, int32_t sr, msg_loudness_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && rec_dev, n_signals, channels)) return rc;
    if (!ld_rate_ok(sr)) return fail(ctx, MSG_E_VALUE, "the sample rate must be a multiple of 10, at least 4000");
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    const int64_t hop = sr / 10;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [hop](int64_t f) { return ld_tiles(f, hop); }, "signal", "loudness"))
        return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    std::vector<double> tab(LD_TAB_N);
    ld_table(sr, tab.data());
    if (const int rc = c.open(ctx->ld_meta)) return rc;
    HIPCHK(ctx, ctx->ld_state.ensure(c.parts() * 4 * channels));
    HIPCHK(ctx, ctx->ld_part.ensure(c.parts() * 2));
    if (const int rc = c.upload(ctx->ld_tab, tab)) return rc;
    HIPCHK(ctx, launch_loudness(n_signals, channels, (unsigned)c.tiles, c.s, x_dev, ctx->ld_meta.p, hop, ctx->ld_tab.p,
                                ctx->ld_state.p, ctx->ld_part.p, rec_dev));
    return c.finish();
}

int msg_loudness_range(msg_ctx* ctx, const float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n,
                       int32_t n_signals, int32_t sr, msg_loudness_rec* loud_rec_dev, msg_lrange_rec* range_rec_dev,
                       double* hops_dev, const int64_t* hop_offsets, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && range_rec_dev && (!hops_dev || hop_offsets), n_signals, channels))
        return rc;
    if (!ld_rate_ok(sr)) return fail(ctx, MSG_E_VALUE, "the sample rate must be a multiple of 10, at least 4000");
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    const int64_t hop = sr / 10;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [hop](int64_t f) { return ld_tiles(f, hop); }, "signal", "loudness",
                              (size_t)2 * n_signals))
        return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    // each signal's hop sums (the caller's places, else back to back in the context's buffer) and windows
    int64_t* hop_row = c.extra_row(n_signals, 0);
    int64_t* win_row = c.extra_row(n_signals, 1);
    int64_t n_hops = 0, n_win = 0;
    SigRanges ranges;
    for (int i = 0; i < n_signals; ++i) {
        const int64_t hops = n[i] / hop;
        if (hops_dev && hop_offsets[i] < 0) return fail(ctx, MSG_E_ARG, "bad hop offset");
        hop_row[i] = hops_dev ? hop_offsets[i] : n_hops;
        win_row[i] = n_win;
        if (hops_dev && hops > 0) ranges.emplace_back(hop_offsets[i], hop_offsets[i] + hops);
        n_hops += hops;
        n_win += lr_windows(hops);
    }
    if (const int rc = sig_disjoint(ctx, ranges, "hop")) return rc;
    std::vector<double> tab(LD_TAB_N);
    ld_table(sr, tab.data());
    if (const int rc = c.open(ctx->ld_meta)) return rc;
    HIPCHK(ctx, ctx->ld_state.ensure(c.parts() * 4 * channels));
    HIPCHK(ctx, ctx->ld_part.ensure(c.parts() * 2));
    if (!hops_dev) HIPCHK(ctx, ctx->lr_hops.ensure((size_t)std::max<int64_t>(1, n_hops)));
    HIPCHK(ctx, ctx->lr_win.ensure((size_t)std::max<int64_t>(1, n_win)));
    if (const int rc = c.upload(ctx->ld_tab, tab)) return rc;
    HIPCHK(ctx, launch_loudness_range(n_signals, channels, (unsigned)c.tiles, c.s, x_dev, ctx->ld_meta.p, hop,
                                      ctx->ld_tab.p, ctx->ld_state.p, ctx->ld_part.p, loud_rec_dev,
                                      hops_dev ? hops_dev : ctx->lr_hops.p, ctx->lr_win.p, range_rec_dev));
    return c.finish();
}

int msg_loudness_gain(msg_ctx* ctx, float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n,
                      int32_t n_signals, msg_loudness_rec* rec_dev, double target_lufs, double ceiling, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && rec_dev, n_signals, channels)) return rc;
    if (!std::isfinite(target_lufs) || std::isnan(ceiling)) return fail(ctx, MSG_E_VALUE, "target and ceiling must be numbers");
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [](int64_t f) { return (f + LD_GAIN_TILE - 1) / LD_GAIN_TILE; },
                              "signal", "gain"))
        return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    if (const int rc = c.open(ctx->ld_meta)) return rc;
    HIPCHK(ctx, launch_loudness_gain(n_signals, channels, (unsigned)c.tiles, c.s, x_dev, ctx->ld_meta.p, rec_dev,
                                     target_lufs, ceiling));
    return c.finish();
}

int msg_truepeak(msg_ctx* ctx, const float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n,
                 int32_t n_signals, int32_t sr, msg_truepeak_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && rec_dev, n_signals, channels)) return rc;
    if (sr < 1) return fail(ctx, MSG_E_VALUE, "the sample rate must be positive");
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, tp_tiles, "signal", "true-peak")) return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    if (const int rc = c.open(ctx->tp_meta)) return rc;
    HIPCHK(ctx, ctx->tp_part.ensure(c.parts()));
    HIPCHK(ctx, launch_truepeak(n_signals, channels, tp_os(sr), (unsigned)c.tiles, c.s, x_dev, ctx->tp_meta.p,
                                ctx->d_tp_tab.p, ctx->tp_part.p, rec_dev));
    return c.finish();
}

int msg_truepeak_gain(msg_ctx* ctx, float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n,
                      int32_t n_signals, msg_loudness_rec* loud_rec_dev, msg_truepeak_rec* tp_rec_dev,
                      double target_lufs, double ceiling_tp, double ceiling_peak, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && tp_rec_dev, n_signals, channels)) return rc;
    if ((loud_rec_dev && !std::isfinite(target_lufs)) || std::isnan(ceiling_tp) || std::isnan(ceiling_peak))
        return fail(ctx, MSG_E_VALUE, "target and ceilings must be numbers");
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [](int64_t f) { return (f + TP_GAIN_TILE - 1) / TP_GAIN_TILE; },
                              "signal", "gain"))
        return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    if (const int rc = c.open(ctx->tp_meta)) return rc;
    HIPCHK(ctx, launch_truepeak_gain(n_signals, channels, (unsigned)c.tiles, c.s, x_dev, ctx->tp_meta.p, loud_rec_dev,
                                     tp_rec_dev, loud_rec_dev ? target_lufs : 0.0, ceiling_tp, ceiling_peak));
    return c.finish();
}

int msg_quantize(msg_ctx* ctx, const float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n,
                 int32_t n_signals, int32_t bits, int32_t dither, uint64_t seed, const uint64_t* keys, void* out_dev,
                 const int64_t* out_byte_off, msg_pcm_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && out_byte_off && rec_dev, n_signals, channels)) return rc;
    if (!pcm_bits_ok(bits)) return fail(ctx, MSG_E_VALUE, "bits must be 16 or 24");
    if (!pcm_dither_ok(dither)) return fail(ctx, MSG_E_VALUE, "dither must be MSG_DITHER_NONE or MSG_DITHER_TPDF");
    if ((reinterpret_cast<uintptr_t>(x_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        return fail(ctx, MSG_E_ARG, "the input must be 4-byte and the output 16-byte aligned");
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [channels](int64_t f) { return pcm_tiles(f * channels); }, "signal",
                              "quantiser", (size_t)2 * n_signals))
        return rc;
    if (c.tiles > 0 && (!x_dev || !out_dev)) return fail(ctx, MSG_E_ARG, "null buffer");
    SigRanges ranges;
    if (const int rc = pcm_rows(c, channels, n, n_signals, bits, seed, keys, out_byte_off, ranges)) return rc;
    if (const int rc = sig_disjoint(ctx, ranges, "output")) return rc;
    if (const int rc = c.open(ctx->pcm_meta)) return rc;
    HIPCHK(ctx, ctx->pcm_part.ensure(c.parts()));
    HIPCHK(ctx, launch_pcm(n_signals, channels, bits, dither, (unsigned)c.tiles, c.s, x_dev, ctx->pcm_meta.p, out_dev,
                           ctx->pcm_part.p, rec_dev));
    return c.finish();
}

// msg_quantize with the error feedback of pcm_shape.h: the same arguments, checks and rows; one
// lane per signal walks the signal's chain, so there are no tiles and no partials
int msg_quantize_shaped(msg_ctx* ctx, const float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n,
                        int32_t n_signals, int32_t bits, int32_t dither, int32_t shape, uint64_t seed,
                        const uint64_t* keys, void* out_dev, const int64_t* out_byte_off, msg_pcm_rec* rec_dev,
                        void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && out_byte_off && rec_dev, n_signals, channels)) return rc;
    if (!pcm_bits_ok(bits)) return fail(ctx, MSG_E_VALUE, "bits must be 16 or 24");
    if (!pcm_dither_ok(dither)) return fail(ctx, MSG_E_VALUE, "dither must be MSG_DITHER_NONE or MSG_DITHER_TPDF");
    if (!pcm_shape_ok(shape)) return fail(ctx, MSG_E_VALUE, "shape must be MSG_SHAPE_E3, MSG_SHAPE_LIPSHITZ5 or MSG_SHAPE_F9");
    if ((reinterpret_cast<uintptr_t>(x_dev) & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        return fail(ctx, MSG_E_ARG, "the input must be 4-byte and the output 16-byte aligned");
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [](int64_t) { return (int64_t)0; }, "signal", "quantiser",
                              (size_t)2 * n_signals))
        return rc;
    SigRanges ranges;
    if (const int rc = pcm_rows(c, channels, n, n_signals, bits, seed, keys, out_byte_off, ranges)) return rc;
    if (!ranges.empty() && (!x_dev || !out_dev)) return fail(ctx, MSG_E_ARG, "null buffer");
    if (const int rc = sig_disjoint(ctx, ranges, "output")) return rc;
    if (const int rc = c.open(ctx->pcm_shape_meta)) return rc;
    HIPCHK(ctx, launch_pcm_shape(n_signals, channels, bits, dither, shape, c.s, x_dev, ctx->pcm_shape_meta.p, out_dev,
                                 rec_dev));
    return c.finish();
}

int msg_limit(msg_ctx* ctx, float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n, int32_t n_signals,
              int32_t sr, double ceiling_tp, int32_t lookahead_frames, const msg_truepeak_rec* tp_rec_dev,
              msg_limit_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && rec_dev, n_signals, channels)) return rc;
    if (const int rc = lim_values(ctx, sr, ceiling_tp, lookahead_frames)) return rc;
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    const int L = lookahead_frames;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [L](int64_t f) { return lim_tiles(f, L); }, "signal", "limiter",
                              (size_t)2 * n_signals + 1))
        return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    // each signal's r in the scratch from a multiple of four floats, and the envelope's own tiles
    int64_t* r_row = c.extra_row(n_signals, 0);
    int64_t* env_row = c.extra_row(n_signals, 1);
    int64_t r_floats = 0, env_tiles = 0;
    for (int i = 0; i < n_signals; ++i) {
        r_row[i] = r_floats;
        env_row[i] = env_tiles;
        r_floats += (n[i] + 3) / 4 * 4;
        env_tiles += lim_env_tiles(n[i]);
    }
    env_row[n_signals] = env_tiles;
    if (env_tiles > INT32_MAX) return fail(ctx, MSG_E_UNSUPPORTED, "too many limiter tiles");
    std::vector<float> w((size_t)lim_taps4(L));
    lim_weights(L, w.data());
    if (const int rc = c.open(ctx->lim_meta)) return rc;
    HIPCHK(ctx, ctx->lim_r.ensure((size_t)r_floats + 4));
    HIPCHK(ctx, ctx->lim_nan.ensure((size_t)std::max<int64_t>(1, env_tiles)));
    HIPCHK(ctx, ctx->lim_state.ensure((size_t)n_signals));
    HIPCHK(ctx, ctx->lim_part.ensure(c.parts()));
    if (const int rc = c.upload(ctx->lim_w, w)) return rc;
    HIPCHK(ctx, launch_limit(n_signals, channels, tp_os(sr), (unsigned)env_tiles, (unsigned)c.tiles, c.s, x_dev,
                             ctx->lim_meta.p, ctx->d_tp_tab.p, (float)ceiling_tp, L, ctx->lim_w.p, tp_rec_dev,
                             ctx->lim_r.p, ctx->lim_nan.p, ctx->lim_state.p, ctx->lim_part.p, rec_dev));
    return c.finish();
}

int msg_edges(msg_ctx* ctx, float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n, int32_t n_signals,
              const msg_edges_opts* opts, msg_edges_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && opts && rec_dev, n_signals, channels)) return rc;
    if (const int rc = edg_values(ctx, opts)) return rc;
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    EdgesOpts o;
    std::memcpy(&o, opts, sizeof(o));
    const EdgesPar par = edg_par(o);
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [&par](int64_t f) { return par.sides ? edg_tiles(f) : (int64_t)0; },
                              "signal", "edges", (size_t)n_signals + 1))
        return rc;
    // the apply kernel's own tiles, from bounds that need no measurement
    int64_t* apply_row = c.extra_row(n_signals, 0);
    int64_t apply_tiles = 0, frames = 0;
    for (int i = 0; i < n_signals; ++i) {
        apply_row[i] = apply_tiles;
        apply_tiles += edg_apply_tiles(par, n[i]);
        frames += n[i];
    }
    apply_row[n_signals] = apply_tiles;
    if (apply_tiles > INT32_MAX) return fail(ctx, MSG_E_UNSUPPORTED, "too many edges tiles");
    if (frames > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    if (const int rc = c.open(ctx->edg_meta)) return rc;
    HIPCHK(ctx, launch_edges(n_signals, channels, (unsigned)c.tiles, (unsigned)apply_tiles, c.s, x_dev, ctx->edg_meta.p,
                             par, rec_dev));
    return c.finish();
}

int msg_filter(msg_ctx* ctx, float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n, int32_t n_signals,
               const msg_filter_opts* opts, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && opts, n_signals, channels)) return rc;
    FilterOpts o;
    if (const int rc = fl_values(ctx, opts, &o)) return rc;
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, fl_tiles, "signal", "filter")) return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    // the pass writes where it reads: two signals sharing a frame would filter each other's output
    SigRanges ranges;
    for (int i = 0; i < n_signals; ++i)
        if (n[i] > 0) ranges.emplace_back(offsets[i], offsets[i] + n[i]);
    if (const int rc = sig_disjoint(ctx, ranges, "signal")) return rc;
    if (c.tiles == 0) return MSG_OK;
    std::vector<double> tab(FL_TAB_N);
    fl_table(o, tab.data());
    if (const int rc = c.open(ctx->fl_meta)) return rc;
    HIPCHK(ctx, ctx->fl_state.ensure(c.parts() * 2 * o.n_sections * channels));
    if (const int rc = c.upload(ctx->fl_tab, tab)) return rc;
    HIPCHK(ctx, launch_filter(n_signals, channels, (unsigned)c.tiles, c.s, x_dev, ctx->fl_meta.p, o.n_sections,
                              o.flags & FL_REVERSE, ctx->fl_tab.p, ctx->fl_state.p));
    return c.finish();
}

int msg_stereo_meter(msg_ctx* ctx, const float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n,
                     int32_t n_signals, int32_t sr, msg_stereo_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && rec_dev, n_signals, channels)) return rc;
    if (channels != 2) return fail(ctx, MSG_E_VALUE, "channels must be 2");
    if (!img_rate_ok(sr)) return fail(ctx, MSG_E_VALUE, "the sample rate must be a multiple of 10, at least 4000");
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    const int64_t hop = sr / 10;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, [hop](int64_t f) { return img_tiles(f, hop); }, "signal", "meter"))
        return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    if (const int rc = c.open(ctx->img_meta)) return rc;
    HIPCHK(ctx, ctx->img_part.ensure(c.parts() * 3));
    HIPCHK(ctx, launch_image_meter(n_signals, (unsigned)c.tiles, c.s, x_dev, ctx->img_meta.p, hop, ctx->img_part.p, rec_dev));
    return c.finish();
}

int msg_stereo(msg_ctx* ctx, float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n, int32_t n_signals,
               const float* matrix, const float* fold, float* y_dev, const int64_t* out_offsets,
               const msg_stereo_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && (matrix || fold) && (!fold || out_offsets), n_signals, channels))
        return rc;
    if (channels != 2) return fail(ctx, MSG_E_VALUE, "channels must be 2");
    if (const int rc = img_values(ctx, matrix, fold)) return rc;
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (fold && (reinterpret_cast<uintptr_t>(y_dev) & 3)) return fail(ctx, MSG_E_ARG, "the output must be 4-byte aligned");
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, img_apply_tiles, "signal", "image", fold ? (size_t)n_signals : 0))
        return rc;
    if (c.tiles > 0 && (!x_dev || (fold && !y_dev))) return fail(ctx, MSG_E_ARG, "null buffer");
    // in place the pass writes where it reads; folded, no output may lie on an input or on another output
    SigRanges ranges;
    const int64_t xb = (int64_t)reinterpret_cast<uintptr_t>(x_dev), yb = (int64_t)reinterpret_cast<uintptr_t>(y_dev);
    for (int i = 0; i < n_signals; ++i) {
        if (fold) {
            if (out_offsets[i] < 0) return fail(ctx, MSG_E_ARG, "bad output offset");
            c.extra_row(n_signals, 0)[i] = out_offsets[i];
        }
        if (n[i] == 0) continue;
        ranges.emplace_back(xb + offsets[i] * 8, xb + (offsets[i] + n[i]) * 8);
        if (fold) ranges.emplace_back(yb + out_offsets[i] * 4, yb + (out_offsets[i] + n[i]) * 4);
    }
    if (const int rc = sig_disjoint(ctx, ranges, "signal")) return rc;
    if (c.tiles == 0 || (!fold && !rec_dev && img_identity(matrix))) return MSG_OK;   // the identity launches nothing
    if (const int rc = c.open(ctx->img_meta)) return rc;
    HIPCHK(ctx, launch_image_apply(n_signals, (unsigned)c.tiles, c.s, x_dev, ctx->img_meta.p, matrix, fold, y_dev, rec_dev));
    return c.finish();
}

int msg_dynamics(msg_ctx* ctx, float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n, int32_t n_signals,
                 const msg_dynamics_opts* opts, msg_dynamics_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && opts && rec_dev, n_signals, channels)) return rc;
    DynPar par;
    if (const int rc = dyn_values(ctx, opts, &par)) return rc;
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, dyn_tiles, "signal", "dynamics")) return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    // the pass writes where it reads: two signals sharing a frame would compress each other's output
    SigRanges ranges;
    for (int i = 0; i < n_signals; ++i)
        if (n[i] > 0) ranges.emplace_back(offsets[i], offsets[i] + n[i]);
    if (const int rc = sig_disjoint(ctx, ranges, "signal")) return rc;
    if (const int rc = c.open(ctx->dyn_meta)) return rc;
    HIPCHK(ctx, ctx->dyn_carry.ensure(c.parts() * 4));
    HIPCHK(ctx, ctx->dyn_flag.ensure(c.parts()));
    HIPCHK(ctx, ctx->dyn_state.ensure((size_t)n_signals));
    if (par.hold > 0) HIPCHK(ctx, ctx->dyn_halo.ensure(c.parts() * (size_t)par.hold));
    // the scan runs without a tile too: it initialises the records
    HIPCHK(ctx, launch_dynamics(n_signals, channels, (unsigned)c.tiles, c.s, x_dev, ctx->dyn_meta.p, par, ctx->dyn_carry.p,
                                ctx->dyn_flag.p, ctx->dyn_state.p, rec_dev, par.hold > 0 ? ctx->dyn_halo.p : nullptr));
    return c.finish();
}

int msg_gate_apply(msg_ctx* ctx, float* x_dev, int32_t channels, const int64_t* offsets, const int64_t* n, int32_t n_signals,
                   const msg_gate_opts* opts, msg_gate_rec* rec_dev, void* stream) {
    if (const int rc = sig_args(ctx, offsets && n && opts && rec_dev, n_signals, channels)) return rc;
    GatePar par;
    if (const int rc = gate_values(ctx, opts, &par)) return rc;
    if (const int rc = sig_aligned(ctx, channels, x_dev)) return rc;
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(offsets, n, n_signals, dyn_tiles, "signal", "gate")) return rc;
    if (c.tiles > 0 && !x_dev) return fail(ctx, MSG_E_ARG, "null input buffer");
    // the pass writes where it reads: two signals sharing a frame would gate each other's output
    SigRanges ranges;
    for (int i = 0; i < n_signals; ++i)
        if (n[i] > 0) ranges.emplace_back(offsets[i], offsets[i] + n[i]);
    if (const int rc = sig_disjoint(ctx, ranges, "signal")) return rc;
    if (const int rc = c.open(ctx->gate_meta)) return rc;
    HIPCHK(ctx, ctx->gate_carry.ensure(c.parts() * 4));
    HIPCHK(ctx, ctx->gate_trans.ensure(c.parts() * 4));
    HIPCHK(ctx, ctx->gate_flag.ensure(c.parts()));
    HIPCHK(ctx, ctx->gate_state.ensure((size_t)n_signals));
    // the envelope scan runs without a tile too: it initialises the records
    HIPCHK(ctx, launch_gate(n_signals, channels, (unsigned)c.tiles, c.s, x_dev, ctx->gate_meta.p, par, ctx->gate_carry.p,
                            ctx->gate_trans.p, ctx->gate_flag.p, ctx->gate_state.p, rec_dev));
    return c.finish();
}

int msg_flac(msg_ctx* ctx, const void* pcm_dev, int32_t channels, const int64_t* byte_off, const int64_t* n, int32_t n_signals,
             int32_t bits, int32_t sr, int32_t block, int32_t md5, void* out_dev, int64_t out_bytes, msg_flac_rec* rec_dev,
             void* stream) {
    if (const int rc = sig_args(ctx, byte_off && n && rec_dev && out_bytes >= 0, n_signals, channels)) return rc;
    if (const int rc = flac_values(ctx, channels, bits, sr, block)) return rc;
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 15) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        return fail(ctx, MSG_E_ARG, "the input and the output must be 16-byte aligned");
    if (n_signals == 0) return MSG_OK;
    SignalCall c(ctx, stream);
    if (const int rc = c.rows(byte_off, n, n_signals, [block](int64_t f) { return flac_blocks(f, block); }, "signal", "FLAC"))
        return rc;
    if (c.tiles > 0 && (!pcm_dev || !out_dev)) return fail(ctx, MSG_E_ARG, "null buffer");
    // the blocks are read as aligned words, and the output must hold every signal's worst case
    int64_t need = 0;
    for (int i = 0; i < n_signals; ++i) {
        if (byte_off[i] & 15) return fail(ctx, MSG_E_VALUE, "input offsets must be multiples of 16");
        need += (flac_bound(n[i], channels, bits, block) + 15) & ~(int64_t)15;
    }
    if (need > out_bytes) return fail(ctx, MSG_E_ARG, "the output is smaller than the signals' msg_flac_bound");
    if (const int rc = c.open(ctx->flac_meta)) return rc;
    static_assert(sizeof(FlacPlan) % 8 == 0, "plans lie in int64 words");
    HIPCHK(ctx, ctx->flac_plan.ensure(c.parts() * (sizeof(FlacPlan) / 8)));
    HIPCHK(ctx, ctx->flac_pre.ensure(c.parts()));
    // the scans run without a block too: they write the records
    HIPCHK(ctx, launch_flac(n_signals, channels, bits, block, sr, md5 != 0, (unsigned)c.tiles, c.s, pcm_dev, ctx->flac_meta.p,
                            ctx->flac_plan.p, ctx->flac_pre.p, rec_dev, out_dev, out_bytes));
    return c.finish();
}
