// host_abi.inc — the host-side entry points of the C ABI (include/msgpu.h): the record
// sizes (msg_sizeof), the render plan (plan.h), the NumPy stream primitives (nprng.h) and
// the host references of the render digest (digest.h), of the loudness and true-peak
// measurements (loudness.h, lrange.h, truepeak.h), of the PCM quantisers (pcm.h, pcm_shape.h) and of the look-ahead
// limiter (limit.h), of the edges pass (edges.h), of the delivery filter (filter.h) and of the stereo
// meter and image (image.h), of the compressor (dynamics.h), of the gate (gate.h) and of the FLAC encoder (flac.h).  Included
// inside extern "C" by msgpu.hip (the product library) and by host_san.cpp (a
// host-only build under AddressSanitizer / UBSan, tests/test_host_sanitizers.py).
// Needs in scope: fail(ctx, code, msg), kHostZig, the ziggurat tables, and the headers
// named above (DigestPart / dg_host, LoudRec / ld_host, LRangeRec / lr_host, TruePeakRec / tp_host, PcmRec / pcm_host,
// LimitRec / lim_host, EdgesRec / edg_host, FilterOpts / fl_host, ImageRec / img_meter_host / img_host,
// DynRec / dyn_host, GateRec / gate_host, FlacRec / flac_host).

int64_t msg_sizeof(int32_t which) {
    switch (which) {
        case 0: return (int64_t)sizeof(msg_preset);
        case 1: return (int64_t)sizeof(msg_event);
        case 2: return (int64_t)sizeof(msg_plan_info);
        case 3: return (int64_t)sizeof(msg_digest_rec);
        case 4: return (int64_t)sizeof(msg_loudness_rec);
        case 5: return (int64_t)sizeof(msg_truepeak_rec);
        case 6: return (int64_t)sizeof(msg_pcm_rec);
        case 7: return (int64_t)sizeof(msg_limit_rec);
        case 8: return (int64_t)sizeof(msg_lrange_rec);
        case 9: return (int64_t)sizeof(msg_edges_rec);
        case 10: return (int64_t)sizeof(msg_edges_opts);
        case 11: return (int64_t)sizeof(msg_filter_opts);
        default: return -1;
    }
}

int msg_plan_host(const msg_preset* preset, const double* bp_bank, const double* ir_frag, int64_t ir_frag_len,
                  msg_plan_info* info, msg_event* events, int32_t max_events,
                  int32_t* er_off, double* er_gain) {
    (void)ir_frag;
    if (!preset || !info) return fail(nullptr, MSG_E_ARG, "null argument");
    for (int l = 0; l < 4; ++l)
        if (preset->n_bp[l] < 0 || (preset->n_bp[l] > 0 && (!bp_bank || preset->bp_off[l] < 0)))
            return fail(nullptr, MSG_E_ARG, "bad breakpoint lane");
    msg_plan_info sz;
    msgplan::plan_sizes(*preset, bp_bank, kHostZig, ir_frag_len, sz);
    *info = sz;
    if (!events) return MSG_OK;
    if (sz.n_slots > max_events) return fail(nullptr, MSG_E_ARG, "event buffer too small");
    const bool er = (preset->flags & MSG_F_ER_CLOUD) != 0;
    msgplan::plan_events(*preset, bp_bank, kHostZig, ir_frag_len, 0, *info, events,
                         er ? er_off : nullptr, er ? er_gain : nullptr);
    return MSG_OK;
}

// The generator's owner assignment (gen_share.h) over every preset of a batch in
// order: owner[slot] for the events at events[slot_base[p] + k], k < n_events[p].
// For the tests of the host function; not part of the ABI.
int msg_debug_gen_owners(const msg_preset* presets, int32_t n_presets, const msg_event* events,
                         const int32_t* slot_base, const int32_t* n_events, int64_t n_slots, int32_t share,
                         int32_t* owner, int64_t* n_owners) {
    if (!presets || !events || !slot_base || !n_events || !owner || n_presets < 0)
        return fail(nullptr, MSG_E_ARG, "bad arguments");
    std::vector<int32_t> list((size_t)n_presets);
    for (int32_t p = 0; p < n_presets; ++p) {
        list[p] = p;
        if (n_events[p] < 0 || slot_base[p] < 0 || (int64_t)slot_base[p] + n_events[p] > n_slots)
            return fail(nullptr, MSG_E_ARG, "events outside the slots");
    }
    genshare::Scratch scratch;
    const int64_t n = genshare::assign(presets, list.data(), n_presets, events, slot_base, n_events, n_slots,
                                       share != 0, owner, scratch);
    if (n_owners) *n_owners = n;
    return MSG_OK;
}

// The spectral owner assignment (gen_share.h, specshare) over the same arguments, every
// preset taken as a float32-chain preset with the default kernel switches:
// owner[slot] is the slot whose grain the event's readers take, the event's own when it
// runs a spectral kernel itself; gen_owner[slot] (optional) the generator's owner.
// The kernel route is taken from specshare::route_standin (the spectral kernels are not
// part of the host-only build).  For the tests of the host function; not part of the ABI.
int msg_debug_spec_owners(const msg_preset* presets, int32_t n_presets, const msg_event* events,
                          const int32_t* slot_base, const int32_t* n_events, int64_t n_slots, int32_t gen_share,
                          int32_t spec_share, int32_t* owner, int32_t* gen_owner, int64_t* n_runs) {
    if (!presets || !events || !slot_base || !n_events || !owner || n_presets < 0)
        return fail(nullptr, MSG_E_ARG, "bad arguments");
    std::vector<int32_t> list((size_t)n_presets);
    for (int32_t p = 0; p < n_presets; ++p) {
        list[p] = p;
        if (n_events[p] < 0 || slot_base[p] < 0 || (int64_t)slot_base[p] + n_events[p] > n_slots)
            return fail(nullptr, MSG_E_ARG, "events outside the slots");
    }
    struct Rec {
        int32_t ops, n, gen_sr;
        double cutoff_gen, roll, stretch, tilt_alpha, env_tau, warp_power;
        int64_t mlast_off;
    };
    std::vector<int32_t> gown((size_t)std::max<int64_t>(n_slots, 1));
    std::vector<Rec> rec((size_t)std::max<int64_t>(n_slots, 1));
    std::vector<int8_t> route((size_t)std::max<int64_t>(n_slots, 1));
    genshare::Scratch gscratch;
    genshare::assign(presets, list.data(), n_presets, events, slot_base, n_events, n_slots, gen_share != 0,
                     gown.data(), gscratch);
    for (int32_t p = 0; p < n_presets; ++p) {
        const specshare::PresetConsts pc = specshare::preset_consts(presets[p]);
        for (int32_t k = 0, s = slot_base[p]; k < n_events[p]; ++k) {
            Rec& x = rec[s + k];
            specshare::key_fields(presets[p], events[s + k], pc, x);
            x.mlast_off = (k == n_events[p] - 1 && (x.ops & (SPEC_TILT_NOISE | SPEC_TILT_SKEW))) ? 0 : -1;
            // preset regions start 16-byte aligned: pool_off carries the offsets' parity
            route[s + k] = specshare::route_standin(x.ops, x.n, events[s + k].pool_off, events[gown[s + k]].pool_off);
            if (gen_owner) gen_owner[s + k] = gown[s + k];
        }
    }
    specshare::Scratch scratch;
    const int64_t n = specshare::assign(rec.data(), route.data(), gown.data(), list.data(), n_presets, slot_base,
                                        n_events, n_slots, gen_share != 0 && spec_share != 0, owner, scratch);
    if (n_runs) *n_runs = n;
    return MSG_OK;
}

// The render digest of one render in host memory: digest.h's fold in the device's order (dg_host)
int msg_digest_host(const float* x, int64_t out_n, msg_digest_rec* rec) {
    static_assert(sizeof(DigestPart) == sizeof(msg_digest_rec), "DigestPart is msg_digest_rec");
    if (!rec || out_n < 0 || (out_n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    DigestPart r;
    dg_host(x, out_n, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// BS.1770-4 integrated loudness of one signal in host memory: the definition of
// loudness.h as one sequential float64 loop (ld_host)
int msg_loudness_host(const float* x, int32_t channels, int64_t n, int32_t sr, msg_loudness_rec* rec) {
    static_assert(sizeof(LoudRec) == sizeof(msg_loudness_rec), "LoudRec is msg_loudness_rec");
    if (!rec || n < 0 || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    if (!ld_rate_ok(sr)) return fail(nullptr, MSG_E_VALUE, "the sample rate must be a multiple of 10, at least 4000");
    LoudRec r;
    ld_host(x, channels, n, sr, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The loudness range and the maximum momentary / short-term loudness from given hop sums:
// the definition of lrange.h in plain C++ (lr_hops_host)
int msg_lrange_hops_host(const double* hops, int64_t n_hops, int64_t hop, msg_lrange_rec* rec) {
    static_assert(sizeof(LRangeRec) == sizeof(msg_lrange_rec), "LRangeRec is msg_lrange_rec");
    if (!rec || n_hops < 0 || hop < 1 || (n_hops > 0 && !hops)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    LRangeRec r;
    lr_hops_host(hops, n_hops, hop, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The same of one signal in host memory: ld_host's loop, then lr_hops_host on its hop sums (lr_host)
int msg_loudness_range_host(const float* x, int32_t channels, int64_t n, int32_t sr, msg_loudness_rec* loud_rec,
                            msg_lrange_rec* range_rec) {
    if (!range_rec || n < 0 || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    if (!ld_rate_ok(sr)) return fail(nullptr, MSG_E_VALUE, "the sample rate must be a multiple of 10, at least 4000");
    LoudRec l;
    LRangeRec r;
    lr_host(x, channels, n, sr, &l, &r);
    if (loud_rec) std::memcpy(loud_rec, &l, sizeof(l));
    std::memcpy(range_rec, &r, sizeof(r));
    return MSG_OK;
}

// BS.1770-4 true peak of one signal in host memory: the definition of truepeak.h as
// one loop (tp_host), the float32 arithmetic and the record of the device to the bit
int msg_truepeak_host(const float* x, int32_t channels, int64_t n, int32_t sr, msg_truepeak_rec* rec) {
    static_assert(sizeof(TruePeakRec) == sizeof(msg_truepeak_rec), "TruePeakRec is msg_truepeak_rec");
    if (!rec || n < 0 || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    if (sr < 1) return fail(nullptr, MSG_E_VALUE, "the sample rate must be positive");
    TruePeakRec r;
    tp_host(x, channels, n, sr, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// Fixed-point PCM of one signal in host memory: the definition of pcm.h word by word
// (pcm_host), the device's bytes and record to the bit
int msg_quantize_host(const float* x, int32_t channels, int64_t n, int32_t bits, int32_t dither, uint64_t seed,
                      uint64_t key, void* out, msg_pcm_rec* rec) {
    static_assert(sizeof(PcmRec) == sizeof(msg_pcm_rec), "PcmRec is msg_pcm_rec");
    static_assert(PCM_DITHER_NONE == MSG_DITHER_NONE && PCM_DITHER_TPDF == MSG_DITHER_TPDF, "the dither codes");
    if (!rec || n < 0 || (n > 0 && (!x || !out))) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    if (!pcm_bits_ok(bits)) return fail(nullptr, MSG_E_VALUE, "bits must be 16 or 24");
    if (!pcm_dither_ok(dither)) return fail(nullptr, MSG_E_VALUE, "dither must be MSG_DITHER_NONE or MSG_DITHER_TPDF");
    PcmRec r;
    pcm_host(x, channels, n, bits, dither, seed, key, out, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The same with noise-shaped dither: the error-feedback loop of pcm_shape.h (pcm_shape_host), the
// device's bytes and record to the bit
int msg_quantize_shaped_host(const float* x, int32_t channels, int64_t n, int32_t bits, int32_t dither, int32_t shape,
                             uint64_t seed, uint64_t key, void* out, msg_pcm_rec* rec) {
    static_assert(PCM_SHAPE_E3 == MSG_SHAPE_E3 && PCM_SHAPE_LIPSHITZ5 == MSG_SHAPE_LIPSHITZ5 &&
                  PCM_SHAPE_F9 == MSG_SHAPE_F9, "the shape codes");
    if (!rec || n < 0 || (n > 0 && (!x || !out))) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    if (!pcm_bits_ok(bits)) return fail(nullptr, MSG_E_VALUE, "bits must be 16 or 24");
    if (!pcm_dither_ok(dither)) return fail(nullptr, MSG_E_VALUE, "dither must be MSG_DITHER_NONE or MSG_DITHER_TPDF");
    if (!pcm_shape_ok(shape)) return fail(nullptr, MSG_E_VALUE, "shape must be MSG_SHAPE_E3, MSG_SHAPE_LIPSHITZ5 or MSG_SHAPE_F9");
    PcmRec r;
    pcm_shape_host(x, channels, n, bits, dither, shape, seed, key, out, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The value checks msg_limit and msg_limit_host share, in their order
static int lim_values(msg_ctx* ctx, int32_t sr, double ceiling_tp, int32_t lookahead_frames) {
    if (sr < 1) return fail(ctx, MSG_E_VALUE, "the sample rate must be positive");
    if (!(ceiling_tp > 0.0) || !std::isfinite(ceiling_tp) || !((float)ceiling_tp > 0.0f) || !std::isfinite((float)ceiling_tp))
        return fail(ctx, MSG_E_VALUE, "the ceiling must be a finite positive number");
    if (lookahead_frames < 1) return fail(ctx, MSG_E_VALUE, "the look-ahead must be at least one frame");
    if (lookahead_frames > LIM_L_MAX) return fail(ctx, MSG_E_UNSUPPORTED, "look-ahead beyond 4096 frames");
    return MSG_OK;
}

// The look-ahead limiter over one signal in host memory, in place: the definition of
// limit.h as one loop (lim_host), the device's samples and record to the bit
int msg_limit_host(float* x, int32_t channels, int64_t n, int32_t sr, double ceiling_tp, int32_t lookahead_frames,
                   msg_limit_rec* rec) {
    static_assert(sizeof(LimitRec) == sizeof(msg_limit_rec), "LimitRec is msg_limit_rec");
    if (!rec || n < 0 || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    if (const int rc = lim_values(nullptr, sr, ceiling_tp, lookahead_frames)) return rc;
    LimitRec r;
    lim_host(x, channels, n, sr, (float)ceiling_tp, lookahead_frames, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The value checks msg_edges and msg_edges_host share, in their order
static int edg_values(msg_ctx* ctx, const msg_edges_opts* o) {
    static_assert(sizeof(EdgesRec) == sizeof(msg_edges_rec), "EdgesRec is msg_edges_rec");
    static_assert(sizeof(EdgesOpts) == sizeof(msg_edges_opts), "EdgesOpts is msg_edges_opts");
    static_assert(EDG_HEAD == MSG_EDGES_HEAD && EDG_TAIL == MSG_EDGES_TAIL && EDG_SILENT == MSG_EDGES_SILENT,
                  "the side and flag codes");
    static_assert(EDG_LINEAR == MSG_CURVE_LINEAR && EDG_HANN == MSG_CURVE_HANN && EDG_QSIN == MSG_CURVE_QSIN,
                  "the curve codes");
    if (o->sides < 0 || o->sides > (MSG_EDGES_HEAD | MSG_EDGES_TAIL))
        return fail(ctx, MSG_E_VALUE, "sides must be 0 or a sum of MSG_EDGES_HEAD and MSG_EDGES_TAIL");
    if (o->sides && (!std::isfinite(o->trim_db) || o->trim_db > 0.0))
        return fail(ctx, MSG_E_VALUE, "the trim threshold must be a finite number of dB, at most 0");
    if (o->curve != MSG_CURVE_LINEAR && o->curve != MSG_CURVE_HANN && o->curve != MSG_CURVE_QSIN)
        return fail(ctx, MSG_E_VALUE, "curve must be MSG_CURVE_LINEAR, MSG_CURVE_HANN or MSG_CURVE_QSIN");
    for (const int64_t v : {o->pre, o->post, o->fade_in, o->fade_out})
        if (v < 0 || v > EDG_MAX_FRAMES) return fail(ctx, MSG_E_VALUE, "pads and fades must be frame counts from 0 up");
    if (o->loop > EDG_MAX_FRAMES) return fail(ctx, MSG_E_VALUE, "the loop crossfade must be a frame count");
    if (o->loop >= 0 && (o->fade_in > 0 || o->fade_out > 0))
        return fail(ctx, MSG_E_VALUE, "a loop crossfade excludes fades: give one");
    return MSG_OK;
}

// Trim, fades and loop crossfade of one signal in host memory, in place: the definition of
// edges.h as one loop (edg_host), the device's samples and record to the bit
int msg_edges_host(float* x, int32_t channels, int64_t n, const msg_edges_opts* opts, msg_edges_rec* rec) {
    if (!rec || !opts || n < 0 || n > EDG_MAX_FRAMES || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    if (const int rc = edg_values(nullptr, opts)) return rc;
    EdgesOpts o;
    std::memcpy(&o, opts, sizeof(o));
    EdgesRec r;
    edg_host(x, channels, n, edg_par(o), &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The value checks msg_filter and msg_filter_host share
static int fl_values(msg_ctx* ctx, const msg_filter_opts* opts, FilterOpts* o) {
    static_assert(sizeof(FilterOpts) == sizeof(msg_filter_opts), "FilterOpts is msg_filter_opts");
    static_assert(FL_MAX_SECTIONS == MSG_FILTER_MAX_SECTIONS && FL_REVERSE == MSG_FILTER_REVERSE, "the filter's limits and flag");
    std::memcpy(o, opts, sizeof(*o));
    if (const char* why = fl_refused(*o)) return fail(ctx, MSG_E_VALUE, why);
    return MSG_OK;
}

// A biquad cascade over one signal in host memory, in place: the definition of filter.h as
// one sequential float64 loop (fl_host)
int msg_filter_host(float* x, int32_t channels, int64_t n, const msg_filter_opts* opts) {
    if (!opts || n < 0 || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    FilterOpts o;
    if (const int rc = fl_values(nullptr, opts, &o)) return rc;
    fl_host(x, channels, n, o);
    return MSG_OK;
}

// The stereo meter over one signal in host memory: the definition of image.h as one sequential
// float64 loop (img_meter_host)
int msg_stereo_meter_host(const float* x, int32_t channels, int64_t n, int32_t sr, msg_stereo_rec* rec) {
    static_assert(sizeof(ImageRec) == sizeof(msg_stereo_rec), "ImageRec is msg_stereo_rec");
    if (!rec || n < 0 || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 2");
    if (!img_rate_ok(sr)) return fail(nullptr, MSG_E_VALUE, "the sample rate must be a multiple of 10, at least 4000");
    ImageRec r;
    img_meter_host(x, n, sr, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The value checks msg_stereo and msg_stereo_host share: a finite matrix, or a finite fold row
static int img_values(msg_ctx* ctx, const float* matrix, const float* fold) {
    const float* v = fold ? fold : matrix;
    for (int i = 0; i < (fold ? 2 : 4); ++i)
        if (!std::isfinite(v[i])) return fail(ctx, MSG_E_VALUE, "the matrix must be finite");
    return MSG_OK;
}

// The stereo image over one signal in host memory (img_host): the matrix in place, or, fold not
// null, the fold row into y (n floats, no overlap with x), x unchanged.  rec: null, or a meter
// record whose corr < 0 inverts the right channel first.
int msg_stereo_host(float* x, int32_t channels, int64_t n, const float* matrix, const float* fold, float* y,
                    const msg_stereo_rec* rec) {
    if ((!matrix && !fold) || n < 0 || (n > 0 && (!x || (fold && !y)))) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 2");
    if (const int rc = img_values(nullptr, matrix, fold)) return rc;
    if (fold && n > 0) {
        const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
        if (x0 < y0 + (uintptr_t)n * 4 && y0 < x0 + (uintptr_t)n * 8) return fail(nullptr, MSG_E_VALUE, "output ranges overlap");
    }
    const bool flip = rec && rec->corr < 0.0;
    if (!fold && !flip && img_identity(matrix)) return MSG_OK;     // the identity touches nothing
    img_host(x, n, matrix, fold, y, flip);
    return MSG_OK;
}

// The value checks msg_dynamics and msg_dynamics_host share, and the kernels' parameters
static int dyn_values(msg_ctx* ctx, const msg_dynamics_opts* opts, DynPar* par) {
    static_assert(sizeof(DynOpts) == sizeof(msg_dynamics_opts), "DynOpts is msg_dynamics_opts");
    static_assert(sizeof(DynRec) == sizeof(msg_dynamics_rec), "DynRec is msg_dynamics_rec");
    DynOpts o;
    std::memcpy(&o, opts, sizeof(o));
    if (const char* why = dyn_refused(o)) return fail(ctx, MSG_E_VALUE, why);
    if (o.hold_frames > DYN_HOLD_MAX) return fail(ctx, MSG_E_UNSUPPORTED, "hold beyond 4096 frames");
    *par = dyn_par(o);
    return MSG_OK;
}

// The compressor over one signal in host memory, in place: the definition of dynamics.h as one
// sequential loop (dyn_host), the device's samples and record to the bit
int msg_dynamics_host(float* x, int32_t channels, int64_t n, const msg_dynamics_opts* opts, msg_dynamics_rec* rec) {
    if (!rec || !opts || n < 0 || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    DynPar par;
    if (const int rc = dyn_values(nullptr, opts, &par)) return rc;
    DynRec r;
    dyn_host(x, channels, n, par, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The same, and the envelope E per frame into env (n words).  For the tests; not part of the ABI.
int msg_debug_dynamics_env(float* x, int32_t channels, int64_t n, const msg_dynamics_opts* opts, msg_dynamics_rec* rec,
                           int64_t* env) {
    if (!rec || !opts || n < 0 || (n > 0 && (!x || !env))) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    DynPar par;
    if (const int rc = dyn_values(nullptr, opts, &par)) return rc;
    DynRec r;
    dyn_host(x, channels, n, par, &r, env);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}
// dyn_log2 over n positive floats and dyn_exp2 over n doubles.  For the tests; not part of the ABI.
int msg_debug_dyn_log2(const float* p, double* out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) out[i] = dyn_log2(p[i]);
    return MSG_OK;
}
int msg_debug_dyn_exp2(const double* x, double* out, int64_t n) {
    for (int64_t i = 0; i < n; ++i) out[i] = dyn_exp2(x[i]);
    return MSG_OK;
}

// The value checks msg_gate_apply and msg_gate_host share, and the kernels' parameters
static int gate_values(msg_ctx* ctx, const msg_gate_opts* opts, GatePar* par) {
    static_assert(sizeof(GateOpts) == sizeof(msg_gate_opts), "GateOpts is msg_gate_opts");
    static_assert(sizeof(GateRec) == sizeof(msg_gate_rec), "GateRec is msg_gate_rec");
    GateOpts o;
    std::memcpy(&o, opts, sizeof(o));
    if (const char* why = gate_refused(o)) return fail(ctx, MSG_E_VALUE, why);
    *par = gate_par(o);
    return MSG_OK;
}

// The gate over one signal in host memory, in place: the definition of gate.h as one sequential
// loop (gate_host), the device's samples and record to the bit
int msg_gate_host(float* x, int32_t channels, int64_t n, const msg_gate_opts* opts, msg_gate_rec* rec) {
    if (!rec || !opts || n < 0 || (n > 0 && !x)) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    GatePar par;
    if (const int rc = gate_values(nullptr, opts, &par)) return rc;
    GateRec r;
    gate_host(x, channels, n, par, &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The same, the envelope E per frame into env (n words) and the held state sh into held (n bytes).
// For the tests; not part of the ABI.
int msg_debug_gate_env(float* x, int32_t channels, int64_t n, const msg_gate_opts* opts, msg_gate_rec* rec, int64_t* env,
                       uint8_t* held) {
    if (!rec || !opts || n < 0 || (n > 0 && (!x || !env || !held))) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (channels != 1 && channels != 2) return fail(nullptr, MSG_E_VALUE, "channels must be 1 or 2");
    GatePar par;
    if (const int rc = gate_values(nullptr, opts, &par)) return rc;
    GateRec r;
    gate_host(x, channels, n, par, &r, env, held);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

// The value checks msg_flac and msg_flac_host share
static int flac_values(msg_ctx* ctx, int32_t channels, int32_t bits, int32_t sr, int32_t block) {
    static_assert(sizeof(FlacRec) == sizeof(msg_flac_rec) && sizeof(FlacRec) == 88, "FlacRec is msg_flac_rec");
    if (channels != 1 && channels != 2) return fail(ctx, MSG_E_VALUE, "channels must be 1 or 2");
    if (bits != 16 && bits != 24) return fail(ctx, MSG_E_VALUE, "bits must be 16 or 24");
    if (!flac_rate_ok(sr)) return fail(ctx, MSG_E_VALUE, "the sample rate must be from 1 to 655350 Hz");
    if (!flac_block_ok(block)) return fail(ctx, MSG_E_VALUE, "block must be 256, 512, 1024, 2048 or 4096");
    return MSG_OK;
}

int64_t msg_flac_bound(int64_t frames, int32_t channels, int32_t bits, int32_t block) {
    if (frames < 0 || frames > FLAC_MAX_FRAMES || (channels != 1 && channels != 2) || (bits != 16 && bits != 24) ||
        !flac_block_ok(block))
        return -1;
    return flac_bound(frames, channels, bits, block);
}

// FLAC frames of one signal in host memory: the definition of flac.h as one sequential bit writer
// (flac_host), the device's bytes and record to the bit
int msg_flac_host(const void* pcm, int32_t channels, int64_t n, int32_t bits, int32_t sr, int32_t block, int32_t md5,
                  void* out, msg_flac_rec* rec) {
    if (!rec || n < 0 || n > FLAC_MAX_FRAMES || (n > 0 && (!pcm || !out))) return fail(nullptr, MSG_E_ARG, "bad arguments");
    if (const int rc = flac_values(nullptr, channels, bits, sr, block)) return rc;
    FlacRec r;
    flac_host(static_cast<const uint8_t*>(pcm), channels, bits, n, block, sr, md5 != 0, static_cast<uint8_t*>(out), &r);
    std::memcpy(rec, &r, sizeof(r));
    return MSG_OK;
}

int msg_rng_raw(uint64_t seed, uint64_t* out, int64_t n) {
    nprng::Pcg64 g = nprng::default_rng(seed);
    for (int64_t i = 0; i < n; ++i) out[i] = nprng::next_u64(g);
    return MSG_OK;
}
int msg_rng_normal(uint64_t seed, double* out, int64_t n) {
    nprng::Pcg64 g = nprng::default_rng(seed);
    for (int64_t i = 0; i < n; ++i) out[i] = nprng::standard_normal(g, kHostZig);
    return MSG_OK;
}
int msg_rng_exponential(uint64_t seed, double* out, int64_t n) {
    nprng::Pcg64 g = nprng::default_rng(seed);
    for (int64_t i = 0; i < n; ++i) out[i] = nprng::standard_exponential(g, kHostZig);
    return MSG_OK;
}
int msg_rng_integers(uint64_t seed, int64_t low, int64_t high, int64_t* out, int64_t n) {
    if (high <= low) return fail(nullptr, MSG_E_VALUE, "low >= high");
    nprng::Pcg64 g = nprng::default_rng(seed);
    for (int64_t i = 0; i < n; ++i) out[i] = nprng::integers(g, low, high);
    return MSG_OK;
}

// Host emulation of k_gen_normal's chunked walk (same decisions, sequential lanes).
int msg_rng_normal_chunked(uint64_t seed, double* out, int64_t n) {
    const nprng::Pcg64 g0 = nprng::default_rng(seed);
    nprng::Jump ja[64];
    for (int l = 0; l < 64; ++l) ja[l] = nprng::jump_of((uint64_t)l + 1);
    const nprng::Jump j64 = nprng::jump_of(64);
    nprng::u128 st[64];
    for (int l = 0; l < 64; ++l) st[l] = ja[l].a * g0.state + g0.inc * ja[l].s;
    int64_t produced = 0;
    int local = 0;
    while (produced < n) {
        uint64_t rabs[64]; int idx[64]; double x[64]; uint64_t F = 0;
        for (int l = 0; l < 64; ++l) {
            const uint64_t raw = nprng::xsl_rr(st[l]);
            idx[l] = (int)(raw & 0xff);
            const uint64_t rr = raw >> 8;
            rabs[l] = (rr >> 1) & 0x000fffffffffffffULL;
            x[l] = (double)rabs[l] * zig_wi_double[idx[l]];
            if (rr & 1) x[l] = -x[l];
            if (rabs[l] < zig_ki_double[idx[l]]) F |= 1ULL << l;
        }
        while (local < 64 && produced < n) {
            const uint64_t S = ~F & (~0ULL << local);
            const int q = S ? __builtin_ctzll(S) : 64;
            for (int l = local; l < q; ++l) {
                const int64_t j = produced + l - local;
                if (j < n) out[j] = x[l];
            }
            produced += q - local;
            if (q == 64) { local = 64; break; }
            nprng::Pcg64 g;
            g.state = st[q]; g.inc = g0.inc; g.has_u32 = 0; g.u32 = 0;
            // replicate slow_normal (host copy of the same control flow)
            int c = 1;
            uint64_t ra = rabs[q]; int id = idx[q]; double xv = x[q]; double v = 0.0;
            for (;;) {
                if (id == 0) {
                    for (;;) {
                        const double xx = -nprng::ZIG_NOR_INV_R * log1p(-nprng::next_double(g));
                        const double yy = -log1p(-nprng::next_double(g));
                        c += 2;
                        if (yy + yy > xx * xx) { v = ((ra >> 8) & 1) ? -(nprng::ZIG_NOR_R + xx) : nprng::ZIG_NOR_R + xx; break; }
                    }
                    break;
                }
                const double u = nprng::next_double(g);
                c += 1;
                if (((zig_fi_double[id - 1] - zig_fi_double[id]) * u + zig_fi_double[id]) < exp(-0.5 * xv * xv)) { v = xv; break; }
                uint64_t r = nprng::next_u64(g);
                c += 1;
                id = (int)(r & 0xff); r >>= 8;
                const int sign = (int)(r & 1);
                ra = (r >> 1) & 0x000fffffffffffffULL;
                xv = (double)ra * zig_wi_double[id];
                if (sign) xv = -xv;
                if (ra < zig_ki_double[id]) { v = xv; break; }
            }
            if (produced < n) out[produced] = v;
            ++produced;
            local = q + c;
        }
        do {
            for (int l = 0; l < 64; ++l) st[l] = j64.a * st[l] + g0.inc * j64.s;
            local -= 64;
        } while (local >= 64);
    }
    return MSG_OK;
}
