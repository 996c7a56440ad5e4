// render_stages.h — host: the stages of msg_render_batch, in the
// order the call runs them.  Part of msgpu.hip, included once after msg_ctx
// (ctx.h), HIPCHK, fail() and the plan caches; not a stand-alone header.  Each stage is
// a static int f(msg_ctx*, Batch&) that returns MSG_OK or the failure code
// (with the context's error text set).
#pragma once

// ---------------------------------------------------------------------------
// check
// ---------------------------------------------------------------------------
static int stage_check(msg_ctx* ctx, Batch& b) {
    for (int p = 0; p < b.P; ++p) {
        for (int l = 0; l < 4; ++l) {   // lanes inside the breakpoint bank
            const int32_t nb = b.presets[p].n_bp[l], ob = b.presets[p].bp_off[l];
            if (nb < 0 || (nb > 0 && (!b.bp_bank || ob < 0 || (int64_t)ob + nb > b.bp_pairs)))
                return fail(ctx, MSG_E_ARG, "preset " + std::to_string(p) + ": breakpoint lane outside the bank");
        }
        const int ic = b.presets[p].ir_conv;
        if (ic >= b.n_irs || (ic >= 0 && !b.irs)) return fail(ctx, MSG_E_ARG, "bad IR index");
    }
    return MSG_OK;
}

// ---------------------------------------------------------------------------
// plan: sizes, then events + ER taps, on the host pool or on the device
// ---------------------------------------------------------------------------
// Event-slot and tap bases of the presets from the planned sizes.
static int plan_bases(msg_ctx* ctx, Batch& b) {
    b.nslots = b.ntaps = 0;
    int64_t frames = 0;
    for (int p = 0; p < b.P; ++p) {
        b.slot_base[p] = (int32_t)b.nslots;
        b.tap_base[p] = (int32_t)b.ntaps;
        b.nslots += b.info[p].n_slots;
        if (b.presets[p].flags & MSG_F_ER_CLOUD) b.ntaps += std::max(1, b.presets[p].er_taps);
        // kernels index a preset's frames with 32-bit integers (byte offsets
        // from a tile's or block's own base; the tile counters of a batch in 32 bits)
        if (b.info[p].out_n > MSG_MAX_FRAMES) return fail(ctx, MSG_E_UNSUPPORTED, "output longer than 2^31 - 2^20 frames");
        frames += b.info[p].out_n;
    }
    if (b.nslots > INT32_MAX / 2) return fail(ctx, MSG_E_UNSUPPORTED, "too many events in one batch");
    if (frames > ((int64_t)1 << 40)) return fail(ctx, MSG_E_UNSUPPORTED, "more than 2^40 frames in one batch");
    return MSG_OK;
}

// Host plan (plan.h, the device planner's code) on the host pool: no device
// round trip, so the call returns once the batch is enqueued.
static int plan_host(msg_ctx* ctx, Batch& b) {
    HostPool& pool = HostPool::get();
    pool.run(b.P, [&](int p) { msgplan::plan_sizes(b.presets[p], b.bp_bank, kHostZig, b.flen[p], b.info[p]); });
    b.hA = Batch::hclock::now();
    if (int st = plan_bases(ctx, b)) return st;
    ctx->h_events.resize(b.nslots);
    ctx->h_er_off.resize(b.ntaps);
    if (ctx->sw.er_dev) {
        ctx->h_er_key.resize(b.ntaps);
        ctx->h_er_first.resize(b.ntaps);
        ctx->h_er_cnt.resize(b.ntaps);
    } else {
        ctx->h_er_gain.resize(b.ntaps);
    }
    // offsets only: the gains (two thirds of the host plan of a 320-tap preset,
    // a float64 exp each) are drawn on the device by k_er_gains
    pool.run(b.P, [&](int p) {
        const bool er = (b.presets[p].flags & MSG_F_ER_CLOUD) != 0;
        msgplan::plan_events(b.presets[p], b.bp_bank, kHostZig, b.flen[p], p, b.info[p],
                             ctx->h_events.data() + b.slot_base[p], er ? ctx->h_er_off.data() + b.tap_base[p] : nullptr,
                             (er && !ctx->sw.er_dev) ? ctx->h_er_gain.data() + b.tap_base[p] : nullptr, true);
    });
    return MSG_OK;
}

// Device plan (MSGPU_DEVICE_PLAN=1): k_plan_sizes, the bases, k_plan_events, read back.
static int plan_device(msg_ctx* ctx, Batch& b) {
    const int P = b.P;
    hipStream_t s = b.s;
    // ---- phase 1: sizes ----
    HIPCHK(ctx, ctx->frag_len.ensure(P));
    HIPCHK(ctx, ctx->info.ensure(P));
    HIPCHK(ctx, ctx->dp_presets.ensure(P));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dp_presets.p, b.presets, sizeof(msg_preset) * P, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->frag_len.p, b.flen.data(), sizeof(int64_t) * P, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, ctx->dp_bp.ensure((size_t)std::max<int64_t>(1, 2 * b.bp_pairs)));
    if (b.bp_pairs > 0)
        HIPCHK(ctx, hipMemcpyAsync(ctx->dp_bp.p, b.bp_bank, sizeof(double) * 2 * b.bp_pairs, hipMemcpyHostToDevice, s));
    const int pb = 64;
    hipLaunchKernelGGL(k_plan_sizes, dim3((P + pb - 1) / pb), dim3(pb), 0, s,
                       ctx->dp_presets.p, P, ctx->dp_bp.p, ctx->frag_len.p, ctx->dzig, ctx->info.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(b.info.data(), ctx->info.p, sizeof(msg_plan_info) * P, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    // ---- phase 2: events + ER taps ----
    if (int st = plan_bases(ctx, b)) return st;
    const int64_t nslots = b.nslots, ntaps = b.ntaps;
    HIPCHK(ctx, ctx->slot_base.ensure(P));
    HIPCHK(ctx, ctx->tap_base.ensure(P));
    HIPCHK(ctx, ctx->dp_events.ensure(nslots));
    HIPCHK(ctx, ctx->dp_er_off.ensure(ntaps));
    HIPCHK(ctx, ctx->dp_er_gain.ensure(ntaps));
    HIPCHK(ctx, hipMemcpyAsync(ctx->slot_base.p, b.slot_base.data(), sizeof(int32_t) * P, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->tap_base.p, b.tap_base.data(), sizeof(int32_t) * P, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_plan_events, dim3((P + pb - 1) / pb), dim3(pb), 0, s,
                       ctx->dp_presets.p, P, ctx->dp_bp.p, ctx->frag_len.p, ctx->dzig, ctx->slot_base.p,
                       ctx->tap_base.p,
                       ctx->dp_events.p, ctx->dp_er_off.p, ctx->dp_er_gain.p, ctx->info.p);
    HIPCHK(ctx, hipGetLastError());
    ctx->h_events.resize(nslots);
    HIPCHK(ctx, hipMemcpyAsync(b.info.data(), ctx->info.p, sizeof(msg_plan_info) * P, hipMemcpyDeviceToHost, s));
    if (nslots)
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_events.data(), ctx->dp_events.p, sizeof(msg_event) * nslots,
                                   hipMemcpyDeviceToHost, s));
    ctx->h_er_off.resize(ntaps);
    ctx->h_er_gain.resize(ntaps);
    if (ntaps) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_er_off.data(), ctx->dp_er_off.p, sizeof(int32_t) * ntaps,
                                   hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_er_gain.data(), ctx->dp_er_gain.p, sizeof(double) * ntaps,
                                   hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    return MSG_OK;
}

static int stage_plan(msg_ctx* ctx, Batch& b) {
    b.hA = b.h0;
    b.flen.assign(b.P, 0);
    for (int p = 0; p < b.P; ++p) {
        const int f = b.presets[p].ir_frag;
        b.flen[p] = (f >= 0 && f < b.n_irs) ? b.ir_lens[f] : 0;
    }
    b.info.resize(b.P);
    b.slot_base.resize(b.P);
    b.tap_base.resize(b.P);
    b.er_dev = !ctx->sw.device_plan && ctx->sw.er_dev;
    return ctx->sw.device_plan ? plan_device(ctx, b) : plan_host(ctx, b);
}

// ---------------------------------------------------------------------------
// tap merge (er_merge.h): per preset, in place in the context's tap arrays
// ---------------------------------------------------------------------------
static int stage_tap_merge(msg_ctx* ctx, Batch& b) {
    b.n_taps_live.assign(b.P, 0);
    b.tap_max.assign(b.P, 0);
    auto merge = [&](int p) {
        if (!(b.presets[p].flags & MSG_F_ER_CLOUD)) return;
        const int nt = std::max(1, b.presets[p].er_taps);
        const int32_t tb = b.tap_base[p];
        b.n_taps_live[p] = er_merge_taps(nt, b.info[p].out_n, ctx->h_er_off.data() + tb,
                                         b.er_dev ? nullptr : ctx->h_er_gain.data() + tb,
                                         b.er_dev ? ctx->h_er_key.data() + tb : nullptr,
                                         b.er_dev ? ctx->h_er_first.data() + tb : nullptr,
                                         b.er_dev ? ctx->h_er_cnt.data() + tb : nullptr, &b.tap_max[p]);
    };
    if (ctx->sw.device_plan) for (int p = 0; p < b.P; ++p) merge(p);
    else HostPool::get().run(b.P, merge);
    return MSG_OK;
}

// ---------------------------------------------------------------------------
// preset records (PresetRt, Fir64Rt, the float64 chain's Ev64 / Chain64)
// ---------------------------------------------------------------------------
// Taps of the space filter h = (delta + ER) * IR of preset p (MS:409-445), 0
// without a FIR: the largest ER offset (planned span or actual) plus the IR
// length, at most out_n (later taps never reach y[:out_n]).
// full8: instead the length of the filter k_fir8's spectrum holds (every
// in-range tap, offset < out_n, and the whole IR), not capped at out_n.
static int64_t h_taps(const Batch& b, int p, bool full8 = false) {
    const msg_preset& pr = b.presets[p];
    const bool er = (pr.flags & MSG_F_ER_CLOUD) != 0;
    const int ic = pr.ir_conv;
    const bool ir = (pr.flags & MSG_F_SPACE_IR) && ic >= 0 && b.ir_lens[ic] > 0;
    if (!er && !ir) return 0;
    const int64_t irl = ir ? std::min<int64_t>(b.ir_lens[ic], 8192) : 1;
    const int64_t span = er ? std::max<int64_t>((int64_t)std::nearbyint(pr.er_max_ms / 1000.0 * (double)pr.base_sr),
                                                b.tap_max[p]) : 0;
    if (full8) return std::min<int64_t>(span, std::max<int64_t>(0, b.info[p].out_n - 1)) + irl;
    return std::max<int64_t>(1, std::min<int64_t>(span + irl, b.info[p].out_n));
}

// The per-preset pure functions of the records (FIR partitioning, stereo
// Bessel taps) in parallel, and the batch's overlap-add decision.
static void pick_fir(msg_ctx* ctx, Batch& b) {
    std::vector<Batch::FirPick>& pick = b.fir.pick;
    pick.resize(b.P);
    HostPool::get().run(b.P, [&](int p) {
        Batch::FirPick& f = pick[p];
        f.M = h_taps(b, p);
        f.N = f.P = f.Q = 0;
        if (f.M > 0) choose_fir(f.M, b.info[p].out_n, f.N, f.P, f.Q, ctx->sw.fir8, h_taps(b, p, true));
        const double w = std::min(std::max(b.presets[p].stereo_width, 0.0), 1.0);
        for (int m = 0; m <= 12; ++m) {                // J_{-m} = (-1)^m J_m: one series per |m|
            const double j = bessel_j(m, w * 0.9);
            f.bess[m + 12] = (float)j;
            f.bess[12 - m] = (float)((m & 1) ? -j : j);
        }
    });
    // The overlap-add inside k_fir8p, decided for the batch as a whole: all of its
    // k_fir8p presets or none, by their grains against their outputs.  A batch
    // with any ola_fir preset runs the fused instantiation for all of its blocks,
    // and that kernel's extra live state costs the plain blocks ~10 % (C3: a few
    // sparse seeds had put every C3 batch on it, isolated FIR 1.88 -> 2.13 ms).
    b.fir.batch_ola = false;
    if (ctx->sw.ola_fir && ctx->sw.fir8p > 0) {
        double grains = 0.0, frames = 0.0;
        for (int p = 0; p < b.P; ++p)
            if (pick[p].M > 0 && pick[p].N == FIR8_N) {
                grains += (double)b.info[p].pool_len;
                frames += (double)b.info[p].out_n;
            }
        b.fir.batch_ola = frames > 0.0 && grains <= ctx->sw.ola_fir_density * frames;
    }
}

// Offsets into the batch's buffers and the generator's sources (MS:333-362).
static int rec_sources(msg_ctx* ctx, Batch& b, int p) {
    const msg_preset& pr = b.presets[p];
    const msg_plan_info& inf = b.info[p];
    PresetRt& r = b.prt[p];
    memset(&r, 0, sizeof(r));
    r.out_n = inf.out_n;
    r.out_off = b.out_offsets[p];
    r.pool_base = b.pool;
    r.y_off = b.ysum;
    r.ev_begin = b.slot_base[p];
    r.n_events = inf.n_events;
    r.er_base = b.tap_base[p];
    r.n_taps = b.n_taps_live[p];          // merged, in-range, offset-sorted taps
    r.tile_begin = b.tiles;
    r.max_n = inf.max_n;
    r.frag_len = b.flen[p];
    r.frag_off = (pr.ir_frag >= 0 && pr.ir_frag < b.n_irs) ? b.ir_off[pr.ir_frag] : 0;
    if (pr.gen_mode == MSG_GEN_IMAGE && pr.image >= 0) {
        if (pr.image >= b.n_images || !b.images) return fail(ctx, MSG_E_ARG, "bad image index");
        r.img_off = b.img_off[pr.image];
        r.img_h = b.img_h[pr.image];
        r.img_w = b.img_w[pr.image];
        if (r.img_h <= 0 || r.img_w <= 0) return fail(ctx, MSG_E_ARG, "empty image");
    }
    return MSG_OK;
}

// ADSR (MS:173-177); A > n raises ValueError in the reference (MS:182).
static int rec_envelope(msg_ctx* ctx, Batch& b, int p) {
    const msg_preset& pr = b.presets[p];
    PresetRt& r = b.prt[p];
    const int64_t n = b.info[p].out_n;
    const double sr = (double)pr.base_sr;
    const int64_t A = std::max<int64_t>(0, (int64_t)std::nearbyint(sr * pr.env_a / 1000.0));
    const int64_t D = std::max<int64_t>(0, (int64_t)std::nearbyint(sr * pr.env_d / 1000.0));
    const int64_t R = std::max<int64_t>(0, (int64_t)std::nearbyint(sr * pr.env_r / 1000.0));
    if (A > n)
        return fail(ctx, MSG_E_VALUE, "could not broadcast input array from shape (" + std::to_string(A) +
                                          ",) into shape (" + std::to_string(n) + ",)");
    r.envA = (int32_t)A; r.envD = (int32_t)std::min<int64_t>(D, INT32_MAX);
    r.envR = (int32_t)std::min<int64_t>(R, INT32_MAX);
    r.envS = (float)std::min(std::max(pr.env_s, 0.0), 1.0);
    r.envC = (float)std::max(1e-6, pr.env_curve);
    const int64_t j = std::min<int64_t>(n, A + D);
    const int64_t s1 = std::max<int64_t>(j, n - R);
    r.envJ = (int32_t)j;
    r.envS1 = (int32_t)s1;
    r.envInvA = A > 0 ? (float)(1.0 / (double)A) : 0.f;
    r.envInvD = j > A ? (float)(1.0 / (double)(j - A)) : 0.f;
    r.envInvR = n - s1 > 1 ? (float)(1.0 / (double)(n - s1 - 1)) : 0.f;
    return MSG_OK;
}

// A one-partition preset whose spectrum comes straight from the taps: H =
// rfft(delta + ER taps) . S_IR (k_fir8_hconv at N = 65536, k_fir4_hconv at
// N = 32768, fir4_fft.h), or S_IR itself for an IR-only preset.
static void place_one_partition(IrBank& bank, int p, const msg_preset& pr, PresetRt& r, int h_fir4) {
    r.h_fir4 = h_fir4;
    const int64_t irs = r.ir_len > 0 ? bank.slot(pr.ir_conv, r.ir_off, r.ir_len, r.fir_N) : -1;
    if (pr.flags & MSG_F_ER_CLOUD) {
        r.irs_off = irs;
        bank.er_list.push_back(p);
    } else {
        r.h_off = irs;                 // relocated past the per-preset spectra (IrBank::relocate)
        bank.ir_only.push_back(p);
    }
}

// Space FIR: partitioning, the engine that builds the spectra, the output
// blocks and the preset's place in hspec / hscratch.
static int rec_space_fir(msg_ctx* ctx, Batch& b, int p) {
    const msg_preset& pr = b.presets[p];
    const msg_plan_info& inf = b.info[p];
    PresetRt& r = b.prt[p];
    Batch::Fir& F = b.fir;
    const bool er = (pr.flags & MSG_F_ER_CLOUD) != 0;
    const int ic = pr.ir_conv;
    const bool ir = (pr.flags & MSG_F_SPACE_IR) && ic >= 0 && b.ir_lens[ic] > 0;   // size<8 check: caller
    r.ir_len = ir ? (int32_t)std::min<int64_t>(b.ir_lens[ic], 8192) : 0;
    r.ir_off = ir ? b.ir_off[ic] : 0;
    r.fir_on = (er || ir) ? 1 : 0;
    r.fir_block_begin = F.fblocks;   // prefix arrays must stay monotone for find_preset
    r.h_block_begin = F.hblocks;
    r.h_fir4 = 0;
    F.h_tile_begin[p] = F.htiles;
    F.fir_begin[p] = r.fir_block_begin;
    F.h_begin[p] = r.h_block_begin;
    if (!r.fir_on) return MSG_OK;
    const int64_t M = F.pick[p].M;
    const int N = F.pick[p].N, Pp = F.pick[p].P, Q = F.pick[p].Q;
    if (N != FIR8_N) {                     // runtime plan for k_fir_h (k_fir8 has its own engine)
        std::string why;
        const int fp = real_plan(ctx->fir_plans, N, why);
        if (fp < 0) return fail(ctx, MSG_E_DEVICE, "FIR plan: " + why);
        F.fir_plan_of[p] = fp;
        F.lds = std::max(F.lds, ctx->fir_plans.host[fp].lds_bytes);
    }
    r.fir_N = N; r.fir_P = Pp; r.fir_Q = Q; r.fir_B = N - Pp + 1;
    r.h_off = F.hsum;
    r.h_len = (int32_t)M;
    if (N == FIR8_N) {
        place_one_partition(F.ir8, p, pr, r, 2);
    } else if (N == 2 * 16384 && ctx->sw.fir4 && ctx->sw.fir4c && Q == 1 && M <= N) {
        place_one_partition(F.ir4, p, pr, r, 3);
    } else {                               // h in the time domain (k_h_build), cut into partitions
        r.hs_off = F.hs_sum;
        F.hs_sum += (M + 3) & ~int64_t(3);    // 16-byte aligned h regions
        F.htiles += (int32_t)((M + H_BUILD_TILE - 1) / H_BUILD_TILE);
        if (N == 2 * 16384 && ctx->sw.fir4) {   // k_fir4_hpart
            r.h_fir4 = 1;
            for (int q = 0; q < Q; ++q) F.hpart_jobs.push_back(make_int2(p, q));
        }
    }
    const int32_t nblk = (int32_t)((inf.out_n + r.fir_B - 1) / r.fir_B);
    // the overlap-add in k_fir8p's segment loads: each segment sums its grains
    // again (N / B ~ 1.6 times per frame), worth it while the grains are sparse
    if (N == FIR8_N && F.batch_ola) {
        r.ola_fir = 1;
        F.n_ola++;
        F.ola_nmax = std::max<int64_t>(F.ola_nmax, inf.out_n);
    }
    std::vector<int2>& fj = F.jobs_by[N == FIR8_N ? 5 : __builtin_ctz(N) - 11];
    for (int32_t k = 0; k < nblk; ++k) fj.push_back(make_int2(p, k));
    F.fblocks += nblk;
    F.hblocks += Q;
    if (!r.h_fir4) F.hblocks_gen += Q;
    // each preset's spectra start on a 128-byte boundary (N / 2 + 1 float2 per
    // partition is odd: unpadded, every other preset's He straddled one more
    // cache line per wave-wide load)
    // (N = 65536: one spectrum of FIR8_HSTRIDE float2, Ho 128-byte aligned inside it)
    static_assert(((FIR8_N / 2 + 1 + 15) & ~15) == FIR8_HSTRIDE, "fir8 spectrum stride");
    if (!((N == FIR8_N || r.h_fir4 == 3) && r.ir_len > 0 && !er))   // an IR-only preset's H is its bank's
        F.hsum += ((int64_t)Q * (N / 2 + 1) + 15) & ~int64_t(15);
    return MSG_OK;
}

// Stereo (MS:423-436), saturation and the stereo tiles.
static int rec_stereo(msg_ctx* ctx, Batch& b, int p) {
    const msg_preset& pr = b.presets[p];
    const msg_plan_info& inf = b.info[p];
    PresetRt& r = b.prt[p];
    const double sr = (double)pr.base_sr;
    const double w = std::min(std::max(pr.stereo_width, 0.0), 1.0);
    const bool stereo = (pr.flags & MSG_F_STEREO) && inf.out_n >= 64;
    r.stereo_fir = stereo ? 1 : 0;
    if (stereo && (inf.out_n % 2)) {      // full-length rotation through Bluestein (kernels_stereo_odd.h)
        const int64_t M = stereo_odd_len(inf.out_n, ctx->sw.so_row, ctx->sw.so_col);
        if (M < 0)
            return fail(ctx, MSG_E_UNSUPPORTED, "stereo diffusion of an odd output beyond the 2^34-point transform");
        r.stereo_fir = 2;
        r.r2_off = b.r2_sum;
        b.r2_sum += (inf.out_n + 3) & ~int64_t(3);
        b.so_M = std::max(b.so_M, M);
        b.odd_presets.push_back(p);
    }
    r.dl = (int32_t)std::nearbyint((1 + 7 * w) * 0.0005 * sr);
    r.dr = (int32_t)std::nearbyint((1 + 9 * w) * 0.0007 * sr);
    std::memcpy(r.bess, b.fir.pick[p].bess, sizeof(r.bess));
    r.drive = (float)pr.sat_drive;
    r.peak = (float)pr.peak;
    b.st_begin[p] = b.stiles;
    b.st_count[p] = (int32_t)((inf.out_n + ST_TILE - 1) / ST_TILE);
    b.stiles += b.st_count[p];
    return MSG_OK;
}

// The float64 FIR's shape (kernels_fir64.h), for every FIR preset.
static void rec_fir64_shape(Batch& b, int p) {
    Batch::Fir64& S = b.f64;
    Fir64Rt& f = S.rt[p];
    const bool fir_on = b.prt[p].fir_on != 0;
    f.h_len = fir_on ? (int32_t)b.fir.pick[p].M : 0;
    f.q = (f.h_len + FIR64_P - 1) / FIR64_P;
    f.blocks = (int32_t)((b.info[p].out_n + FIR64_B - 1) / FIR64_B);
    f.st_tiles = b.st_count[p];
    if (fir_on) {
        S.cand++;
        S.hmax = std::max<int64_t>(S.hmax, f.h_len);
        S.qmax = std::max(S.qmax, f.q);
        S.bmax = std::max(S.bmax, f.blocks);
        S.stmax = std::max(S.stmax, f.st_tiles);
    }
}

// The preset's chain: the float32 one (its events' records come in the next
// stage), or the float64 chain's Ev64 / Chain64 records.
static int rec_events64(msg_ctx* ctx, Batch& b, int p) {
    const msg_preset& pr = b.presets[p];
    const msg_plan_info& inf = b.info[p];
    const PresetRt& r = b.prt[p];
    Batch::G64& G = b.g64;
    bool precise = is_precise(pr);
    if (!precise) {
        // grains beyond the LDS-resident float32 spectral kernels run the float64
        // chain in global memory (micro_ms up to 80 ms at 30 MHz: 2.4 M samples)
        int last_n = -1;
        for (int k = 0; k < inf.n_events && !precise; ++k) {
            const msg_event& e = ctx->h_events[b.slot_base[p] + k];
            if (!spec_ops(pr, e) || e.n == last_n) continue;   // each spectral grain length once
            last_n = e.n;
            if (b.use_ct && spectral_ct_plan(e.n) >= 0) continue;
            std::string why;
            const int pi = real_plan(ctx->grain_plans, e.n, why);
            if (pi < 0) return fail(ctx, MSG_E_DEVICE, "grain plan: " + why);
            const RealPlan& gp = ctx->grain_plans.host[pi];
            if (gp.lds_bytes > LDS_MAX || gp.c.size > SPEC_M_BIG) precise = true;
        }
    }
    if (!(precise && inf.n_events > 0)) {
        b.f32.presets.push_back(p);
        return MSG_OK;
    }
    const bool chained = (pr.flags & (MSG_F_EVENT_FEEDBACK | MSG_F_IMPRINT)) != 0;
    bool chain_global = false;
    if (chained) {
        Chain64 c;
        memset(&c, 0, sizeof(c));
        c.preset = p;
        c.ev_begin = (int32_t)G.ev.size();
        c.n_events = inf.n_events;
        c.prev_off = G.state_sum;
        c.mem_off = G.state_sum + ((inf.max_n + 1) & ~1);
        G.state_sum += ((inf.max_n + 1) & ~1) + ((inf.max_n / 2 + 2) & ~1);
        G.chains.push_back(c);
    }
    for (int k = 0; k < inf.n_events; ++k) {
        const int ei = b.slot_base[p] + k;
        const msg_event& e = ctx->h_events[ei];
        memset(&b.ert[ei], 0, sizeof(EventRt));
        Ev64 v;
        memset(&v, 0, sizeof(v));
        std::string why;
        v.plan = real64_plan(ctx->plans64, e.n, why);
        if (v.plan < 0) return fail(ctx, MSG_E_DEVICE, "float64 grain plan: " + why);
        const Real64Plan& gp = ctx->plans64.host[v.plan];
        if (gp.cap > G64_SLOTS) {        // beyond the LDS engine: a global-memory slot
            G.big_cap = std::max<int64_t>(G.big_cap, gp.cap);
            G.glb.push_back((int32_t)G.ev.size());
            chain_global = true;
        } else {
            G.cap = std::max(G.cap, gp.cap);
            G.lds.push_back((int32_t)G.ev.size());
        }
        v.ops = g64_ops(pr, e);
        if (b.stop_cep && (v.ops & G64_CEP))   // debug: the grain as cepstral_warp receives it
            v.ops &= G64_LOWPASS | G64_WARP | G64_CHAIN;
        v.n = e.n;
        v.n0 = msgplan::grain_len(e.gen_sr, pr.micro_ms, 16);
        v.gen_sr = e.gen_sr;
        v.preset = p;
        v.index = e.index;
        v.ei = ei;
        v.off64 = G.sum;
        v.grain_off = r.pool_base + e.pool_off;
        ctx->h_grain_off[ei] = v.grain_off;          // float64-chain events keep their own slots
        v.cutoff_gen = e.cutoff_out * e.ufac;
        v.stretch = e.stretch;
        if (v.ops & G64_CEP) { v.save_off = G.save_sum; G.save_sum += e.n / 2 + 1; }
        if (pr.gen_mode == MSG_GEN_WAVELET) {
            // morlet_atom is max(16, round(..)) long, the grain max(128, ..): shorter
            // atoms do not broadcast into the grain (MS:319, 166, 329)
            const int na = msgplan::grain_len(e.gen_sr, pr.micro_ms, 16);
            if (na < e.n)
                return fail(ctx, MSG_E_VALUE, "operands could not be broadcast together with shapes (" +
                                                  std::to_string(e.n) + ",) (" + std::to_string(na) +
                                                  ",) (" + std::to_string(e.n) + ",)");
        }
        if (normal_driven(pr.gen_mode)) {
            G.gen_list.push_back(ei);
            G.gen_off.push_back(G.sum);
        }
        G.sum += (e.n + 1) & ~1;
        G.last[p] = (int32_t)G.ev.size();
        G.ev.push_back(v);
    }
    if (chained && chain_global) {                  // the chain walks big grains too
        G.chains_glb.push_back(G.chains.back());
        G.chains.pop_back();
    }
    return MSG_OK;
}

static int stage_preset_records(msg_ctx* ctx, Batch& b) {
    const int P = b.P;
    b.prt.resize(P);
    // host EventRt records: a grow-only buffer reused across batches (a C5 sub-batch
    // holds 512 k events; a fresh zero-filled vector cost ~8 ms of page faults and
    // memset per batch).  Every slot an event list references is written by the
    // record stages.
    if ((size_t)b.nslots > ctx->h_ert_cap) {
        ctx->h_ert.reset(new EventRt[(size_t)b.nslots + b.nslots / 4]);
        ctx->h_ert_cap = (size_t)b.nslots + b.nslots / 4;
    }
    b.ert = ctx->h_ert.get();
    if ((size_t)b.nslots > ctx->h_grain_off.size()) ctx->h_grain_off.resize((size_t)b.nslots + b.nslots / 4);
    // slots a preset reserves beyond its events are never written: zero them
    // so the whole uploaded range is defined
    for (int p = 0; p < P; ++p)
        if (b.info[p].n_slots > b.info[p].n_events) {
            memset(b.ert + b.slot_base[p] + b.info[p].n_events, 0,
                   sizeof(EventRt) * (size_t)(b.info[p].n_slots - b.info[p].n_events));
            std::fill_n(ctx->h_grain_off.begin() + b.slot_base[p] + b.info[p].n_events,
                        b.info[p].n_slots - b.info[p].n_events, int64_t(0));
        }
    b.f64.rt.resize(P);
    b.st_count.resize(P);
    b.tile_begin.resize(P);
    b.st_begin.resize(P);
    b.fir.fir_begin.resize(P);
    b.fir.h_begin.resize(P);
    b.fir.fir_plan_of.assign(P, 0);
    b.fir.h_tile_begin.assign(P, 0);
    b.g64.last.assign(P, -1);
    b.ir_off.assign(std::max(b.n_irs, 1), 0);
    for (int i = 0; i < b.n_irs; ++i) {
        b.ir_off[i] = (int64_t)b.irbank.size();
        b.irbank.insert(b.irbank.end(), b.irs[i], b.irs[i] + b.ir_lens[i]);
    }
    b.img_off.assign(std::max(b.n_images, 1), 0);
    for (int i = 0; i < b.n_images; ++i) {
        b.img_off[i] = (int64_t)b.imgbank.size();
        b.imgbank.insert(b.imgbank.end(), b.images[i], b.images[i] + (int64_t)b.img_h[i] * b.img_w[i]);
    }
    const char* ct_env = getenv("MSGPU_SPEC_CT");         // "0": runtime-plan kernels only (tests)
    b.use_ct = !(ct_env && ct_env[0] == '0');
    const char* s3_env = getenv("MSGPU_SPEC3");          // "0": no band-pruned kernel (A/B, tests)
    b.use_s3 = b.use_ct && !(s3_env && s3_env[0] == '0');
    // MSGPU_G64_STOP=cep (tests only): float64-chain grains stop before the cepstral
    // warp (MS:696-697), so meta grain_last is that stage's input (stage-pin tests)
    const char* stop_env = getenv("MSGPU_G64_STOP");
    b.stop_cep = stop_env && std::strcmp(stop_env, "cep") == 0;
    pick_fir(ctx, b);
    // one pass over the presets: the prefix sums depend on their order
    for (int p = 0; p < P; ++p) {
        if (int rc = rec_sources(ctx, b, p)) return rc;
        if (int rc = rec_envelope(ctx, b, p)) return rc;
        if (int rc = rec_space_fir(ctx, b, p)) return rc;
        if (int rc = rec_stereo(ctx, b, p)) return rc;
        rec_fir64_shape(b, p);
        if (!b.prt[p].ola_fir) b.tiles += (int32_t)((b.info[p].out_n + OLA_TILE - 1) / OLA_TILE);
        b.pool += (b.info[p].pool_len + 3) & ~int64_t(3);   // 16-byte aligned grain regions (float4 loads)
        b.ysum += (b.info[p].out_n + 3) & ~int64_t(3);      // keep every mono region 16-byte aligned
        if (int rc = rec_events64(ctx, b, p)) return rc;
    }
    return MSG_OK;
}

// ---------------------------------------------------------------------------
// float32-chain event records (EventRt), presets in parallel on the host
// pool; the per-kernel event lists are concatenated in preset order.  Events
// that need a runtime FFT plan (no compile-time plan for their length) are
// planned afterwards on this thread (the plan cache is not shared).
// ---------------------------------------------------------------------------
static int stage_event_records(msg_ctx* ctx, Batch& b) {
    using F32Lists = Batch::F32::Lists;
    Batch::F32& F = b.f32;
    // Generator sharing (gen_share.h): the first event of the batch with a generator
    // key is its owner, and the only one on k_gen_normal's list; every event reads
    // its owner's micro slot.  One pass on this thread, before the records: the
    // first event in list order owns.  The tilt step's micro_last (the one write
    // into a micro slot after the generator) goes to a slot of the preset's own
    // behind the pool, for the preset's last event only, so a shared slot is never
    // written.
    if ((size_t)b.nslots > ctx->h_gen_owner.size()) ctx->h_gen_owner.resize((size_t)b.nslots + b.nslots / 4);
    int32_t* const owner = ctx->h_gen_owner.data();
    F.micro_last.assign(b.P, -1);
    {
        std::vector<int32_t> nev(b.P);
        for (int p = 0; p < b.P; ++p) nev[p] = b.info[p].n_events;
        F.n_owners = genshare::assign(b.presets, F.presets.data(), (int)F.presets.size(), ctx->h_events.data(),
                                      b.slot_base.data(), nev.data(), b.nslots, ctx->sw.gen_share, owner,
                                      ctx->gen_scratch);
        for (int p : F.presets) {
            const int ne = nev[p];
            F.n_events += ne;
            if (ne <= 0) continue;
            const int last = b.slot_base[p] + ne - 1;
            const int gm = b.presets[p].gen_mode;
            if (gm == MSG_GEN_NOISE_BURST || gm == MSG_GEN_FALLBACK || gm == MSG_GEN_SKEWED) {   // spec_ops' tilt modes
                F.micro_last[p] = b.pool + F.mlast_sum;
                F.mlast_sum += (ctx->h_events[last].n + 3) & ~int64_t(3);
            } else {
                const msg_event& oe = ctx->h_events[owner[last]];
                F.micro_last[p] = b.prt[oe.preset].pool_base + oe.pool_off;
            }
        }
    }
    if ((size_t)b.nslots > ctx->h_spec_owner.size()) {
        ctx->h_spec_owner.resize((size_t)b.nslots + b.nslots / 4);
        ctx->h_spec_route.resize((size_t)b.nslots + b.nslots / 4);
    }
    int8_t* const route = ctx->h_spec_route.data();
    HostPool::get().run((int)F.presets.size(), [&](int i) {
        const int p = F.presets[i];
        const msg_preset& pr = b.presets[p];
        const PresetRt& r = b.prt[p];
        const specshare::PresetConsts pc = specshare::preset_consts(pr);
        const int ne = b.info[p].n_events;
        for (int k = 0; k < ne; ++k) {
            const int ei = b.slot_base[p] + k;
            const msg_event& e = ctx->h_events[ei];
            EventRt& x = b.ert[ei];
            memset(&x, 0, sizeof(x));
            specshare::key_fields(pr, e, pc, x);
            const msg_event& oe = ctx->h_events[owner[ei]];
            x.micro_off = b.prt[oe.preset].pool_base + oe.pool_off;
            x.mlast_off = (k == ne - 1 && (x.ops & (SPEC_TILT_NOISE | SPEC_TILT_SKEW))) ? F.micro_last[p] : -1;
            // the kernel the event alone would run: part of its spectral key, so sharing
            // never changes a grain's kernel
            const int ctp = (x.ops && b.use_ct) ? spectral_ct_plan(e.n) : -1;
            // k_spec3 reads the micro slot and writes the grain slot in 8-byte pairs: both offsets even
            if (b.use_s3 && x.ops &&
                spec3_eligible(e.n, x.ops, x.gen_sr, x.cutoff_gen, x.roll, x.stretch,
                               (r.pool_base + e.pool_off) | x.micro_off,
                               &x.s3_kb, &x.s3_kz, &x.s3_ky, &x.s3_inv_f, &x.s3_pad))
                route[ei] = specshare::ROUTE_SPEC3;
            else if (ctp >= 0)
                route[ei] = (int8_t)(specshare::ROUTE_CT + ctp);
            else
                route[ei] = x.ops ? specshare::ROUTE_RUNTIME : specshare::ROUTE_COPY;
        }
    });
    // Spectral sharing (gen_share.h): the first event in list order with a spectral key
    // runs the chain, and the overlap-add reads every event's grain from its owner's slot
    // (grain_off).  One pass on this thread, in list order, as for the generator.
    int32_t* const sown = ctx->h_spec_owner.data();
    int64_t* const goff = ctx->h_grain_off.data();
    {
        std::vector<int32_t> nev(b.P);
        for (int p = 0; p < b.P; ++p) nev[p] = b.info[p].n_events;
        F.n_spec_runs = specshare::assign(b.ert, route, owner, F.presets.data(), (int)F.presets.size(),
                                          b.slot_base.data(), nev.data(), b.nslots, ctx->sw.spec_share, sown,
                                          ctx->spec_scratch);
    }
    // each preset's grain offsets and lists (owners only), presets in parallel again
    std::vector<F32Lists>& f32l = F.per_preset;
    f32l.resize(F.presets.size());
    HostPool::get().run((int)F.presets.size(), [&](int i) {
        const int p = F.presets[i];
        F32Lists& L = f32l[i];
        const int ne = b.info[p].n_events;
        for (int k = 0; k < ne; ++k) {
            const int ei = b.slot_base[p] + k;
            const msg_event& se = ctx->h_events[sown[ei]];
            goff[ei] = b.prt[se.preset].pool_base + se.pool_off;
            if (owner[ei] == ei) L.gen.push_back(ei);
            if (sown[ei] != ei) continue;
            const int8_t rt = route[ei];
            if (rt == specshare::ROUTE_SPEC3) L.s3.push_back(ei);
            else if (rt >= specshare::ROUTE_CT) L.ct[rt - specshare::ROUTE_CT].push_back(ei);
            else if (rt == specshare::ROUTE_RUNTIME) L.pending.push_back(ei);
            else L.small.push_back(ei);
        }
    });
    for (F32Lists& L : f32l) {
        F.gen_list.insert(F.gen_list.end(), L.gen.begin(), L.gen.end());
        F.spec3.insert(F.spec3.end(), L.s3.begin(), L.s3.end());
        for (int c = 0; c < SPEC_CT_PLANS; ++c) F.ct[c].insert(F.ct[c].end(), L.ct[c].begin(), L.ct[c].end());
        F.spec_small.insert(F.spec_small.end(), L.small.begin(), L.small.end());
        F.n_copy += (int64_t)L.small.size();
        for (int ei : L.pending) {   // no compile-time plan for the length: a runtime plan, planned on this thread
            EventRt& x = b.ert[ei];
            std::string why;
            const int pi = real_plan(ctx->grain_plans, x.n, why);
            if (pi < 0) return fail(ctx, MSG_E_DEVICE, "grain plan: " + why);
            x.plan = pi;
            const RealPlan& gp = ctx->grain_plans.host[pi];
            if (gp.lds_bytes <= SPEC_SMALL_BYTES && gp.c.size <= SPEC_M_SMALL) {
                F.spec_small.push_back(ei);
                F.small_lds = std::max(F.small_lds, gp.lds_bytes);
            } else if (gp.lds_bytes <= LDS_MAX && gp.c.size <= SPEC_M_BIG) {
                F.spec_big.push_back(ei);
                F.big_lds = std::max(F.big_lds, gp.lds_bytes);
            } else {
                return fail(ctx, MSG_E_UNSUPPORTED, "grain of " + std::to_string(x.n) +
                            " samples exceeds the LDS-resident FFT (even n <= ~39900)");
            }
        }
    }
    return MSG_OK;
}

// ---------------------------------------------------------------------------
// plans, lists, buffers
// ---------------------------------------------------------------------------
// The fused overlap-add's first event per k_fir8p block: the events of a
// preset are sorted by start, so one moving index per preset finds, block by
// block, the first event starting after the segment's start - max_n.
static void fir_first_events(msg_ctx* ctx, Batch& b) {
    const std::vector<int2>& fj = b.fir.jobs_by[5];
    b.fir.lo.resize(fj.size());
    int cur_p = -1, k = 0;
    for (size_t j = 0; j < fj.size(); ++j) {
        const int p = fj[j].x;
        if (p != cur_p) { cur_p = p; k = 0; }
        const PresetRt& r = b.prt[p];
        const int64_t lim = (int64_t)fj[j].y * r.fir_B - (r.fir_P - 1) - (int64_t)r.max_n;
        const msg_event* ev = ctx->h_events.data() + r.ev_begin;
        if (fj[j].y == 0) k = 0;
        while (k < r.n_events && (int64_t)ev[k].start <= lim) ++k;
        b.fir.lo[j] = k;
    }
}

// The FFT plans on the device (before any launch), the concatenated lists the
// kernels read, and the launch scalars that follow from them.
static int stage_lists(msg_ctx* ctx, Batch& b) {
    Batch::Fir& F = b.fir;
    Batch::G64& G = b.g64;
    Batch::Fir64& S = b.f64;
    if (ctx->sw.fir64 > 0 && S.cand > 0) {                  // the float64 FIR's transform (kernels_fir64.h)
        std::string why;
        S.plan = real64_plan(ctx->plans64, FIR64_N, why);
        if (S.plan < 0) return fail(ctx, MSG_E_DEVICE, "float64 FIR plan: " + why);
    }
    HIPCHK(ctx, sync_plans(ctx->grain_plans, b.s));
    HIPCHK(ctx, sync_plans(ctx->fir_plans, b.s));
    HIPCHK(ctx, sync_plans(ctx->plans64, b.s));
    G.list = G.lds;
    G.list.insert(G.list.end(), G.glb.begin(), G.glb.end());
    G.n_lds_chains = G.chains.size();
    G.chains.insert(G.chains.end(), G.chains_glb.begin(), G.chains_glb.end());
    // global slots: persistent workgroups, at most ~8 GB of grain + scratch buffers
    if (!G.glb.empty() || !G.chains_glb.empty()) {
        int64_t cap = G.big_cap;
        for (const Chain64& c : G.chains_glb)
            for (int q = 0; q < c.n_events; ++q)
                cap = std::max<int64_t>(cap, ctx->plans64.host[G.ev[c.ev_begin + q].plan].cap);
        G.gg.slot_cap = (cap + 1) & ~int64_t(1);
        G.gg.mask_words = G.gg.slot_cap / 32 + 2;
        const int64_t per_slot = 2 * G.gg.slot_cap * 16 + G.gg.mask_words * 4;
        const int64_t lim = std::max<int64_t>(1, std::min<int64_t>(1024, (int64_t(8) << 30) / per_slot));
        G.g_grid = (unsigned)std::min<int64_t>((int64_t)G.glb.size(), lim);
        G.c_grid = (unsigned)std::min<int64_t>((int64_t)G.chains_glb.size(), lim);
    }
    for (int i = 0; i < 6; ++i) {
        F.job_off[i] = (int32_t)F.jobs.size();
        F.jobs.insert(F.jobs.end(), F.jobs_by[i].begin(), F.jobs_by[i].end());
    }
    F.job_off[6] = (int32_t)F.jobs.size();
    if (F.n_ola > 0) fir_first_events(ctx, b);
    // the IR spectra of the k_fir8 presets follow the per-preset spectra in hspec,
    // then the k_fir4_hconv presets' IR spectra
    F.ir8.relocate(b.prt, F.hsum);
    F.ir4.relocate(b.prt, F.hsum + F.ir8.sum);
    for (int p = 0; p < b.P; ++p) b.tile_begin[p] = b.prt[p].tile_begin;
    for (int i = 0; i < SPEC_CT_PLANS; ++i) {
        b.f32.ct_off[i] = (int32_t)b.f32.ct_list.size();
        b.f32.ct_list.insert(b.f32.ct_list.end(), b.f32.ct[i].begin(), b.f32.ct[i].end());
    }
    b.f32.ct_off[SPEC_CT_PLANS] = (int32_t)b.f32.ct_list.size();
    b.n_odd = (int32_t)b.odd_presets.size();
    // the float64 FIR chain: slots for up to FIR64_CAP flagged presets of the batch
    S.on = ctx->sw.fir64 > 0 && S.cand > 0;
    S.hstride = (S.hmax + 3) & ~int64_t(3);
    S.hsstride = (int64_t)S.qmax * FIR64_K;
    // slots per window: every flagged preset is served, FIR64_WINDOW_BYTES of h and H_q at a time
    const int64_t slot_bytes = S.hstride * (int64_t)sizeof(float) + S.hsstride * (int64_t)sizeof(double2);
    S.cap = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(S.cand, ctx->sw.fir64_cap),
                                                        FIR64_WINDOW_BYTES / std::max<int64_t>(1, slot_bytes)));
    // filter spectra before the generator (MSGPU_H_EARLY)
    int64_t fir_nmax = 0;
    for (int p = 0; p < b.P; ++p)
        if (b.prt[p].fir_on) fir_nmax = std::max<int64_t>(fir_nmax, b.prt[p].out_n);
    F.h_early = F.hblocks > 0 && (ctx->sw.h_early == 1 || (ctx->sw.h_early == 2 && fir_nmax >= ((int64_t)1 << 22)));
    return MSG_OK;
}

// Every device buffer of the batch at its size (DevBuf::ensure: grow-only).
static int stage_buffers(msg_ctx* ctx, Batch& b) {
    const Batch::Fir& F = b.fir;
    Batch::G64& G = b.g64;
    const Batch::Fir64& S = b.f64;
    if (!G.glb.empty() || !G.chains_glb.empty()) {
        const int64_t slots = std::max<int64_t>(std::max(G.g_grid, G.c_grid), 1);
        HIPCHK(ctx, ctx->g64A.ensure(slots * G.gg.slot_cap));
        HIPCHK(ctx, ctx->g64B.ensure(slots * G.gg.slot_cap));
        HIPCHK(ctx, ctx->g64mask.ensure(slots * G.gg.mask_words));
        G.gg.A = ctx->g64A.p;
        G.gg.B = ctx->g64B.p;
        G.gg.mask = ctx->g64mask.p;
    }
    HIPCHK(ctx, ctx->micro64.ensure(G.sum));
    HIPCHK(ctx, ctx->grain64.ensure(G.sum));
    HIPCHK(ctx, ctx->save64.ensure(G.save_sum));
    HIPCHK(ctx, ctx->state64.ensure(G.state_sum));
    HIPCHK(ctx, ctx->so_r2.ensure(b.r2_sum));
    HIPCHK(ctx, ctx->so_A.ensure(b.so_M));
    HIPCHK(ctx, ctx->micro.ensure(b.pool + b.f32.mlast_sum));   // the pool, then the presets' micro_last slots
    HIPCHK(ctx, ctx->grain.ensure(b.pool));
    HIPCHK(ctx, ctx->mono_a.ensure(b.ysum));
    HIPCHK(ctx, ctx->mono_y.ensure(b.ysum));
    HIPCHK(ctx, ctx->hspec.ensure(F.hsum + F.ir8.sum + F.ir4.sum));
    HIPCHK(ctx, ctx->hscratch.ensure(F.hs_sum));
    if (S.on) {
        HIPCHK(ctx, ctx->f64_stats.ensure(2 * (size_t)b.P));
        HIPCHK(ctx, ctx->f64_flag.ensure(b.P));
        HIPCHK(ctx, ctx->st_part.ensure(2 * (size_t)b.stiles));
        HIPCHK(ctx, ctx->f64_slot_preset.ensure(S.cand));
        HIPCHK(ctx, ctx->f64_nslots.ensure(1));
        HIPCHK(ctx, ctx->f64_h.ensure((size_t)(S.cap * S.hstride)));
        HIPCHK(ctx, ctx->f64_hs.ensure((size_t)(S.cap * S.hsstride)));
    }
    if (b.er_dev) {   // k_er_gains' outputs (host batch path)
        HIPCHK(ctx, ctx->er_gain_d.ensure((size_t)std::max<int64_t>(1, b.ntaps)));
        HIPCHK(ctx, ctx->er_tap_d.ensure((size_t)std::max<int64_t>(1, b.ntaps)));
    }
    if (ctx->maxbits_zero.size() < (size_t)b.P) ctx->maxbits_zero.assign((size_t)b.P, 0u);
    return MSG_OK;
}

// ---------------------------------------------------------------------------
// upload: the batch's one staging.add sequence and its flush.  Nothing between
// the first add and the flush can fail, and every source is owned by the
// caller's arguments, the Batch or the context, so no return path leaves an
// item queued in ctx->staging.  The order of the adds is the arena's layout.
// ---------------------------------------------------------------------------
static int stage_upload(msg_ctx* ctx, Batch& b) {
    Staging& st = ctx->staging;
    const int P = b.P;
    auto add_vec = [&](auto& slice, const auto& v) { st.add(&slice.p, v.data(), sizeof(v[0]) * v.size()); };
    st.add(&ctx->presets.p, b.presets, sizeof(msg_preset) * P);
    st.add(&ctx->events.p, ctx->h_events.data(), sizeof(msg_event) * b.nslots);
    st.add(&ctx->er_off.p, ctx->h_er_off.data(), sizeof(int32_t) * b.ntaps);
    if (!b.er_dev) {
        st.add(&ctx->er_gain.p, ctx->h_er_gain.data(), sizeof(double) * b.ntaps);
    } else {
        st.add(&ctx->er_key.p, ctx->h_er_key.data(), sizeof(int32_t) * b.ntaps);
        st.add(&ctx->er_first.p, ctx->h_er_first.data(), sizeof(int32_t) * b.ntaps);
        st.add(&ctx->er_cnt.p, ctx->h_er_cnt.data(), sizeof(int32_t) * b.ntaps);
    }
    st.add(&ctx->ert.p, b.ert, sizeof(EventRt) * b.nslots);
    st.add(&ctx->grain_off.p, ctx->h_grain_off.data(), sizeof(int64_t) * b.nslots);
    add_vec(ctx->prt, b.prt);
    add_vec(ctx->gen_list, b.f32.gen_list);
    add_vec(ctx->spec_small, b.f32.spec_small);
    add_vec(ctx->spec_big, b.f32.spec_big);
    add_vec(ctx->spec3_list, b.f32.spec3);
    add_vec(ctx->spec_ct_list, b.f32.ct_list);
    add_vec(ctx->tile_begin, b.tile_begin);
    add_vec(ctx->fir_begin, b.fir.fir_begin);
    add_vec(ctx->fir_jobs, b.fir.jobs);
    add_vec(ctx->fir_lo, b.fir.lo);
    add_vec(ctx->h_begin, b.fir.h_begin);
    add_vec(ctx->st_begin, b.st_begin);
    add_vec(ctx->fir_plan_of, b.fir.fir_plan_of);
    add_vec(ctx->irbank, b.irbank);
    add_vec(ctx->h_tile_begin, b.fir.h_tile_begin);
    add_vec(ctx->fir8_list, b.fir.ir8.er_list);
    add_vec(ctx->ir8_jobs, b.fir.ir8.jobs);
    add_vec(ctx->fir4c_list, b.fir.ir4.er_list);
    add_vec(ctx->ir4_jobs, b.fir.ir4.jobs);
    add_vec(ctx->hpart_jobs, b.fir.hpart_jobs);
    st.add(&ctx->maxbits.p, ctx->maxbits_zero.data(), sizeof(unsigned) * P);   // zeros in the one upload, no fill launch
    if (b.f64.on) add_vec(ctx->f64rt, b.f64.rt);
    add_vec(ctx->st_count, b.st_count);
    add_vec(ctx->odd_list, b.odd_presets);
    st.add(&ctx->odd_cnt.p, &b.n_odd, sizeof(int32_t));
    add_vec(ctx->ev64, b.g64.ev);
    add_vec(ctx->g64_list, b.g64.list);
    add_vec(ctx->gen64_list, b.g64.gen_list);
    add_vec(ctx->gen64_off, b.g64.gen_off);
    add_vec(ctx->chains, b.g64.chains);
    add_vec(ctx->imgbank, b.imgbank);
    b.h2 = Batch::hclock::now();
    HIPCHK(ctx, st.flush(b.s));
    return MSG_OK;
}

// ---------------------------------------------------------------------------
// enqueue: one function per stage mark
// ---------------------------------------------------------------------------
// The merged ER gains the filter kernels read (host batch path: k_er_gains'
// output; it runs first in enqueue_h_spectra, before every filter kernel that
// reads them -- the float64 FIR's k_h64 comes later still -- so it does not
// hold up the generator).
static const double* er_gains(const msg_ctx* ctx, const Batch& b) {
    return b.er_dev ? ctx->er_gain_d.p : ctx->er_gain.p;
}

// The filter spectra depend on the presets' taps and IRs only, not on the
// audio: launched before the generator (h_early), they run while
// the GPU holds the other streams' earlier stages, instead of queueing
// behind a persistent k_fir8p of another stream that holds every CU
// (C5's fir_h window had been ~100x its isolated time).
static int enqueue_h_spectra(msg_ctx* ctx, Batch& b) {
    const Batch::Fir& F = b.fir;
    hipStream_t s = b.s;
    const double* erg = er_gains(ctx, b);
    if (b.er_dev && b.ntaps > 0) {
        hipLaunchKernelGGL(k_er_gains, dim3((unsigned)b.P), dim3(ER_T), 0, s, ctx->presets.p, ctx->prt.p, b.P,
                           ctx->er_key.p, ctx->er_first.p, ctx->er_cnt.p, ctx->er_tap_d.p, ctx->er_gain_d.p);
        HIPCHK(ctx, hipGetLastError());
    }
    if (F.htiles > 0)
        HIPCHK(ctx, launch_h_build((unsigned)F.htiles, s, ctx->prt.p, ctx->h_tile_begin.p, b.P, ctx->er_off.p,
                                   erg, ctx->irbank.p, ctx->hscratch.p));
    if (!F.ir8.jobs.empty())
        HIPCHK(ctx, launch_fir8_spec64((unsigned)(F.ir8.jobs.size() / 4), s, ctx->ir8_jobs.p, ctx->d_fir4tab.p,
                                       ctx->irbank.p, ctx->hspec.p));
    if (!F.hpart_jobs.empty())
        HIPCHK(ctx, launch_fir4_hpart(16384, (unsigned)F.hpart_jobs.size(), s, ctx->prt.p, ctx->hpart_jobs.p,
                                      ctx->d_fir4tab.p, ctx->hscratch.p, ctx->hspec.p));
    if (!F.ir8.er_list.empty())
        HIPCHK(ctx, launch_fir8_hconv((unsigned)F.ir8.er_list.size(), s, ctx->prt.p, ctx->fir8_list.p, ctx->d_fir4tab.p,
                                      ctx->er_off.p, erg, ctx->hspec.p));
    if (!F.ir4.jobs.empty())
        HIPCHK(ctx, launch_fir4_irspec((unsigned)(F.ir4.jobs.size() / 4), s, ctx->ir4_jobs.p, ctx->d_fir4tab.p,
                                       ctx->irbank.p, ctx->hspec.p));
    if (!F.ir4.er_list.empty())
        HIPCHK(ctx, launch_fir4_hconv((unsigned)F.ir4.er_list.size(), s, ctx->prt.p, ctx->fir4c_list.p, ctx->d_fir4tab.p,
                                      ctx->er_off.p, erg, ctx->hspec.p));
    if (F.hblocks_gen > 0)   // blocks of k_fir4/k_fir8-engine presets return at once
        HIPCHK(ctx, launch_fir_h((unsigned)F.hblocks, F.lds, s, ctx->prt.p, ctx->h_begin.p, b.P,
                                 ctx->fir_plans.dev.p, ctx->fir_plan_of.p, ctx->hscratch.p, ctx->hspec.p));
    return MSG_OK;
}

static int enqueue_generate(msg_ctx* ctx, Batch& b) {
    const std::vector<int32_t>& gen = b.f32.gen_list;
    const std::vector<int32_t>& gen64 = b.g64.gen_list;
    if (!gen.empty())
        hipLaunchKernelGGL(k_gen_normal<false>, dim3((unsigned)gen.size()), dim3(GEN_T), 0, b.s,
                           ctx->presets.p, ctx->events.p, ctx->prt.p, ctx->gen_list.p, (int)gen.size(),
                           ctx->dzig, ctx->d_jump.p, ctx->micro.p, (double*)nullptr, (const int64_t*)nullptr);
    HIPCHK(ctx, hipGetLastError());
    if (!gen64.empty())   // raw normals of the float64 chain's normal-driven generators
        hipLaunchKernelGGL(k_gen_normal<true>, dim3((unsigned)gen64.size()), dim3(GEN_T), 0, b.s,
                           ctx->presets.p, ctx->events.p, ctx->prt.p, ctx->gen64_list.p, (int)gen64.size(),
                           ctx->dzig, ctx->d_jump.p, ctx->micro.p, ctx->micro64.p, (const int64_t*)ctx->gen64_off.p);
    HIPCHK(ctx, hipGetLastError());
    return MSG_OK;
}

// The float32 spectral chain, then the float64 grain chain.
static int enqueue_spectral(msg_ctx* ctx, Batch& b) {
    const Batch::F32& F = b.f32;
    const Batch::G64& G = b.g64;
    hipStream_t s = b.s;
    if (!F.spec3.empty())
        HIPCHK(ctx, launch_spec3((unsigned)F.spec3.size(), s, ctx->events.p, ctx->ert.p, ctx->prt.p, ctx->d_spec3_tab.p,
                                 ctx->spec3_list.p, (int)F.spec3.size(), ctx->micro.p, ctx->grain.p));
    for (int i = 0; i < SPEC_CT_PLANS; ++i)
        if (F.ct_off[i + 1] > F.ct_off[i])
            HIPCHK(ctx, launch_spectral_ct(i, (unsigned)(F.ct_off[i + 1] - F.ct_off[i]), s, ctx->events.p, ctx->ert.p,
                                           ctx->prt.p, ctx->d_spec_ct_tab[i].p, ctx->spec_ct_list.p + F.ct_off[i],
                                           F.ct_off[i + 1] - F.ct_off[i], ctx->micro.p, ctx->grain.p));
    if (!F.spec_small.empty())
        HIPCHK(ctx, launch_spectral(false, (unsigned)F.spec_small.size(), F.small_lds, s, ctx->presets.p,
                                    ctx->events.p, ctx->ert.p, ctx->prt.p, ctx->grain_plans.dev.p, ctx->spec_small.p,
                                    (int)F.spec_small.size(), ctx->micro.p, ctx->grain.p));
    if (!F.spec_big.empty())
        HIPCHK(ctx, launch_spectral(true, (unsigned)F.spec_big.size(), F.big_lds, s, ctx->presets.p,
                                    ctx->events.p, ctx->ert.p, ctx->prt.p, ctx->grain_plans.dev.p, ctx->spec_big.p,
                                    (int)F.spec_big.size(), ctx->micro.p, ctx->grain.p));
    if (!G.lds.empty())
        HIPCHK(ctx, launch_grain64(nullptr, (unsigned)G.lds.size(), G.cap * 16, s, ctx->presets.p, ctx->ev64.p,
                                   ctx->prt.p, ctx->plans64.dev.p, ctx->g64_list.p, (int)G.lds.size(),
                                   ctx->irbank.p, ctx->imgbank.p, ctx->dzig, ctx->micro64.p, ctx->grain64.p,
                                   ctx->save64.p, ctx->grain.p));
    if (!G.glb.empty())
        HIPCHK(ctx, launch_grain64(&G.gg, G.g_grid, 0, s, ctx->presets.p, ctx->ev64.p, ctx->prt.p, ctx->plans64.dev.p,
                                   ctx->g64_list.p + G.lds.size(), (int)G.glb.size(), ctx->irbank.p,
                                   ctx->imgbank.p, ctx->dzig, ctx->micro64.p, ctx->grain64.p, ctx->save64.p,
                                   ctx->grain.p));
    if (G.n_lds_chains > 0)
        HIPCHK(ctx, launch_chain64(nullptr, (unsigned)G.n_lds_chains, G.cap * 16, s, ctx->presets.p, ctx->ev64.p,
                                   ctx->chains.p, (int)G.n_lds_chains, ctx->plans64.dev.p, ctx->grain64.p,
                                   ctx->state64.p, ctx->grain.p));
    if (!G.chains_glb.empty())
        HIPCHK(ctx, launch_chain64(&G.gg, G.c_grid, 0, s, ctx->presets.p, ctx->ev64.p, ctx->chains.p + G.n_lds_chains,
                                   (int)G.chains_glb.size(), ctx->plans64.dev.p, ctx->grain64.p, ctx->state64.p,
                                   ctx->grain.p));
    return MSG_OK;
}

// Overlap-add x ADSR.
static int enqueue_ola(msg_ctx* ctx, Batch& b) {
    if (b.tiles > 0) {
        hipLaunchKernelGGL(k_ola_env, dim3((unsigned)b.tiles), dim3(OLA_T), 0, b.s, ctx->events.p, ctx->grain_off.p,
                           ctx->prt.p, ctx->tile_begin.p, b.P, ctx->grain.p, ctx->mono_a.p);
        HIPCHK(ctx, hipGetLastError());
    }
    return MSG_OK;
}

// FIR (presets without ER/IR pass a through); sets b.yb.
static int enqueue_fir(msg_ctx* ctx, Batch& b) {
    const Batch::Fir& F = b.fir;
    hipStream_t s = b.s;
    b.yb = ctx->mono_a.p;
    if (F.hblocks <= 0) return MSG_OK;
    if (!F.h_early)
        if (const int rc = enqueue_h_spectra(ctx, b)) return rc;
    stage_mark(ctx, 8, s);
    for (int i = 0; i < 6; ++i) {
        if (F.job_off[i + 1] <= F.job_off[i]) continue;
        const unsigned nj = (unsigned)(F.job_off[i + 1] - F.job_off[i]);
        if (i == 5 && ctx->sw.fir8p > 0) {
            // persistent: one workgroup per CU (at most one per block), a multiple of the XCD
            // count.  Long outputs (h_early: milliseconds per launch) leave one CU in eight
            // to the other streams' small kernels, which cannot start beside a k_fir8p
            // workgroup (its VGPRs fill the CU): C5 118.4 - 119.4 ms with 224 of 256 CUs
            // against 118.8 - 124.0 with all of them; C3 keeps every CU
            const int cus = ctx->sw.fir8p_cus > 0 ? std::min(ctx->sw.fir8p_cus, ctx->n_cu)
                                               : (F.h_early ? ctx->n_cu - ctx->n_cu / 8 : ctx->n_cu);
            const unsigned grid = (unsigned)std::max(MSG_XCDS, (std::min((int)nj, cus) / MSG_XCDS) * MSG_XCDS);
            HIPCHK(ctx, fir8_counters(ctx, s));
            HIPCHK(ctx, launch_fir8p(nj, grid, s, ctx->prt.p, ctx->fir_jobs.p + F.job_off[i],
                                     ctx->d_fir4tab.p, ctx->hspec.p, ctx->mono_a.p, ctx->mono_y.p, ctx->fir8_ctr.p,
                                     F.n_ola > 0 ? ctx->events.p : nullptr, ctx->grain_off.p, ctx->grain.p,
                                     ctx->fir_lo.p));
        } else if (i == 5)
            HIPCHK(ctx, launch_fir8(nj, s, ctx->prt.p, ctx->fir_jobs.p + F.job_off[i], ctx->d_fir4tab.p, ctx->hspec.p,
                                    ctx->mono_a.p, ctx->mono_y.p));
        else if (i == 4 && ctx->sw.fir4)
            HIPCHK(ctx, launch_fir4(16384, nj, s, ctx->prt.p, ctx->fir_jobs.p + F.job_off[i], ctx->d_fir4tab.p,
                                    ctx->hspec.p, ctx->mono_a.p, ctx->mono_y.p));
        else
            HIPCHK(ctx, launch_fir2(1024 << i, nj, s, ctx->prt.p, ctx->fir_jobs.p + F.job_off[i],
                                    ctx->d_fir2tab[i].p, ctx->hspec.p, ctx->mono_a.p, ctx->mono_y.p));
    }
    stage_mark(ctx, 9, s);
    // presets with fir_on == 0 in a mixed batch: copy a -> y
    for (int p = 0; p < b.P; ++p)
        if (!b.prt[p].fir_on)
            HIPCHK(ctx, hipMemcpyAsync(ctx->mono_y.p + b.prt[p].y_off, ctx->mono_a.p + b.prt[p].y_off,
                                       sizeof(float) * b.prt[p].out_n, hipMemcpyDeviceToDevice, s));
    b.yb = ctx->mono_y.p;
    return MSG_OK;
}

// The chirp kernel spectrum of an odd length n (kernels_stereo_odd.h), cached
// per context by n and built on first use.
static int odd_chirp(msg_ctx* ctx, Batch& b, int64_t n, const double2** spec) {
    auto it = ctx->so_bp.find(n);
    if (it == ctx->so_bp.end()) {
        // bound the cache (one entry per distinct odd length, for the
        // life of the process): drop least-recently-used spectra of earlier
        // batches while the cache holds more than 1 GiB (erase frees the entry;
        // the free waits for the batches that read it)
        auto bytes = [&]() {
            size_t n_bytes = 0;
            for (auto& kv : ctx->so_bp) n_bytes += kv.second.cap * sizeof(double2);
            return n_bytes;
        };
        while (bytes() > ((size_t)1 << 30)) {
            int64_t victim = -1;
            uint64_t oldest = ctx->batch_serial;
            for (auto& kv : ctx->so_bp_use)
                if (kv.second < oldest) { oldest = kv.second; victim = kv.first; }
            if (victim < 0) break;
            ctx->so_bp.erase(victim);
            ctx->so_bp_use.erase(victim);
        }
        it = ctx->so_bp.emplace(n, DevBuf<double2>()).first;
        HIPCHK(ctx, it->second.ensure(stereo_odd_len(n, ctx->sw.so_row, ctx->sw.so_col)));
        HIPCHK(ctx, launch_stereo_odd_kernel(n, ctx->sw.so_row, ctx->sw.so_col, it->second.p, ctx->so_A.p, b.s));
    }
    ctx->so_bp_use[n] = ctx->batch_serial;
    *spec = it->second.p;
    return MSG_OK;
}

// Stereo, tanh, normalise (with the float64 FIR of the flagged presets).
static int enqueue_stereo(msg_ctx* ctx, Batch& b) {
    const Batch::Fir64& S = b.f64;
    const int P = b.P;
    hipStream_t s = b.s;
    float* yb = b.yb;
    // peak of L (and the float64 FIR's error predictor) over the float32 y
    StereoSync sy{};
    sy.flag64 = S.on ? ctx->f64_flag.p : nullptr;
    sy.part = S.on ? ctx->st_part.p : nullptr;
    sy.stats = S.on ? ctx->f64_stats.p : nullptr;
    sy.f64mode = S.on ? ctx->sw.fir64 : 0;
    HIPCHK(ctx, launch_stereo_max((unsigned)b.stiles, s, ctx->prt.p, ctx->st_begin.p, P, yb, ctx->maxbits.p, sy));
    if (S.on)   // the float64 FIR's predictor per preset, from the tiles' partial sums
        HIPCHK(ctx, launch_stereo_pred((unsigned)P, s, ctx->prt.p, ctx->st_begin.p, b.stiles, ctx->maxbits.p, sy));
    if (S.on) {   // flagged presets: the FIR again in float64, y overwritten (kernels_fir64.h)
        Fir64Launch a;
        a.rt = ctx->prt.p; a.n_presets = P; a.flag64 = ctx->f64_flag.p; a.maxbits = ctx->maxbits.p;
        a.slot_preset = ctx->f64_slot_preset.p; a.n_slots = ctx->f64_nslots.p;
        a.n_cand = S.cand; a.cap = S.cap;
        a.fr = ctx->f64rt.p; a.tmax = (int)((S.hmax + H_BUILD_TILE - 1) / H_BUILD_TILE); a.qmax = S.qmax;
        a.bmax = S.bmax;
        a.er_off = ctx->er_off.p; a.er_gain = er_gains(ctx, b); a.irbank = ctx->irbank.p;
        a.h64 = ctx->f64_h.p; a.h_stride = S.hstride; a.hs64 = ctx->f64_hs.p; a.hs_stride = S.hsstride;
        a.plans = ctx->plans64.dev.p; a.plan = S.plan;
        a.lds_bytes = FIR64_K * (int)sizeof(double2);   // the packed transform and its Nyquist slot
        a.x = ctx->mono_a.p; a.y = yb;
        HIPCHK(ctx, launch_fir64_flag(a, s));
        if (b.fir.n_ola > 0) {   // the flagged ola_fir presets' mono a, which k_fir8p never wrote
            const int tmax = (int)((b.fir.ola_nmax + OLA_TILE - 1) / OLA_TILE);
            hipLaunchKernelGGL(k_ola_slots, dim3((unsigned)std::min<int64_t>((int64_t)S.cand * tmax, 1024)),
                               dim3(OLA_T), 0, s, ctx->events.p, ctx->grain_off.p, ctx->prt.p, ctx->f64_slot_preset.p,
                               ctx->f64_nslots.p, tmax, ctx->grain.p, ctx->mono_a.p);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, launch_fir64(a, s));
    }
    ++ctx->batch_serial;
    for (int p : b.odd_presets) {           // odd out_n: R = irfft(rfft(roll(y, -dr)) . rot) (MS:432-435)
        const int64_t n = b.info[p].out_n;
        const double2* chirp = nullptr;
        if (const int rc = odd_chirp(ctx, b, n, &chirp)) return rc;
        const double w = std::min(std::max(b.presets[p].stereo_width, 0.0), 1.0);
        HIPCHK(ctx, launch_stereo_odd(n, ctx->sw.so_row, ctx->sw.so_col, b.prt[p].dr, w, yb + b.prt[p].y_off, chirp, ctx->so_A.p,
                                      ctx->so_r2.p + b.prt[p].r2_off, s));
    }
    int odd_tmax = 0;
    for (int p : b.odd_presets) odd_tmax = std::max(odd_tmax, b.st_count[p]);
    if (S.on)   // the float64 presets' peak from their new y (and R)
        HIPCHK(ctx, launch_stereo_remax((unsigned)std::min<int64_t>((int64_t)S.cand * S.stmax, 256), s, ctx->prt.p, ctx->st_count.p,
                                        ctx->f64_slot_preset.p, ctx->f64_nslots.p, S.stmax, yb, ctx->so_r2.p,
                                        ctx->maxbits.p));
    if (b.n_odd > 0)   // odd lengths: the peak of the rotated R
        HIPCHK(ctx, launch_stereo_remax((unsigned)std::min<int64_t>((int64_t)b.n_odd * odd_tmax, 4096), s, ctx->prt.p,
                                        ctx->st_count.p, ctx->odd_list.p, ctx->odd_cnt.p, odd_tmax, yb, ctx->so_r2.p,
                                        ctx->maxbits.p));
    HIPCHK(ctx, launch_stereo_out((unsigned)b.stiles, s, ctx->prt.p, ctx->st_begin.p, P, yb, ctx->so_r2.p,
                                  ctx->maxbits.p, b.out_dev));
    return MSG_OK;
}

// ---------------------------------------------------------------------------
// host clocks and mirrors
// ---------------------------------------------------------------------------
// host_sum[0..7]: plan, records, pinned upload, then the splits plan sizes,
// plan events + tap merge, preset records, event records, lists + buffers.
static void host_clocks(msg_ctx* ctx, const Batch& b) {
    if (!ctx->prof.batch) return;
    const auto h3 = Batch::hclock::now();
    auto ms = [](Batch::hclock::time_point a, Batch::hclock::time_point z) {
        return std::chrono::duration<double, std::milli>(z - a).count();
    };
    ctx->prof.host_sum[0] += ms(b.h0, b.h1);
    ctx->prof.host_sum[1] += ms(b.h1, b.h2);
    ctx->prof.host_sum[2] += ms(b.h2, h3);
    ctx->prof.host_sum[3] += ms(b.h0, b.hA);
    ctx->prof.host_sum[4] += ms(b.hA, b.h1);
    ctx->prof.host_sum[5] += ms(b.h1, b.hB);
    ctx->prof.host_sum[6] += ms(b.hB, b.hC);
    ctx->prof.host_sum[7] += ms(b.hC, b.h2);
    ctx->prof.ola_fir_sum += b.fir.n_ola;
    ctx->prof.gen_events_sum += (double)b.f32.n_events;
    ctx->prof.gen_grains_sum += (double)b.f32.n_owners;
    ctx->prof.spec_runs_sum += (double)b.f32.n_spec_runs;
    ++ctx->prof.host_cnt;
}

// Host mirrors of the last batch (msg_last_*), written only on success.
static void keep_mirrors(msg_ctx* ctx, const Batch& b) {
    ctx->h_info = b.info;
    ctx->h_prt = b.prt;
    ctx->h_slot_base = b.slot_base;
    ctx->h_ev64 = b.g64.ev;
    ctx->h_last64 = b.g64.last;
    ctx->h_micro_last = b.f32.micro_last;
    static_assert(MSG_ROUTE_CT + SPEC_CT_PLANS == MSG_ROUTE_SPEC3, "msg_spec_route numbers the compile-time plans");
    int64_t* const rc = ctx->h_spec_routes;
    rc[MSG_ROUTE_COPY] = b.f32.n_copy;
    rc[MSG_ROUTE_SMALL] = (int64_t)b.f32.spec_small.size() - b.f32.n_copy;
    rc[MSG_ROUTE_BIG] = (int64_t)b.f32.spec_big.size();
    for (int c = 0; c < SPEC_CT_PLANS; ++c) rc[MSG_ROUTE_CT + c] = (int64_t)b.f32.ct[c].size();
    rc[MSG_ROUTE_SPEC3] = (int64_t)b.f32.spec3.size();
    rc[MSG_ROUTE_F64] = (int64_t)b.g64.ev.size();
    ctx->last_n = b.P;
}
