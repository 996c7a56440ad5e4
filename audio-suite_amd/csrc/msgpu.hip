// msgpu.hip — libmsgpu: host orchestration and the C ABI (include/msgpu.h).
//
// One msg_render_batch call renders N independent presets (each one call of
// the reference's render(), microsound_0.2.1/main_v2.py:588-792) on one
// MI355X: device planner -> generator -> LDS spectral chain -> overlap-add x
// ADSR -> partitioned FFT FIR (ER + IR) -> stereo/tanh/normalise.  All work is
// batched across presets so every launch has thousands of workgroups.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <sched.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "msg_common.h"
#include "ziggurat_tables.h"
#include "nprng.h"
#include "plan.h"
#include "fftplan.h"
#include "fft_lds.h"
#include "kernels_core.h"
#include "launch.h"
#include "digest.h"
#include "loudness.h"
#include "lrange.h"
#include "truepeak.h"
#include "pcm.h"
#include "pcm_shape.h"
#include "limit.h"
#include "edges.h"
#include "filter.h"
#include "image.h"
#include "dynamics.h"
#include "gate.h"
#include "flac.h"
#include "host_pool.h"
#include "er_merge.h"
#include "batch.h"
#include "../../include/msgpu.h"
#include "ctx.h"

namespace {

const nprng::Zig kHostZig = {zig_ki_double, zig_wi_double, zig_fi_double,
                             zig_ke_double, zig_we_double, zig_fe_double};

thread_local std::string g_err;   // errors before a context exists

}  // namespace

// the longest output a preset may have: every kernel indexes a preset's frames
// with 32-bit integers (round 4 stopped at 2^29, where a 32-bit byte offset of
// the float2 output from the preset's own base ran out; the offsets are now
// formed from each tile's or block's base)
constexpr int64_t MSG_MAX_FRAMES = ((int64_t)1 << 31) - ((int64_t)1 << 20);

#define HIPCHK(ctx, expr)                                                        \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) {                                                  \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);      \
            return MSG_E_DEVICE;                                                 \
        }                                                                        \
    } while (0)

static int fail(msg_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_err = msg;
    return code;
}

// ---------------------------------------------------------------------------
// FFT plan creation
// ---------------------------------------------------------------------------
// A plan's table (scalars S read as pairs V) on the device, owned by the store.
template <class P, class S, class V>
static hipError_t upload(PlanStoreT<P, S>& ps, const std::vector<S>& v, const V** out) {
    DevBuf<S> d;
    const hipError_t e = d.upload(v.data(), v.size());
    *out = reinterpret_cast<const V*>(d.p);
    ps.allocs.push_back(std::move(d));
    return e;
}

static bool make_fftdesc(PlanStore& ps, int m, FftDesc& d, std::string& why) {
    std::vector<int> rad;
    memset(&d, 0, sizeof(d));
    d.m = m;
    if (fftplan::factor(m, rad)) {
        d.blue = 0;
        d.size = m;
    } else {
        d.blue = 1;
        d.size = fftplan::next_pow2(2 * m - 1);
        fftplan::factor(d.size, rad);
        std::vector<float> chirp, bspec;
        fftplan::bluestein(m, d.size, chirp, bspec);
        if (upload(ps, chirp, &d.chirp) != hipSuccess || upload(ps, bspec, &d.bspec) != hipSuccess) {
            why = "hip upload failed";
            return false;
        }
    }
    if ((int)rad.size() > FFT_MAXRAD) { why = "too many radix passes"; return false; }
    d.nrad = (int)rad.size();
    for (size_t i = 0; i < rad.size(); ++i) d.rad[i] = rad[i];
    d.tw_hi_n = (d.size + TW_LO - 1) / TW_LO;
    if (upload(ps, fftplan::twiddles(d.size, TW_LO, 1), &d.tw0) != hipSuccess ||
        upload(ps, fftplan::twiddles(d.size, d.tw_hi_n, TW_LO), &d.tw1) != hipSuccess) {
        why = "hip upload failed";
        return false;
    }
    return true;
}

// Real-FFT plan for n samples; returns index or -1.
static int real_plan(PlanStore& ps, int n, std::string& why) {
    auto it = ps.by_n.find(n);
    if (it != ps.by_n.end()) return it->second;
    RealPlan rp;
    memset(&rp, 0, sizeof(rp));
    rp.n = n;
    rp.even = (n % 2 == 0);
    const int m = rp.even ? n / 2 : n;
    if (!make_fftdesc(ps, m, rp.c, why)) return -1;
    rp.lds_c = lds_phys(std::max(rp.even ? m + 1 : m, rp.c.size));
    if (rp.even) {
        rp.rt_hi_n = (m + 1 + TW_LO - 1) / TW_LO;
        if (upload(ps, fftplan::twiddles(n, TW_LO, 1), &rp.rt0) != hipSuccess ||
            upload(ps, fftplan::twiddles(n, rp.rt_hi_n, TW_LO), &rp.rt1) != hipSuccess) {
            why = "hip upload failed";
            return -1;
        }
    }
    rp.lds_bytes = (rp.lds_c + TW_LO + rp.c.tw_hi_n + (rp.even ? TW_LO + rp.rt_hi_n : 0)) * 8;
    const int idx = (int)ps.host.size();
    ps.host.push_back(rp);
    ps.by_n[n] = idx;
    ps.dirty = true;
    return idx;
}

// float64 real-FFT plan for n samples (fft64.h); returns index or -1.
static int real64_plan(Plan64Store& ps, int n, std::string& why) {
    auto it = ps.by_n.find(n);
    if (it != ps.by_n.end()) return it->second;
    Real64Plan rp;
    memset(&rp, 0, sizeof(rp));
    rp.n = n;
    rp.even = (n % 2 == 0);
    const int m = rp.even ? n / 2 : n;
    Fft64& c = rp.c;
    c.m = m;
    std::vector<int> rad;
    std::vector<double> tab;
    if (fft64plan::factor(m, rad)) {
        c.blue = 0;
        c.size = m;
    } else {
        c.blue = 1;
        c.size = fft64plan::next_pow2(2 * m - 1);
        fft64plan::factor(c.size, rad);
        std::vector<double> bs;
        fft64plan::chirp(m, tab);
        fft64plan::bluestein_spec(m, c.size, tab, bs);
        if (upload(ps, tab, &c.chirp) != hipSuccess || upload(ps, bs, &c.bspec) != hipSuccess) {
            why = "hip upload failed";
            return -1;
        }
    }
    if ((int)rad.size() > F64_MAXRAD) { why = "too many radix passes"; return -1; }
    c.nrad = (int)rad.size();
    for (size_t i = 0; i < rad.size(); ++i) c.rad[i] = rad[i];
    fft64plan::twiddles(c.size, tab);
    if (upload(ps, tab, &c.tw) != hipSuccess) { why = "hip upload failed"; return -1; }
    if (rp.even) {
        std::vector<double> rt(2 * (size_t)(m + 1));
        for (int k = 0; k <= m; ++k) {
            const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
            rt[2 * k] = (double)cosl(a);
            rt[2 * k + 1] = (double)sinl(a);
        }
        if (upload(ps, rt, &rp.rt) != hipSuccess) { why = "hip upload failed"; return -1; }
    }
    rp.cap = std::max(std::max(c.size, rp.even ? m + 1 : n), n);
    const int idx = (int)ps.host.size();
    ps.host.push_back(rp);
    ps.by_n[n] = idx;
    ps.dirty = true;
    return idx;
}

// The descriptors on the device; a store stays dirty until its copy has run.
template <class P, class S>
static hipError_t sync_plans(PlanStoreT<P, S>& ps, hipStream_t s) {
    if (!ps.dirty) return hipSuccess;
    hipError_t e = ps.dev.ensure(ps.host.size());
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(ps.dev.p, ps.host.data(), ps.host.size() * sizeof(P), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) ps.dirty = false;
    return e;
}

// Bessel J_m(x), m >= 0, power series (x <= 0.9 here).
static double bessel_j(int m, double x) {
    double term = 1.0;
    for (int k = 1; k <= m; ++k) term *= (x / 2.0) / k;
    double sum = term;
    for (int k = 1; k < 60; ++k) {
        term *= -(x / 2.0) * (x / 2.0) / ((double)k * (double)(k + m));
        sum += term;
        if (std::fabs(term) < 1e-30) break;
    }
    return sum;
}

// Choose (N, P, Q) minimising FFT work for an M-tap FIR over n outputs (h is
// built in the time domain by k_h_build, so any N with P < N qualifies).
// fir8: also consider N = 65536 with one partition (k_fir8: two half-size
// transforms per transform of N, P = M).
// M8: the length of the filter k_fir8 would apply (its spectrum holds every
// in-range ER tap and the whole IR, so it can be longer than an M capped at
// out_n); the 65536-point candidate needs M8 + B - 1 <= N or it wraps.
static void choose_fir(int64_t M, int64_t n, int& N, int& P, int& Q, bool fir8, int64_t M8 = -1) {
    if (M8 < M) M8 = M;
    double best = 1e300;
    N = FIR_NMAX; P = (int)std::min<int64_t>(M, FIR_NMAX / 2); Q = (int)((M + P - 1) / P);
    for (int lg = 11; lg <= 15; ++lg) {   // k_fir2 / k_fir4 sizes: M = N/2 in 1024..16384
        const int NN = 1 << lg;
        for (int q = 1; q <= 64; ++q) {
            const int64_t pp = (M + q - 1) / q;
            if (pp >= NN) continue;
            const int64_t B = NN - pp + 1;
            const int64_t blocks = (n + B - 1) / B;
            const double cost = (double)blocks * (q + 1) * NN * lg + (double)blocks * NN * 4.0;
            if (cost < best) { best = cost; N = NN; P = (int)pp; Q = q; }
        }
    }
    if (fir8 && M8 < FIR8_N / 2 + FIR8_N / 4) {   // B >= N/4
        const int64_t B = FIR8_N - M8 + 1;
        const int64_t blocks = (n + B - 1) / B;
        const double cost = (double)blocks * 2 * FIR8_N * 16 + (double)blocks * FIR8_N * 4.0;
        if (cost < best) { best = cost; N = FIR8_N; P = (int)M8; Q = 1; }
    }
}

using specshare::spec_ops;   // gen_share.h: shared with the host-only build

static bool normal_driven(int gen_mode) {
    return gen_mode == MSG_GEN_GAUSSIAN_CLICK || gen_mode == MSG_GEN_NOISE_BURST || gen_mode == MSG_GEN_SKEWED ||
           gen_mode == MSG_GEN_RESONANT || gen_mode == MSG_GEN_FALLBACK;
}
// Presets whose grains run the float64 chain (kernels_grain64.h): the
// generators outside the normal-driven closed forms, and every stage whose
// reference result hinges on float64 magnitudes or noise floors.
static bool is_precise(const msg_preset& p) {
    const uint32_t f64_stages = MSG_F_PARTIAL_LOCK | MSG_F_CEP_WARP | MSG_F_RES_BANK | MSG_F_WAVEGUIDE |
                                MSG_F_EVENT_FEEDBACK | MSG_F_IMPRINT | MSG_F_MULTIBAND;
    return (p.flags & f64_stages) || !normal_driven(p.gen_mode);
}

// Stages of the float64 chain one event runs, with the reference's own
// length / identity guards (MS:42, 105, 119-121, 132-134, 152, 372, 389).
static int g64_ops(const msg_preset& p, const msg_event& e) {
    int ops = 0;
    const int n = e.n;
    const bool stretch_id = std::fabs(e.stretch - 1.0) < 1e-9;
    if ((p.flags & MSG_F_BANDLIMIT) && n >= 8) ops |= G64_LOWPASS;
    if ((p.flags & MSG_F_NL_WARP) && n >= 16) ops |= G64_WARP;
    if ((p.flags & MSG_F_CEP_WARP) && n >= 64) ops |= G64_CEP;
    if (p.flags & MSG_F_PARTIAL_LOCK) {
        if (n >= 64 && !stretch_id) ops |= G64_LOCK;
    } else if (n >= 16 && !stretch_id) {
        ops |= G64_STRETCH;
    }
    if ((p.flags & MSG_F_RES_BANK) && n >= 32) ops |= G64_RES;
    if ((p.flags & MSG_F_WAVEGUIDE) && n >= 64) ops |= G64_WG;
    if (p.flags & MSG_F_MULTIBAND) ops |= G64_MB;
    if (p.flags & (MSG_F_EVENT_FEEDBACK | MSG_F_IMPRINT)) ops |= G64_CHAIN;
    return ops;
}

static void stage_mark(msg_ctx* ctx, int i, hipStream_t s) {
    Gate& g = ctx->gate;
    if (g.wait >= 0 || g.rec >= 0) {
        std::lock_guard<std::mutex> lk(g_gate_mu);   // the peer may be unlinked by msg_destroy
        if (g.peer) {
            // the gate's wait comes before the stage's profiling event, so a stage's
            // time is its kernels' span on the stream, not the time it was held
            if (i == g.wait && g.peer->gate.armed.load())
                hipStreamWaitEvent(s, g.peer->gate.ev, 0);
            if (i == g.rec) {
                hipEventRecord(g.ev, s);
                g.armed.store(true);
            }
        }
    }
    if (ctx->prof.batch) hipEventRecord(ctx->prof.ev[ctx->prof.cur][i], s);
}

// A batch on a different stream than the context's last one waits for that
// batch's end (the staging arena and buffers are stream-ordered).
static hipError_t stream_handover(msg_ctx* ctx, hipStream_t s) {
    if (ctx->done_armed && s != ctx->last_stream) return hipStreamWaitEvent(s, ctx->done_ev, 0);
    return hipSuccess;
}
static hipError_t stream_done(msg_ctx* ctx, hipStream_t s) {
    if (!ctx->done_ev) {
        const hipError_t e = ctx->done_ev.create(hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    ctx->last_stream = s;
    ctx->done_armed = true;
    return hipEventRecord(ctx->done_ev, s);
}

// Records done_ev on every exit of a call that may have enqueued work, the
// early fail() returns included: a later batch on another stream
// then still waits for this one before it reuses the staging arena and buffers.
struct DoneGuard {
    msg_ctx* ctx;
    hipStream_t s;
    bool armed = true;
    DoneGuard(msg_ctx* c, hipStream_t st) : ctx(c), s(st) {}
    hipError_t finish() { armed = false; return stream_done(ctx, s); }
    ~DoneGuard() { if (armed) stream_done(ctx, s); }
};

// k_fir8p's per-XCD block counters: zeroed once; every launch leaves them zero
static hipError_t fir8_counters(msg_ctx* ctx, hipStream_t s) {
    if (ctx->fir8_ctr.p) return hipSuccess;
    const hipError_t e = ctx->fir8_ctr.ensure((size_t)(MSG_XCDS + 1) * FIR8P_CTR);
    if (e != hipSuccess) return e;
    return hipMemsetAsync(ctx->fir8_ctr.p, 0, sizeof(int32_t) * ctx->fir8_ctr.cap, s);
}

// Wait for the context's last batch (not the whole device: other contexts'
// streams keep running).
static hipError_t wait_last(msg_ctx* ctx) {
    return ctx->done_armed ? hipEventSynchronize(ctx->done_ev) : hipSuccess;
}

#include "render_stages.h"

// msg_fir: one PresetRt per signal (signal i at frame i * n of x and y) and its
// jobs (i, j) for j = 0, step, 2 step, ... < nblk.
static void sf_signals(int n_signals, int64_t n, int N, int P, int Q, int64_t B, int64_t nblk, int64_t step,
                       std::vector<PresetRt>& prt, std::vector<int2>& jobs) {
    prt.resize((size_t)n_signals);
    jobs.reserve((size_t)(((nblk + step - 1) / step) * n_signals));
    for (int i = 0; i < n_signals; ++i) {
        PresetRt& r = prt[i];
        memset(&r, 0, sizeof(r));
        r.out_n = n;
        r.y_off = (int64_t)i * n;
        r.fir_on = 1; r.fir_N = N; r.fir_P = P; r.fir_Q = Q; r.fir_B = (int32_t)B;
        for (int64_t j = 0; j < nblk; j += step) jobs.push_back(make_int2(i, (int)j));
    }
}

// msg_fir's uploads: the records, the jobs, the spectrum jobs and the taps
// (float for the k_fir8 engine, float64 for the IR-spectrum kernel).  Pageable
// sources are staged before hipMemcpyAsync returns, so they may go afterwards.
template <class T>
static int sf_upload(msg_ctx* ctx, hipStream_t s, const std::vector<PresetRt>& prt, const std::vector<int2>& jobs,
                     const int64_t* irjobs, size_t n_irjobs, DevBuf<T>& taps_dev, const T* taps, int64_t M) {
    HIPCHK(ctx, ctx->sf_prt.ensure(prt.size()));
    HIPCHK(ctx, ctx->sf_jobs.ensure(jobs.size()));
    HIPCHK(ctx, taps_dev.ensure((size_t)M));
    HIPCHK(ctx, ctx->sf_irjobs.ensure(n_irjobs));
    HIPCHK(ctx, hipMemcpyAsync(ctx->sf_prt.p, prt.data(), sizeof(PresetRt) * prt.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->sf_jobs.p, jobs.data(), sizeof(int2) * jobs.size(), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(taps_dev.p, taps, sizeof(T) * (size_t)M, hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(ctx->sf_irjobs.p, irjobs, sizeof(int64_t) * n_irjobs, hipMemcpyHostToDevice, s));
    return MSG_OK;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int msg_abi_version(void) { return MSG_ABI_VERSION; }

int msg_host_threads(void) { return HostPool::get().threads(); }

const char* msg_last_error(msg_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

msg_ctx* msg_create(int device_ordinal) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { g_err = "no HIP device available"; return nullptr; }
    if (device_ordinal < 0 || device_ordinal >= ndev) { g_err = "bad device ordinal"; return nullptr; }
    if (hipSetDevice(device_ordinal) != hipSuccess) { g_err = "hipSetDevice failed"; return nullptr; }
    // every early return frees what is already there through ~msg_ctx
    std::unique_ptr<msg_ctx> ctx(new msg_ctx());
    ctx->device = device_ordinal;
    ctx->sw = Switches::from_env();
    auto up = [](auto& dst, const auto* src, size_t n) { return dst.upload(src, n) == hipSuccess; };
    auto up2 = [](DevBuf<float2>& dst, bool ok, const std::vector<float>& tab) {   // pairs of floats
        return ok && dst.upload(reinterpret_cast<const float2*>(tab.data()), tab.size() / 2) == hipSuccess;
    };
    if (!up(ctx->d_ki, zig_ki_double, 256) || !up(ctx->d_wi, zig_wi_double, 256) ||
        !up(ctx->d_fi, zig_fi_double, 256) || !up(ctx->d_ke, zig_ke_double, 256) ||
        !up(ctx->d_we, zig_we_double, 256) || !up(ctx->d_fe, zig_fe_double, 256)) {
        g_err = "uploading ziggurat tables failed";
        return nullptr;
    }
    ctx->dzig = nprng::Zig{ctx->d_ki.p, ctx->d_wi.p, ctx->d_fi.p, ctx->d_ke.p, ctx->d_we.p, ctx->d_fe.p};
    JumpTab jt;
    for (int l = 0; l < GEN_T; ++l) {
        const nprng::Jump j = nprng::jump_of((uint64_t)l + 1);
        jt.a[l] = j.a; jt.s[l] = j.s;
    }
    const nprng::Jump j64 = nprng::jump_of(GEN_T);
    jt.a64 = j64.a; jt.s64 = j64.s;
    const nprng::Jump jG = nprng::jump_of((uint64_t)GEN_T * GEN_G);
    jt.aG = jG.a; jt.sG = jG.s;
    for (int i = 0; i < 256; ++i) {
        const float w = (float)(zig_wi_double[i] * 1048576.0);
        uint32_t wb;
        memcpy(&wb, &w, 4);
        jt.kw[i] = make_uint2((uint32_t)(zig_ki_double[i] >> 20), wb);
        jt.fif[i] = (float)zig_fi_double[i];
    }
    if (!up(ctx->d_jump, &jt, 1)) { g_err = "uploading jump table failed"; return nullptr; }
    std::vector<float> tab;
    for (int i = 0; i < 5; ++i)
        if (!up2(ctx->d_fir2tab[i], fir2_tables_host(1024 << i, tab), tab)) {
            g_err = "uploading FIR twiddle tables failed";
            return nullptr;
        }
    if (!up2(ctx->d_fir4tab, fir4_tables_host(16384, tab), tab)) {
        g_err = "uploading FIR4 twiddle tables failed";
        return nullptr;
    }
    for (int i = 0; i < SPEC_CT_PLANS; ++i)
        if (!up2(ctx->d_spec_ct_tab[i], spectral_ct_tables(i, tab), tab)) {
            g_err = "uploading spectral twiddle tables failed";
            return nullptr;
        }
    if (!up2(ctx->d_spec3_tab, spec3_tables(tab), tab)) {
        g_err = "uploading spectral twiddle tables failed";
        return nullptr;
    }
    {
        float tp_tab[TP_TAB_N];
        tp_table(tp_tab);
        if (!up(ctx->d_tp_tab, tp_tab, (size_t)TP_TAB_N)) { g_err = "uploading the true-peak taps failed"; return nullptr; }
    }
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device_ordinal) == hipSuccess && cu >= MSG_XCDS)
        ctx->n_cu = cu;
    if (ctx->prof.create_events() != hipSuccess) { g_err = "creating the stage events failed"; return nullptr; }
    spectral_ct_init_attrs();
    spec3_init_attrs();
    spectral_init_attrs();
    fir_init_attrs();
    fft_bench_init_attrs();
    grain64_init_attrs();
    stereo_odd_init_attrs();
    fir64_init_attrs();
    limit_init_attrs();
    dynamics_init_attrs();
    return ctx.release();
}

void msg_destroy(msg_ctx* ctx) {
    if (ctx) delete ctx;
}

// The owners' process-wide counts of what is live (dev_own.h): device
// allocations, their bytes, pinned allocations, events.  Not part of the ABI.
int msg_debug_live(int64_t out[4]) {
    const devown::Live& l = devown::g_live;
    out[0] = l.dev_n.load(devown::RLX);
    out[1] = l.dev_bytes.load(devown::RLX);
    out[2] = l.pinned_n.load(devown::RLX);
    out[3] = l.events.load(devown::RLX);
    return 0;
}

int msg_set_profiling(msg_ctx* ctx, int32_t on) {
    if (!ctx) return MSG_E_ARG;
    Prof& pr = ctx->prof;
    pr.collect();
    pr.on = on != 0;
    pr.every = on > 1 ? on : 1;
    pr.n = 0;
    if (pr.on) pr.reset_sums();
    return MSG_OK;
}

int msg_gate(msg_ctx* ctx, msg_ctx* peer, int32_t wait_stage, int32_t record_stage) {
    if (!ctx || peer == ctx || wait_stage < -1 || wait_stage > 9 || record_stage < -1 || record_stage > 9)
        return MSG_E_ARG;
    if (peer && peer->device != ctx->device) return MSG_E_ARG;
    Gate& g = ctx->gate;
    if (peer && !g.ev && g.ev.create(hipEventDisableTiming) != hipSuccess)
        return fail(ctx, MSG_E_DEVICE, "creating the gate event failed");
    std::lock_guard<std::mutex> lk(g_gate_mu);
    if (g.peer) {
        auto& v = g.peer->gate.gated_by;
        v.erase(std::remove(v.begin(), v.end(), ctx), v.end());
    }
    g.peer = peer;
    if (peer) peer->gate.gated_by.push_back(ctx);
    g.wait = peer ? wait_stage : -1;
    g.rec = peer ? record_stage : -1;
    g.armed.store(false);
    return MSG_OK;
}

// ms[0..9] stage times, [10..17] host clocks, [18] fused overlap-adds per batch,
// [19] float32-chain events per batch, [20] the grains the generator wrote for them,
// [21] the events among them that ran a spectral kernel
int msg_stage_times(msg_ctx* ctx, float* ms, int32_t n) {
    if (!ctx || !ms) return MSG_E_ARG;
    Prof& pr = ctx->prof;
    pr.collect();
    for (int i = 0; i < n && i < 10; ++i)
        ms[i] = pr.stage_cnt ? (float)(pr.stage_sum[i] / (double)pr.stage_cnt) : 0.f;
    for (int i = 10; i < n && i < 18; ++i)
        ms[i] = pr.host_cnt ? (float)(pr.host_sum[i - 10] / (double)pr.host_cnt) : 0.f;
    if (n > 18) ms[18] = pr.host_cnt ? (float)(pr.ola_fir_sum / (double)pr.host_cnt) : 0.f;
    if (n > 19) ms[19] = pr.host_cnt ? (float)(pr.gen_events_sum / (double)pr.host_cnt) : 0.f;
    if (n > 20) ms[20] = pr.host_cnt ? (float)(pr.gen_grains_sum / (double)pr.host_cnt) : 0.f;
    if (n > 21) ms[21] = pr.host_cnt ? (float)(pr.spec_runs_sum / (double)pr.host_cnt) : 0.f;
    return MSG_OK;
}

#include "host_abi.inc"

int msg_bench_fft(msg_ctx* ctx, int32_t n, int32_t reps, int32_t blocks, float* ms_out) {
    if (!ctx || !ms_out || n < 2 || reps < 1 || blocks < 1) return MSG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string why;
    const bool po2 = (n & (n - 1)) == 0;
    PlanStore& ps = po2 ? ctx->fir_plans : ctx->grain_plans;
    const int pi = real_plan(ps, n, why);
    if (pi < 0) return fail(ctx, MSG_E_DEVICE, why);
    HIPCHK(ctx, sync_plans(ps, nullptr));
    const RealPlan& rp = ps.host[pi];
    if (rp.lds_bytes > LDS_MAX) return fail(ctx, MSG_E_UNSUPPORTED, "too large for LDS");
    DevBuf<float> sink;
    Event a, b;
    HIPCHK(ctx, sink.alloc((size_t)blocks));
    HIPCHK(ctx, a.create());
    HIPCHK(ctx, b.create());
    HIPCHK(ctx, launch_fft_bench(po2, blocks, rp.lds_bytes, nullptr, ps.dev.p, pi, 1, sink.p));   // warm-up
    hipEventRecord(a, nullptr);
    HIPCHK(ctx, launch_fft_bench(po2, blocks, rp.lds_bytes, nullptr, ps.dev.p, pi, reps, sink.p));
    hipEventRecord(b, nullptr);
    HIPCHK(ctx, hipEventSynchronize(b));
    hipEventElapsedTime(ms_out, a, b);
    return MSG_OK;
}

int msg_fft64(msg_ctx* ctx, int32_t n, int32_t inverse, const double* in, double* out) {
    if (!ctx || !in || !out || n < 2) return MSG_E_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string why;
    const int pi = real64_plan(ctx->plans64, n, why);
    if (pi < 0) return fail(ctx, MSG_E_DEVICE, why);
    const Real64Plan rp = ctx->plans64.host[pi];
    HIPCHK(ctx, sync_plans(ctx->plans64, nullptr));
    const int K = n / 2 + 1;
    const size_t cnt = (size_t)std::max(n, 2 * K);
    DevBuf<double> io;
    DevBuf<double2> gA, gB;
    HIPCHK(ctx, io.alloc(cnt));
    HIPCHK(ctx, hipMemcpy(io.p, in, (inverse ? 2 * K : n) * sizeof(double), hipMemcpyHostToDevice));
    if (rp.cap > G64_SLOTS) {     // beyond LDS: the engine's global ping-pong mode
        HIPCHK(ctx, gA.alloc((size_t)rp.cap));
        HIPCHK(ctx, gB.alloc((size_t)rp.cap));
    }
    HIPCHK(ctx, launch_fft64_one(rp.cap * 16, nullptr, ctx->plans64.dev.p, pi, inverse ? 1 : 0, io.p, gA.p, gB.p));
    HIPCHK(ctx, hipMemcpy(out, io.p, (inverse ? n : 2 * K) * sizeof(double), hipMemcpyDeviceToHost));
    return MSG_OK;
}

int msg_stft_mag_db(msg_ctx* ctx, const void* x_dev, int32_t elem_bytes, int64_t n, int32_t channels, int32_t win,
                    int32_t hop, int32_t max_frames, double* S_dev, int32_t* frames, void* stream) {
    if (!ctx || !frames || n < 1 || win < 2 || hop < 1 || (channels != 1 && channels != 2) ||
        (elem_bytes != 4 && elem_bytes != 8))
        return fail(ctx, MSG_E_ARG, "bad arguments");
    const int64_t fr = n < win ? 1 : std::min<int64_t>(1 + (n - win) / hop, std::max(max_frames, 0));
    *frames = (int32_t)fr;
    if (!S_dev || fr <= 0) return MSG_OK;                 // size query
    if (!x_dev) return fail(ctx, MSG_E_ARG, "null input");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::string why;
    const int pi = real64_plan(ctx->plans64, win, why);
    if (pi < 0) return fail(ctx, MSG_E_DEVICE, why);
    const int cap = ctx->plans64.host[pi].cap;
    if (cap > G64_SLOTS) return fail(ctx, MSG_E_UNSUPPORTED, "STFT window beyond the LDS float64 engine");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, sync_plans(ctx->plans64, s));
    HIPCHK(ctx, launch_stft64((unsigned)fr, cap * 16, s, ctx->plans64.dev.p, pi, x_dev, elem_bytes, n, channels, win,
                                     hop, S_dev));
    return MSG_OK;
}

int msg_fir(msg_ctx* ctx, const float* x_dev, float* y_dev, int64_t n, int32_t n_signals, const double* h,
            int64_t M, int32_t* fir_shape, void* stream) {
    if (!ctx || !x_dev || !y_dev || !h || n < 1 || n_signals < 1 || M < 1)
        return fail(ctx, MSG_E_ARG, "bad arguments");
    if ((const void*)x_dev == (const void*)y_dev) return fail(ctx, MSG_E_ARG, "x and y must not alias");
    if (M > (int64_t)64 * (FIR_NMAX - 1)) return fail(ctx, MSG_E_UNSUPPORTED, "FIR longer than 64 partitions");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, stream_handover(ctx, s));
    DoneGuard done(ctx, s);
    int N = 0, Pp = 0, Q = 0;
    choose_fir(M, n, N, Pp, Q, ctx->sw.fir8);
    // Many partitions: a frequency-domain delay line (fir_fft.h) computes each
    // input segment's spectrum once and reuses it for Q blocks -- two transforms
    // per block of N/2 outputs instead of Q + 1 per block of N - P + 1, for
    // 8 B/output of spectrum writes and 8 Q B/output of reads.  Measured on
    // MI355X: slower at 64 k taps (classic Q = 5: 7.1 ms vs 7.7 ms per 1024
    // signals), so it takes over only from Q = 8 (>= ~115 k taps).
    // Two partitions of 32 768 taps on the 65 536-point engine (k_fir8q, 32 768
    // < M <= 65 536 beyond the one-partition limit): one forward and one inverse
    // per 32 768 outputs (MSGPU_FIR8Q=0: the choice above, k_fir4 at 64 k taps).
    // Above 35 748 taps the two partitions' 32 768-frame blocks beat one
    // partition's 65 537 - M (a k_fir8q block costs ~1.1 k_fir8p blocks).
    if (ctx->sw.fir8 && ctx->sw.fir8q && ctx->sw.fir8p > 0 && M <= 2 * (int64_t)FIR8Q_P &&
        (double)(FIR8_N + 1 - M) * 1.1 < (double)FIR8Q_P) {
        const int64_t nb = (n + FIR8Q_P - 1) / FIR8Q_P;
        if (nb * n_signals > INT32_MAX) return fail(ctx, MSG_E_UNSUPPORTED, "too many output blocks");
        if (fir_shape) { fir_shape[0] = FIR8_N; fir_shape[1] = FIR8Q_P; fir_shape[2] = 2; }
        // runs of consecutive blocks: about four per CU over the call, whole signals when they suffice
        const int64_t want = 4 * (int64_t)ctx->n_cu;
        const int run_len = (int)std::max<int64_t>(1, std::min<int64_t>(nb, (nb * n_signals + want - 1) / want));
        std::vector<PresetRt> prt;
        std::vector<int2> runs;
        sf_signals(n_signals, n, FIR8_N, FIR8Q_P, (int32_t)nb, FIR8Q_P, nb, run_len, prt, runs);
        const std::vector<float> hf(h, h + M);
        const int64_t K8 = FIR8_HSTRIDE;          // float2 per spectrum (fir8_fft.h layout)
        const int64_t job[8] = {0, FIR8Q_P, 0, 0, FIR8Q_P, M - FIR8Q_P, K8, 0};   // H_0, H_1 from the float taps
        const unsigned grid = (unsigned)std::min<int64_t>((int64_t)runs.size(), ctx->n_cu);
        if (const int rc = sf_upload(ctx, s, prt, runs, job, 8, ctx->sf_hf, hf.data(), M)) return rc;
        HIPCHK(ctx, ctx->sf_hspec.ensure((size_t)(2 * K8)));
        HIPCHK(ctx, ctx->sf_xspec.ensure((size_t)grid * (size_t)fir8q_scratch_per_wg()));
        HIPCHK(ctx, fir8_counters(ctx, s));
        HIPCHK(ctx, launch_fir8_spec32(2, s, ctx->sf_irjobs.p, ctx->d_fir4tab.p, ctx->sf_hf.p, ctx->sf_hspec.p));
        HIPCHK(ctx, launch_fir8q((unsigned)runs.size(), run_len, grid, s, ctx->sf_prt.p, ctx->sf_jobs.p, ctx->d_fir4tab.p,
                                 ctx->sf_hspec.p, x_dev, y_dev, ctx->sf_xspec.p, ctx->fir8_ctr.p));
        HIPCHK(ctx, done.finish());
        return MSG_OK;
    }
    const bool fdl = Q >= 8;
    if (fdl) {
        N = FIR_NMAX;
        Pp = N / 2;
        Q = (int)((M + Pp - 1) / Pp);
    }
    const int64_t B = fdl ? Pp : N - Pp + 1;
    const int64_t blocks = (n + B - 1) / B;
    if (blocks * n_signals > INT32_MAX) return fail(ctx, MSG_E_UNSUPPORTED, "too many output blocks");
    if (fir_shape) { fir_shape[0] = N; fir_shape[1] = Pp; fir_shape[2] = Q; }
    if (N == FIR8_N) {   // one partition on k_fir8: H from the float taps by k_fir8_hpart
        std::vector<PresetRt> prt;
        std::vector<int2> fj;
        sf_signals(n_signals, n, N, Pp, 1, B, blocks, 1, prt, fj);
        for (PresetRt& r : prt) r.h_len = (int32_t)M;
        const std::vector<float> hf(h, h + M);
        const int64_t job[4] = {0, M, 0, 0};      // k_fir8_spec: taps [0, M) -> spectrum at 0
        if (const int rc = sf_upload(ctx, s, prt, fj, job, 4, ctx->sf_hf, hf.data(), M)) return rc;
        HIPCHK(ctx, ctx->sf_hspec.ensure((size_t)FIR8_HSTRIDE));
        HIPCHK(ctx, launch_fir8_spec32(1, s, ctx->sf_irjobs.p, ctx->d_fir4tab.p, ctx->sf_hf.p, ctx->sf_hspec.p));
        if (ctx->sw.fir8p > 0) {   // persistent, as in the render (one workgroup per CU, per-XCD block counters)
            const int nj = (int)fj.size();
            const unsigned grid = (unsigned)std::max(MSG_XCDS, (std::min(nj, ctx->n_cu) / MSG_XCDS) * MSG_XCDS);
            HIPCHK(ctx, fir8_counters(ctx, s));
            HIPCHK(ctx, launch_fir8p((unsigned)nj, grid, s, ctx->sf_prt.p, ctx->sf_jobs.p, ctx->d_fir4tab.p,
                                     ctx->sf_hspec.p, x_dev, y_dev, ctx->fir8_ctr.p, nullptr, nullptr, nullptr,
                                     nullptr));
        } else {
            HIPCHK(ctx, launch_fir8((unsigned)fj.size(), s, ctx->sf_prt.p, ctx->sf_jobs.p, ctx->d_fir4tab.p,
                                    ctx->sf_hspec.p, x_dev, y_dev));
        }
        HIPCHK(ctx, done.finish());
        return MSG_OK;
    }
    std::string why;
    const int fp = real_plan(ctx->fir_plans, N, why);
    if (fp < 0) return fail(ctx, MSG_E_DEVICE, "FIR plan: " + why);
    HIPCHK(ctx, sync_plans(ctx->fir_plans, s));
    const int K = N / 2 + 1;
    // partition spectra H_q = FFT_N(h[qP, qP + P)) by the IR-spectrum kernel
    std::vector<int64_t> jobs;
    for (int q = 0; q < Q; ++q)
        jobs.insert(jobs.end(), {(int64_t)q * Pp, std::min<int64_t>(Pp, M - (int64_t)q * Pp), (int64_t)fp,
                                 (int64_t)q * K});
    std::vector<PresetRt> prt;
    std::vector<int2> fj;
    sf_signals(n_signals, n, N, Pp, Q, B, blocks, 1, prt, fj);
    for (int i = 0; i < n_signals; ++i)
        prt[i].fir_block_begin = (int32_t)(i * blocks);     // FDL: first segment spectrum of this signal
    if (const int rc = sf_upload(ctx, s, prt, fj, jobs.data(), jobs.size(), ctx->sf_h, h, M)) return rc;
    HIPCHK(ctx, ctx->sf_hspec.ensure((size_t)Q * K));
    if (fdl) HIPCHK(ctx, ctx->sf_xspec.ensure((size_t)fj.size() * K));
    HIPCHK(ctx, launch_ir_spec((unsigned)Q, ctx->fir_plans.host[fp].lds_bytes, s, ctx->sf_irjobs.p, Q,
                               ctx->fir_plans.dev.p, ctx->sf_h.p, ctx->sf_hspec.p));
    int ti = 0;
    while ((1024 << ti) != N / 2) ++ti;
    if (fdl)
        HIPCHK(ctx, launch_fdl(N / 2, (unsigned)fj.size(), s, ctx->sf_prt.p, ctx->sf_jobs.p, ctx->d_fir2tab[ti].p,
                               ctx->sf_hspec.p, ctx->sf_xspec.p, x_dev, y_dev));
    else if (N / 2 == 16384 && ctx->sw.fir4)
        HIPCHK(ctx, launch_fir4(N / 2, (unsigned)fj.size(), s, ctx->sf_prt.p, ctx->sf_jobs.p, ctx->d_fir4tab.p,
                                ctx->sf_hspec.p, x_dev, y_dev));
    else
        HIPCHK(ctx, launch_fir2(N / 2, (unsigned)fj.size(), s, ctx->sf_prt.p, ctx->sf_jobs.p, ctx->d_fir2tab[ti].p,
                                ctx->sf_hspec.p, x_dev, y_dev));
    // pageable-host H2D copies are staged before hipMemcpyAsync returns (as in
    // msg_render_batch), so the host vectors may go; the FIR runs asynchronously.
    HIPCHK(ctx, done.finish());
    return MSG_OK;
}

#include "signal_abi.inc"

int msg_last_plan(msg_ctx* ctx, msg_plan_info* info, int32_t n_presets) {
    if (!ctx || !info) return MSG_E_ARG;
    if (n_presets > ctx->last_n) return fail(ctx, MSG_E_ARG, "n_presets exceeds last batch");
    std::memcpy(info, ctx->h_info.data(), sizeof(msg_plan_info) * n_presets);
    return MSG_OK;
}

int msg_last_events(msg_ctx* ctx, int32_t preset, msg_event* events, int32_t cap, int32_t* n) {
    if (!ctx || !n) return MSG_E_ARG;
    if (preset < 0 || preset >= ctx->last_n) return fail(ctx, MSG_E_ARG, "bad preset index");
    const int32_t k = ctx->h_info[preset].n_events;
    *n = k;
    if (!events) return MSG_OK;
    if (k > cap) return fail(ctx, MSG_E_ARG, "event buffer too small");
    std::memcpy(events, ctx->h_events.data() + ctx->h_slot_base[preset], sizeof(msg_event) * k);
    return MSG_OK;
}

int msg_last_meta(msg_ctx* ctx, int32_t preset, double* micro, double* grain, int64_t cap, int64_t* n) {
    if (!ctx || !n) return MSG_E_ARG;
    if (preset < 0 || preset >= ctx->last_n) return fail(ctx, MSG_E_ARG, "bad preset index");
    hipSetDevice(ctx->device);
    const msg_plan_info& inf = ctx->h_info[preset];
    *n = 0;
    if (inf.n_events <= 0) return MSG_OK;
    const msg_event& e = ctx->h_events[ctx->h_slot_base[preset] + inf.n_events - 1];
    if (e.n > cap) return fail(ctx, MSG_E_ARG, "meta buffer too small");
    std::vector<float> tmp(e.n);
    const int64_t off = ctx->h_prt[preset].pool_base + e.pool_off;
    HIPCHK(ctx, wait_last(ctx));
    const int32_t l64 = ctx->h_last64.empty() ? -1 : ctx->h_last64[preset];
    if (l64 >= 0) {   // float64 chain: micro_last / grain_last kept in float64
        const int64_t o64 = ctx->h_ev64[l64].off64;
        if (micro) HIPCHK(ctx, hipMemcpy(micro, ctx->micro64.p + o64, e.n * sizeof(double), hipMemcpyDeviceToHost));
        if (grain) HIPCHK(ctx, hipMemcpy(grain, ctx->grain64.p + o64, e.n * sizeof(double), hipMemcpyDeviceToHost));
        *n = e.n;
        return MSG_OK;
    }
    if (micro) {
        // the generator's grain lies in its owner's slot, a tilted one in the preset's slot behind the pool
        const int64_t moff = ctx->h_micro_last[preset] >= 0 ? ctx->h_micro_last[preset] : off;
        HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->micro.p + moff, e.n * sizeof(float), hipMemcpyDeviceToHost));
        for (int i = 0; i < e.n; ++i) micro[i] = tmp[i];
    }
    if (grain) {
        // the grain lies in its spectral owner's slot (gen_share.h)
        const int64_t goff = ctx->h_grain_off[(size_t)ctx->h_slot_base[preset] + inf.n_events - 1];
        HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->grain.p + goff, e.n * sizeof(float), hipMemcpyDeviceToHost));
        for (int i = 0; i < e.n; ++i) grain[i] = tmp[i];
    }
    *n = e.n;
    return MSG_OK;
}

int msg_last_grain64(msg_ctx* ctx, int32_t preset, int32_t k, double* grain, int64_t cap, int64_t* n) {
    if (!ctx || !n) return MSG_E_ARG;
    if (preset < 0 || preset >= ctx->last_n) return fail(ctx, MSG_E_ARG, "bad preset index");
    const int32_t l64 = ctx->h_last64.empty() ? -1 : ctx->h_last64[preset];
    const int32_t ne = ctx->h_info[preset].n_events;
    if (l64 < 0) return fail(ctx, MSG_E_ARG, "preset is not on the float64 chain");
    if (k < 0 || k >= ne) return fail(ctx, MSG_E_ARG, "bad event index");
    const int64_t at = (int64_t)l64 - (ne - 1) + k;   // the preset's events end at its last float64 record
    if (at < 0 || at >= (int64_t)ctx->h_ev64.size()) return fail(ctx, MSG_E_ARG, "event not on the float64 chain");
    const Ev64& v = ctx->h_ev64[at];
    *n = v.n;
    if (!grain) return MSG_OK;
    if (v.n > cap) return fail(ctx, MSG_E_ARG, "grain buffer too small");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, wait_last(ctx));
    HIPCHK(ctx, hipMemcpy(grain, ctx->grain64.p + v.off64, v.n * sizeof(double), hipMemcpyDeviceToHost));
    return MSG_OK;
}

int msg_last_spec_routes(msg_ctx* ctx, int64_t* counts, int32_t n) {
    if (!ctx || !counts || n < 0) return MSG_E_ARG;
    for (int r = 0; r < n && r < MSG_ROUTE_COUNT; ++r) counts[r] = ctx->h_spec_routes[r];
    return MSG_OK;
}

// The stages are in render_stages.h, in this order.
int msg_render_batch(msg_ctx* ctx, const msg_preset* presets, int32_t P,
                     const double* bp_bank, int64_t bp_pairs, const double* const* irs, const int64_t* ir_lens, int32_t n_irs,
                     const uint8_t* const* images, const int32_t* img_h, const int32_t* img_w,
                     int32_t n_images, float* out_dev, const int64_t* out_offsets, void* stream) {
    if (!ctx || !presets || P <= 0 || !out_dev || !out_offsets) return fail(ctx, MSG_E_ARG, "bad arguments");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, stream_handover(ctx, s));
    DoneGuard done(ctx, s);
    ctx->prof.collect_set(ctx->prof.cur);  // this batch's event set: from two batches back
    Batch b;
    b.presets = presets; b.P = P; b.bp_bank = bp_bank; b.bp_pairs = bp_pairs;
    b.irs = irs; b.ir_lens = ir_lens; b.n_irs = n_irs;
    b.images = images; b.img_h = img_h; b.img_w = img_w; b.n_images = n_images;
    b.out_dev = out_dev; b.out_offsets = out_offsets; b.s = s;
#define STAGE(f) do { if (const int rc_ = f(ctx, b)) return rc_; } while (0)
    STAGE(stage_check);
    ctx->prof.batch = ctx->prof.on && (ctx->prof.n++ % ctx->prof.every) == 0;
    stage_mark(ctx, 0, s);
    // ---- host: plan, records, one upload
    b.h0 = Batch::hclock::now();
    STAGE(stage_plan);
    STAGE(stage_tap_merge);
    stage_mark(ctx, 1, s);
    b.h1 = Batch::hclock::now();
    STAGE(stage_preset_records);
    b.hB = Batch::hclock::now();
    STAGE(stage_event_records);
    b.hC = Batch::hclock::now();
    STAGE(stage_lists);
    STAGE(stage_buffers);
    STAGE(stage_upload);                   // takes h2 between its last add and the flush
    host_clocks(ctx, b);
    // ---- device: every launch of the batch
    if (b.fir.h_early) {
        stage_mark(ctx, 10, s);
        STAGE(enqueue_h_spectra);
        stage_mark(ctx, 11, s);
    }
    stage_mark(ctx, 2, s);
    STAGE(enqueue_generate);
    stage_mark(ctx, 3, s);
    STAGE(enqueue_spectral);
    stage_mark(ctx, 4, s);
    STAGE(enqueue_ola);
    stage_mark(ctx, 5, s);
    STAGE(enqueue_fir);                    // marks 8 and 9 around the FIR kernels
    stage_mark(ctx, 6, s);
    STAGE(enqueue_stereo);
    stage_mark(ctx, 7, s);
#undef STAGE
    HIPCHK(ctx, done.finish());
    keep_mirrors(ctx, b);
    if (ctx->prof.batch) {
        ctx->prof.pending[ctx->prof.cur] = true;
        ctx->prof.pending_fir[ctx->prof.cur] = b.fir.hblocks > 0;
        ctx->prof.pending_h_early[ctx->prof.cur] = b.fir.h_early;
        ctx->prof.cur ^= 1;
    }
    return MSG_OK;
}

}  // extern "C"
