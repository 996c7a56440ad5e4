// ctx.h — msg_ctx, the context behind the C ABI, and the types it is made of.
// Part of msgpu.hip (the runtime records, the plan structs and the launch
// constants are in scope there); not a stand-alone header.
#pragma once
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "dev_own.h"
#include "host_pool.h"

namespace {

std::mutex g_gate_mu;              // msg_gate links between contexts

// Pinned staging for a batch's host -> device uploads.  Every per-batch input
// (presets, events, runtime records, job lists, IR bank ...) is packed into one
// pinned slot and moved by ONE copy into a device arena; each input's device
// pointer is then set to its place in the arena.  (One copy per input cost ~35
// copy-engine blits per batch, ~2 ms of GPU time per C3 sub-batch.)  Two pinned
// slots alternate between batches; a slot is refilled only after the copy that
// read it (two batches back) has run, so msg_render_batch never waits on the
// render stream.  The arena itself is reused in stream order.
struct Staging {
    struct Item { void** slot; const void* src; size_t bytes; };
    struct Slot { PinnedBuf host; Event done; bool armed = false; };
    Slot slot[2];
    int cur = 0;
    DevBuf<char> arena;
    std::vector<Item> items;
    template <class T> void add(T** dst, const T* src, size_t bytes) {
        items.push_back(Item{reinterpret_cast<void**>(dst), src, bytes});
    }
    hipError_t flush(hipStream_t s) {
        Slot& sl = slot[cur];
        hipError_t e = hipSuccess;
        if (!sl.done) e = sl.done.create(hipEventDisableTiming);
        if (e == hipSuccess && sl.armed) e = hipEventSynchronize(sl.done);
        std::vector<size_t> at(items.size());
        size_t total = 0;
        for (size_t i = 0; i < items.size(); ++i) {
            at[i] = total;
            total += (items[i].bytes + 255) & ~size_t(255);
        }
        total = std::max<size_t>(total, 256);
        if (e == hipSuccess && total > sl.host.cap) e = sl.host.alloc(total + total / 4 + 4096);
        // growth frees the old arena first (the free waits for the work that reads it)
        if (e == hipSuccess && total > arena.cap) e = arena.alloc(total + total / 4 + 4096);
        if (e == hipSuccess) {   // pack in 1 MiB pieces on the host pool (C5: ~100 MB per sub-batch)
            constexpr size_t PIECE = size_t(1) << 20;
            std::vector<std::pair<size_t, size_t>> pieces;   // (item, byte offset in item)
            for (size_t i = 0; i < items.size(); ++i)
                for (size_t b = 0; b < items[i].bytes; b += PIECE) pieces.emplace_back(i, b);
            HostPool::get().run((int)pieces.size(), [&](int k) {
                const Item& it = items[pieces[k].first];
                const size_t b = pieces[k].second;
                std::memcpy(sl.host.p + at[pieces[k].first] + b, (const char*)it.src + b, std::min(PIECE, it.bytes - b));
            });
            size_t used = 0;
            for (size_t i = 0; i < items.size(); ++i) used = at[i] + items[i].bytes;
            if (used) e = hipMemcpyAsync(arena.p, sl.host.p, used, hipMemcpyHostToDevice, s);
        }
        for (size_t i = 0; i < items.size(); ++i) *items[i].slot = e == hipSuccess ? arena.p + at[i] : nullptr;
        if (e == hipSuccess) e = hipEventRecord(sl.done, s);
        sl.armed = e == hipSuccess;
        items.clear();
        cur ^= 1;
        return e;
    }
};

// A per-batch input living in the Staging arena (set at each flush).
template <class T> struct Slice { T* p = nullptr; };

// FFT plans by length: the descriptors (P, device pointers inside), the
// tables those point to (S: their scalar type) and the descriptors' device copy.
template <class P, class S>
struct PlanStoreT {
    std::vector<P> host;
    std::vector<DevBuf<S>> allocs;
    std::map<int, int> by_n;
    bool dirty = false;
    DevBuf<P> dev;
};
using PlanStore = PlanStoreT<RealPlan, float>;
using Plan64Store = PlanStoreT<Real64Plan, double>;

// Runtime switches, read from the environment once per context.
struct Switches {
    bool device_plan = false;     // MSGPU_DEVICE_PLAN=1: plan on the device (k_plan_*), read back
    bool fir4 = true;            // M = 16384 blocks on k_fir4 (MSGPU_FIR4=0: k_fir2, A/B and tests)
    // one-partition k_fir4 spectra from the taps (k_fir4_hconv; MSGPU_FIR4C=0: k_h_build + k_fir4_hpart)
    bool fir4c = true;
    bool fir8 = true;            // N = 65536 one-partition filters on k_fir8 (MSGPU_FIR8=0: off, A/B and tests)
    int fir64 = 1;               // float64 FIR of saturated renders: 0 off, 1 predicted, 2 every FIR preset (MSGPU_FIR64)
    int fir64_cap = FIR64_CAP;   // float64 FIR slots per window (MSGPU_FIR64_CAP: tests force several windows)
    // k_fir8 blocks (MSGPU_FIR8P): 0 one workgroup per block, 1 persistent workgroups
    // (one per CU, per-XCD block counters; C3 isolated FIR 2.03 -> 1.86 ms, C5 131.6
    // -> 125.9 ms per step, profiles/r04r_ab.json)
    int fir8p = 1;
    bool fir8q = true;           // msg_fir: 32 k < M <= 64 k taps as two partitions on k_fir8q (MSGPU_FIR8Q=0: off)
    int fir8p_cus = 0;           // persistent FIR workgroups (MSGPU_FIR8P_CUS, A/B; 0: one per CU)
    // overlap-add inside k_fir8p's loads (PresetRt::ola_fir) for batches whose k_fir8p
    // presets' grains total at most ola_fir_density x their frames (MSGPU_OLA_FIR=0: never)
    bool ola_fir = true;
    double ola_fir_density = 1.25;
    // filter spectra before the generator (MSGPU_H_EARLY): 0 at the FIR stage, 1 always,
    // 2 (default) for batches with an output of at least 2^22 frames, whose FIR
    // holds every CU for milliseconds (C5 -2.5 %); shorter ones lose by it (C3 +2 %)
    int h_early = 2;
    bool er_dev = true;          // ER gains drawn on the device (k_er_gains; MSGPU_ER_DEV=0: on the host plan)
    int so_row = 0, so_col = 0;  // odd-stereo transform-split limits (MSGPU_SO_ROW / _COL, tests; 0 = default)
    // each distinct generator grain once per batch (gen_share.h); MSGPU_GEN_SHARE=0: every
    // event generates its own (the bit-identity tests and the A/B)
    bool gen_share = true;
    // the float32 spectral chain once per distinct spectral key (gen_share.h, specshare);
    // MSGPU_SPEC_SHARE=0: every event runs it.  MSGPU_GEN_SHARE=0 implies it: no micro grain is shared
    bool spec_share = true;

    static Switches from_env() {
        Switches w;
        if (const char* e = getenv("MSGPU_DEVICE_PLAN")) w.device_plan = e[0] == '1';
        if (const char* e = getenv("MSGPU_FIR4")) w.fir4 = e[0] != '0';
        if (const char* e = getenv("MSGPU_FIR4C")) w.fir4c = e[0] != '0';
        if (const char* e = getenv("MSGPU_FIR8")) w.fir8 = e[0] != '0';
        if (const char* e = getenv("MSGPU_FIR64")) w.fir64 = atoi(e);
        if (const char* e = getenv("MSGPU_FIR64_CAP")) w.fir64_cap = std::max(1, std::min(FIR64_CAP, atoi(e)));
        if (const char* e = getenv("MSGPU_FIR8P")) w.fir8p = atoi(e);
        if (const char* e = getenv("MSGPU_FIR8Q")) w.fir8q = e[0] != '0';
        if (const char* e = getenv("MSGPU_FIR8P_CUS")) w.fir8p_cus = std::max(0, atoi(e));
        if (const char* e = getenv("MSGPU_OLA_FIR")) w.ola_fir = e[0] != '0';
        if (const char* e = getenv("MSGPU_OLA_FIR_DENSITY")) w.ola_fir_density = atof(e);
        if (const char* e = getenv("MSGPU_H_EARLY")) w.h_early = atoi(e);
        if (const char* e = getenv("MSGPU_ER_DEV")) w.er_dev = e[0] != '0';
        if (const char* e = getenv("MSGPU_SO_ROW")) w.so_row = atoi(e);
        if (const char* e = getenv("MSGPU_SO_COL")) w.so_col = atoi(e);
        if (const char* e = getenv("MSGPU_GEN_SHARE")) w.gen_share = e[0] != '0';
        if (const char* e = getenv("MSGPU_SPEC_SHARE")) w.spec_share = e[0] != '0';
        if (!w.gen_share) w.spec_share = false;        return w;
    }
};

// msg_gate: this context's stream waits, before stage `wait`, for the peer's
// gate event, and records its own after stage `rec` begins (peer / gated_by
// change under g_gate_mu: msg_gate, ~msg_ctx).
struct Gate {
    msg_ctx* peer = nullptr;
    std::vector<msg_ctx*> gated_by;   // contexts whose peer is this one (unlinked by ~msg_ctx)
    int wait = -1, rec = -1;
    Event ev;
    std::atomic<bool> armed{false};   // ev recorded at least once (read by the gated context)
};

// Stage profiling.  Two event sets alternate between batches; a set is read
// (folded into the sums) when it comes round again, two batches later, or at
// msg_stage_times -- profiling never makes the host wait for the last batch.
struct Prof {
    bool on = false;
    // msg_set_profiling(ctx, k): batches 0, k, 2k, ... of the context record the
    // stage events and host clocks (k = 1: every batch).  Each profiled batch
    // adds 12 timed events to its stream and a host read of the set two batches
    // back (bench.py samples every 4th batch)
    int every = 1;
    int64_t n = 0;
    bool batch = false;           // this batch records (on && its turn)
    Event ev[2][12];
    int cur = 0;
    bool pending[2] = {false, false};
    bool pending_fir[2] = {false, false};
    bool pending_h_early[2] = {false, false};
    double stage_sum[10] = {0};   // accumulated stage times since msg_set_profiling(ctx, 1)
    int64_t stage_cnt = 0;
    // host wall clock per batch: plan, records, pinned upload, then the splits
    // plan sizes, plan events + tap merge, preset records, event records, lists + buffers
    double host_sum[8] = {0};
    double ola_fir_sum = 0.0;    // presets whose overlap-add ran inside k_fir8p, summed over profiled batches
    // float32-chain events and the grains k_gen_normal generated for them (gen_share.h),
    // summed over profiled batches
    double gen_events_sum = 0.0, gen_grains_sum = 0.0;
    double spec_runs_sum = 0.0;  // float32-chain events that ran a spectral kernel (specshare)
    int64_t host_cnt = 0;

    hipError_t create_events() {
        for (auto& set : ev)
            for (Event& e : set)
                if (const hipError_t err = e.create()) return err;
        return hipSuccess;
    }
    // Fold the event times of set k's profiled batch into the running sums.
    // The events are read lazily (at the next batch of the same context that
    // uses the set, or at msg_stage_times) so profiling never blocks the host
    // between batches.
    void collect_set(int k) {
        if (!pending[k]) return;
        Event* e = ev[k];
        hipEventSynchronize(e[7]);
        float ms[10] = {0};
        for (int i = 0; i < 7; ++i) hipEventElapsedTime(&ms[i], e[i], e[i + 1]);
        hipEventElapsedTime(&ms[7], e[0], e[7]);
        if (pending_fir[k]) {   // the FIR kernel alone, and the filter spectra
            hipEventElapsedTime(&ms[8], e[8], e[9]);
            if (pending_h_early[k]) {   // launched before the generator: out of host_prep
                hipEventElapsedTime(&ms[9], e[10], e[11]);
                hipEventElapsedTime(&ms[1], e[1], e[10]);
            } else {
                hipEventElapsedTime(&ms[9], e[5], e[8]);
            }
        }
        for (int i = 0; i < 10; ++i) stage_sum[i] += ms[i];
        ++stage_cnt;
        pending[k] = false;
    }
    // all sets (msg_stage_times / msg_set_profiling): waits for the profiled batches
    void collect() {
        collect_set(cur ^ 1);
        collect_set(cur);
    }
    void reset_sums() {
        for (double& v : stage_sum) v = 0.0;
        for (double& v : host_sum) v = 0.0;
        ola_fir_sum = 0.0;
        gen_events_sum = gen_grains_sum = spec_runs_sum = 0.0;
        stage_cnt = 0;
        host_cnt = 0;
    }
};

}  // namespace

// Every device buffer, pinned buffer and event below is an owner from
// dev_own.h (alone, or inside Staging, PlanStoreT, Gate, Prof or the so_bp
// map), so a new one needs no line anywhere else: ~msg_ctx waits for the
// device and unlinks the gate, then the members free themselves.
struct msg_ctx {
    int device = 0;
    std::string err;
    Switches sw;
    Gate gate;
    Prof prof;
    // the stream of the last batch and an event at its end: a batch enqueued on
    // another stream first waits for it (the staging arena and the per-batch
    // buffers are reused in stream order only)
    hipStream_t last_stream = nullptr;
    Event done_ev;
    bool done_armed = false;
    int n_cu = 256;               // compute units (persistent grids)
    Staging staging;              // pinned uploads of a batch
    // constant tables, uploaded once by msg_create
    DevBuf<uint64_t> d_ki, d_ke;  // ziggurat tables (dzig points into these six)
    DevBuf<double> d_wi, d_fi, d_we, d_fe;
    nprng::Zig dzig{};
    DevBuf<JumpTab> d_jump;
    DevBuf<float2> d_fir2tab[5];  // k_fir2 twiddle tables, M = 1024 << i
    DevBuf<float2> d_fir4tab;     // k_fir4 twiddle tables (M = 16384)
    DevBuf<float2> d_spec_ct_tab[SPEC_CT_PLANS];   // compile-time spectral plans (spec_ct.h)
    DevBuf<float2> d_spec3_tab;                    // band-pruned spectral kernel (spec3.h)
    Slice<int32_t> spec3_list;
    PlanStore grain_plans, fir_plans;
    // per-batch buffers
    // device planner (MSGPU_DEVICE_PLAN=1)
    DevBuf<msg_preset> dp_presets;
    DevBuf<double> dp_bp;                                 // breakpoint bank (device planner)
    DevBuf<int64_t> frag_len;
    DevBuf<msg_plan_info> info;
    DevBuf<int32_t> slot_base, tap_base;
    DevBuf<msg_event> dp_events;
    DevBuf<int32_t> dp_er_off;
    DevBuf<double> dp_er_gain;
    // per-batch inputs, uploaded in one copy (Staging arena)
    Slice<msg_preset> presets;
    Slice<msg_event> events;
    Slice<int32_t> er_off;
    Slice<double> er_gain;
    Slice<int32_t> er_key, er_first, er_cnt;
    DevBuf<double> er_gain_d;           // k_er_gains' output (host batch path)
    DevBuf<double> er_tap_d;            // k_er_gains' per-tap gains
    Slice<EventRt> ert;
    Slice<int64_t> grain_off;           // per event slot: the grain the overlap-add reads (specshare)
    Slice<PresetRt> prt;
    Slice<int32_t> gen_list, spec_small, spec_big, tile_begin, fir_begin, h_begin, st_begin, fir_plan_of;
    DevBuf<float> micro, grain, mono_a, mono_y;
    DevBuf<float2> hspec;
    DevBuf<float> hscratch;                     // h of every FIR preset (k_h_build -> k_fir_h / k_fir4_hpart)
    Slice<int32_t> h_tile_begin, fir8_list, fir_lo;
    Slice<int64_t> ir8_jobs;
    Slice<int32_t> fir4c_list;                  // k_fir4_hconv presets (one partition at N = 32768)
    Slice<int64_t> ir4_jobs;                    // k_fir4_irspec jobs
    Slice<int2> hpart_jobs;
    Slice<int2> fir_jobs;
    Slice<int32_t> spec_ct_list;
    Slice<double> irbank;
    Slice<unsigned> maxbits;            // per preset: k_stereo_max's peak bits, zeroed by the batch's upload
    std::vector<unsigned> maxbits_zero;
    // float64 space FIR of saturated renders (kernels_fir64.h)
    Slice<Fir64Rt> f64rt;
    Slice<int32_t> st_count, odd_list, odd_cnt;
    DevBuf<double> f64_stats;                   // per preset: sum y^2, sum (1 + (d y)^2)^-2
    DevBuf<int32_t> f64_flag, f64_slot_preset, f64_nslots;
    DevBuf<double> st_part;             // stereo pass (kernels_stereo.h): per-tile partial sums
    DevBuf<int32_t> fir8_ctr;           // k_fir8p's per-XCD block counters
    DevBuf<float> f64_h;
    DevBuf<double2> f64_hs;
    // float64 grain chain (kernels_grain64.h)
    Plan64Store plans64;
    Slice<Ev64> ev64;
    Slice<int32_t> g64_list, gen64_list;
    Slice<int64_t> gen64_off;
    DevBuf<double> micro64, grain64, state64;
    DevBuf<double2> save64;
    Slice<Chain64> chains;
    Slice<uint8_t> imgbank;
    DevBuf<double2> g64A, g64B;                 // global-class float64 grains (G64Global)
    DevBuf<uint32_t> g64mask;
    // standalone FIR (msg_fir): its own buffers, so it never touches a render batch's
    DevBuf<PresetRt> sf_prt;
    DevBuf<int2> sf_jobs;
    DevBuf<int64_t> sf_irjobs;
    DevBuf<double> sf_h;
    DevBuf<float2> sf_hspec, sf_xspec;
    DevBuf<float> sf_hf;                        // float taps of a k_fir8 filter
    // msg_digest: render extents + tile bases, per-tile partials
    DevBuf<int64_t> dg_meta;
    DevBuf<char> dg_part;
    // msg_resample: signal extents + tile bases, the tap table
    DevBuf<int64_t> rs_meta;
    DevBuf<float> rs_tab;
    // msg_loudness / msg_loudness_gain: signal extents + tile bases, the rate's table
    // (loudness.h), per-tile filter states, per-tile energy and peak
    DevBuf<int64_t> ld_meta;
    DevBuf<double> ld_tab, ld_state, ld_part;
    // msg_loudness_range: the hop sums when the caller takes none, one double per short-term window
    DevBuf<double> lr_hops, lr_win;
    // msg_truepeak / msg_truepeak_gain: the interpolator's taps (truepeak.h, uploaded once
    // by msg_create), signal extents + tile bases, per-tile maxima
    DevBuf<float> d_tp_tab;
    DevBuf<int64_t> tp_meta;
    DevBuf<uint2> tp_part;
    // odd-length stereo rotation (kernels_stereo_odd.h)
    std::map<int64_t, DevBuf<double2>> so_bp;  // chirp kernel spectra by n (float64), LRU-bounded
    std::map<int64_t, uint64_t> so_bp_use;     // batch serial of each entry's last use
    uint64_t batch_serial = 0;
    DevBuf<double2> so_A;
    DevBuf<float> so_r2;
    // host mirrors of the last batch
    std::vector<msg_plan_info> h_info;
    std::vector<msg_event> h_events;
    std::unique_ptr<EventRt[]> h_ert;   // host EventRt records (grow-only, msg_render_batch)
    size_t h_ert_cap = 0;
    std::vector<int32_t> h_er_off;
    std::vector<double> h_er_gain;
    // the host batch path's merged ER taps: per live slot its first key and
    // key count, the keys' tap indices (k_er_gains draws the gains on the device)
    std::vector<int32_t> h_er_key, h_er_first, h_er_cnt;
    std::vector<PresetRt> h_prt;
    std::vector<int32_t> h_slot_base;
    std::vector<Ev64> h_ev64;
    std::vector<int32_t> h_last64;      // per preset: Ev64 index of its last event, -1 = float32 chain
    std::vector<int64_t> h_micro_last;  // per float32-chain preset: its last event's micro_last in the micro pool
    // generator sharing (gen_share.h): each event slot's owner and the lookup's buffers, kept between batches
    std::vector<int32_t> h_gen_owner;
    genshare::Scratch gen_scratch;
    // spectral sharing (gen_share.h, specshare): each float32-chain slot's spectral owner and
    // kernel route, and per event slot the absolute float offset of the grain its readers
    // take (the owner's slot; a float64-chain event's own), uploaded as grain_off
    std::vector<int32_t> h_spec_owner;
    std::vector<int8_t> h_spec_route;
    std::vector<int64_t> h_grain_off;
    specshare::Scratch spec_scratch;
    int64_t h_spec_routes[MSG_ROUTE_COUNT] = {0};   // msg_last_spec_routes: spectral runs per kernel route
    int32_t last_n = 0;
    // msg_quantize: signal extents, tile bases, stream keys and output offsets; per-tile partials
    DevBuf<int64_t> pcm_meta;
    DevBuf<int4> pcm_part;
    // msg_quantize_shaped: the same rows; its lanes write the records themselves
    DevBuf<int64_t> pcm_shape_meta;
    // msg_limit: signal extents, both kernels' tile bases and the scratch offsets; the smoothing
    // weights; r of every frame; per envelope tile the NaN flag; per signal the state; per apply
    // tile the least gain and the count
    DevBuf<int64_t> lim_meta;
    DevBuf<float> lim_w, lim_r;
    DevBuf<uint32_t> lim_nan;
    DevBuf<int32_t> lim_state;
    DevBuf<uint2> lim_part;
    // msg_edges: signal extents and both kernels' tile bases (the records are the caller's)
    DevBuf<int64_t> edg_meta;
    // msg_filter: signal extents + tile bases, the cascade's table (filter.h), per-tile states
    DevBuf<int64_t> fl_meta;
    DevBuf<double> fl_tab, fl_state;
    // msg_stereo_meter / msg_stereo: signal extents + tile bases (+ the fold's output offsets), per-tile sums
    DevBuf<int64_t> img_meta;
    DevBuf<double> img_part;
    // msg_dynamics: signal extents + tile bases; per tile the two summaries and the two carries; per
    // tile the non-finite flag; per signal the state; with a hold, per tile the demands of the
    // hold_frames before it
    DevBuf<int64_t> dyn_meta, dyn_carry, dyn_halo;
    DevBuf<uint32_t> dyn_flag;
    DevBuf<int32_t> dyn_state;
    // msg_gate_apply: signal extents + tile bases; per tile the two summaries and the two carries; per
    // tile its transfer (3 words) and the age that enters it; per tile the non-finite flag; per signal
    // the state
    DevBuf<int64_t> gate_meta, gate_carry, gate_trans;
    DevBuf<uint32_t> gate_flag;
    DevBuf<int32_t> gate_state;
    // msg_flac: signal extents + block bases; per block its plan (21 words) and the bytes in front of its frame
    DevBuf<int64_t> flac_meta, flac_plan, flac_pre;

    // What must come first and in this order; the members' destructors follow.
    ~msg_ctx() {
        hipSetDevice(device);
        hipDeviceSynchronize();
        std::lock_guard<std::mutex> lk(g_gate_mu);
        for (msg_ctx* c : gate.gated_by) { c->gate.peer = nullptr; c->gate.wait = c->gate.rec = -1; }
        if (gate.peer) {
            auto& v = gate.peer->gate.gated_by;
            v.erase(std::remove(v.begin(), v.end(), this), v.end());
        }
    }
};
