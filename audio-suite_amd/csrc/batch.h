// batch.h — host: the state of one msg_render_batch call, grouped by the
// pipeline stage that fills it.  The stage functions in msgpu.hip
// take (msg_ctx*, Batch&); everything the batch's one upload registers lives
// here or in the context, so it outlives the flush.
#pragma once
#include <chrono>
#include <map>
#include <vector>
#include "rt.h"
#include "gen_share.h"
#include "launch.h"
#include "../../include/msgpu.h"

namespace {

// The IR spectra of the one-partition presets at one transform size (N = 65536
// on k_fir8, N = 32768 on k_fir4): each IR of the batch is transformed once.
// Offsets count from the bank's start until relocate() moves the bank behind
// the per-preset spectra in hspec.
struct IrBank {
    std::map<int, int64_t> spec_of;   // IR index -> spectrum offset
    std::vector<int64_t> jobs;        // spectrum jobs: [ir_off, len, spec_off, 0]
    int64_t sum = 0;
    std::vector<int32_t> er_list;     // ER presets: H = rfft(delta + ER taps) . S_IR (k_fir8_hconv / k_fir4_hconv)
    std::vector<int32_t> ir_only;     // IR-only presets: H = the IR's spectrum itself
    int64_t slot(int ir_index, int64_t ir_off, int32_t ir_len, int N) {
        auto it = spec_of.find(ir_index);
        if (it == spec_of.end()) {
            it = spec_of.emplace(ir_index, sum).first;
            jobs.insert(jobs.end(), {ir_off, (int64_t)ir_len, sum, 0});
            sum += (N / 2 + 1 + 15) & ~15;
        }
        return it->second;
    }
    void relocate(std::vector<PresetRt>& prt, int64_t base) {
        for (int p : er_list)
            if (prt[p].ir_len > 0) prt[p].irs_off += base;
        for (int p : ir_only) prt[p].h_off += base;
        for (size_t j = 0; j < jobs.size(); j += 4) jobs[j + 2] += base;
    }
};

struct Batch {
    using hclock = std::chrono::steady_clock;
    // ---- the call's arguments
    const msg_preset* presets = nullptr;
    int P = 0;
    const double* bp_bank = nullptr;
    int64_t bp_pairs = 0;
    const double* const* irs = nullptr;
    const int64_t* ir_lens = nullptr;
    int n_irs = 0;
    const uint8_t* const* images = nullptr;
    const int32_t* img_h = nullptr;
    const int32_t* img_w = nullptr;
    int n_images = 0;
    float* out_dev = nullptr;
    const int64_t* out_offsets = nullptr;
    hipStream_t s = nullptr;
    // host clocks at the stage boundaries (msg_ctx::host_sum)
    hclock::time_point h0, hA, h1, hB, hC, h2;

    // ---- plan and tap merge
    std::vector<int64_t> flen;                  // per preset: its fragment IR's length
    std::vector<msg_plan_info> info;
    std::vector<int32_t> slot_base, tap_base;
    int64_t nslots = 0, ntaps = 0;
    std::vector<int32_t> n_taps_live, tap_max;  // merged in-range taps per preset, their largest offset
    bool er_dev = false;                        // the ER gains are drawn on the device (host plan && MSGPU_ER_DEV)

    // ---- preset records
    std::vector<PresetRt> prt;
    EventRt* ert = nullptr;                     // msg_ctx::h_ert
    std::vector<double> irbank;
    std::vector<int64_t> ir_off;
    std::vector<uint8_t> imgbank;
    std::vector<int64_t> img_off;
    int64_t pool = 0, ysum = 0;                 // running sums: grain pool, mono frames
    int32_t tiles = 0, stiles = 0;              // k_ola_env tiles, stereo tiles
    std::vector<int32_t> tile_begin, st_begin, st_count;
    std::vector<int32_t> odd_presets;           // odd-length stereo rotation (kernels_stereo_odd.h)
    int32_t n_odd = 0;
    int64_t r2_sum = 0, so_M = 0;
    bool use_ct = true, use_s3 = true, stop_cep = false;   // MSGPU_SPEC_CT / MSGPU_SPEC3 / MSGPU_G64_STOP

    struct FirPick { int64_t M; int N, P, Q; float bess[25]; };
    struct Fir {                                // space FIR and spectrum layout
        std::vector<FirPick> pick;              // per preset: taps, partitioning, stereo Bessel taps
        bool batch_ola = false;                 // the overlap-add runs inside k_fir8p for this batch
        int n_ola = 0;                          // presets with PresetRt::ola_fir
        int64_t ola_nmax = 0;                   // their longest output
        std::vector<int32_t> fir_begin, h_begin, fir_plan_of;
        std::vector<int32_t> h_tile_begin;      // k_h_build tiles per preset (prefix)
        int32_t fblocks = 0, hblocks = 0, htiles = 0;
        int32_t hblocks_gen = 0;                // k_fir_h blocks of presets not on the k_fir4 engine
        int64_t hsum = 0, hs_sum = 0;           // float2 of per-preset spectra, floats of time-domain h
        int lds = 0;                            // k_fir_h's LDS bytes
        std::vector<int2> hpart_jobs;           // (preset, q) of the presets on the k_fir4 engine
        std::vector<int2> jobs_by[6];           // FIR output blocks per transform size; [5]: k_fir8
        std::vector<int2> jobs;                 // jobs_by concatenated, [job_off[i], job_off[i + 1]) per size
        int32_t job_off[7] = {0};
        std::vector<int32_t> lo;                // k_fir8p<true>: each block's first event
        IrBank ir8, ir4;                        // N = 65536 (k_fir8), N = 32768 (k_fir4, MSGPU_FIR4C)
        bool h_early = false;                   // filter spectra before the generator
    } fir;

    struct G64 {                                // float64 grain chain (kernels_grain64.h)
        std::vector<Ev64> ev;
        std::vector<int32_t> gen_list;          // normal-driven float64 events (event slots)
        std::vector<int64_t> gen_off;           // their raw-normal offsets in micro64
        std::vector<Chain64> chains, chains_glb;   // chains: LDS class first, the global class appended
        size_t n_lds_chains = 0;
        std::vector<int32_t> last;              // per preset: Ev64 index of its last event, -1 = float32 chain
        int64_t sum = 0, save_sum = 0, state_sum = 0;
        int cap = 0;                            // LDS slots of the LDS-class grains
        int64_t big_cap = 0;                    // slot size of the global-class grains
        std::vector<int32_t> lds, glb, list;    // Ev64 indices by class; list = lds + glb
        G64Global gg{};
        unsigned g_grid = 0, c_grid = 0;
    } g64;

    struct F32 {                                // float32-chain event lists
        std::vector<int32_t> presets;           // presets on the float32 chain
        // each preset's lists before they are concatenated.  Freed with the Batch, after the
        // launches: freeing these ~10 P vectors inside the stage put their cost ahead of the
        // upload (host_event_records 0.15 -> 0.22 ms per C3 sub-batch)
        struct Lists { std::vector<int32_t> gen, s3, ct[SPEC_CT_PLANS], small, pending; };
        std::vector<Lists> per_preset;
        // the lists hold owners only: gen_list the generator owners, the others the events
        // that run a spectral kernel (gen_share.h)
        std::vector<int32_t> gen_list, spec_small, spec_big, spec3;
        std::vector<int32_t> ct[SPEC_CT_PLANS]; // events of the compile-time spectral plans
        std::vector<int32_t> ct_list;           // ct concatenated
        int32_t ct_off[SPEC_CT_PLANS + 1] = {0};
        int small_lds = 0, big_lds = 0;
        // generator sharing (gen_share.h): float32-chain events, the owners among them
        // (gen_list holds the owners only), the floats of the micro_last slots behind the
        // micro pool, and per preset the offset msg_last_meta reads micro_last from
        int64_t n_events = 0, n_owners = 0;
        int64_t n_spec_runs = 0;                // events on a spectral list (specshare)
        int64_t n_copy = 0;                     // those of spec_small without a spectral stage (copies)
        int64_t mlast_sum = 0;
        std::vector<int64_t> micro_last;
    } f32;

    struct Fir64 {                              // float64 FIR of saturated renders (kernels_fir64.h)
        std::vector<Fir64Rt> rt;
        int cand = 0, qmax = 0, bmax = 0, stmax = 0;
        int64_t hmax = 0;
        int plan = -1;
        bool on = false;
        int64_t hstride = 0, hsstride = 0;
        int cap = 1;                            // slots per window
    } f64;

    // ---- enqueue
    float* yb = nullptr;                        // the mono signal the stereo stage reads
};

}  // namespace
