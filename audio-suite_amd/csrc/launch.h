// launch.h — host-side launchers of the kernels compiled in their own
// translation units (k_spectral.hip, k_fir.hip), so the FFT-heavy kernels
// build in parallel.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "rt.h"
#include "fft64.h"
#include "resample.h"

constexpr int LDS_MAX = 163840;                              // 160 KiB per CU
constexpr int SPEC_T_BIG = 512, SPEC_M_BIG = 20480;           // up to 160 KiB LDS
constexpr int SPEC_T_SMALL = 256, SPEC_M_SMALL = 8192;        // up to 64 KiB LDS
constexpr int SPEC_SMALL_BYTES = 65536;
constexpr int FIR_T = 512, FIR_M = 16384;                     // N <= 32768 real
constexpr int FIR_NMAX = 32768;

void spectral_init_attrs();
hipError_t launch_spectral(bool big, unsigned grid, int lds_bytes, hipStream_t s,
                           const msg_preset* presets, const msg_event* events, const EventRt* ert,
                           const PresetRt* rt, const RealPlan* plans, const int32_t* ev_list, int n_list,
                           float* micro_pool, float* grain_pool);

// compile-time-plan spectral kernels for hot grain lengths (spec_ct.h)
constexpr int SPEC_CT_PLANS = 6;
void spectral_ct_init_attrs();
int spectral_ct_plan(int n);
bool spectral_ct_tables(int plan, std::vector<float>& out);
hipError_t launch_spectral_ct(int plan, unsigned grid, hipStream_t s, const msg_event* events, const EventRt* ert,
                              const PresetRt* rt, const float2* tables, const int32_t* ev_list, int n_list,
                              float* micro_pool, float* grain_pool);

// band-pruned register-resident spectral kernel for the 30 MHz hot length (spec3.h)
void spec3_init_attrs();
bool spec3_tables(std::vector<float>& out);
bool spec3_eligible(int n, int ops, int gen_sr, double cutoff_gen, double roll, double stretch, int64_t float_off,
                    int32_t* kb, int32_t* kz, int32_t* ky, double* inv_f, int32_t* exact32);
hipError_t launch_spec3(unsigned grid, hipStream_t s, const msg_event* events, const EventRt* ert, const PresetRt* rt,
                        const float2* tables, const int32_t* ev_list, int n_list, const float* micro_pool,
                        float* grain_pool);

void fir_init_attrs();
// the float64 space FIR of heavily saturated renders (kernels_fir64.h): flag, h, H_q, blocks
struct Fir64Launch {
    const PresetRt* rt; int n_presets; const int32_t* flag64; unsigned* maxbits;
    int32_t* slot_preset; int32_t* n_slots;
    int n_cand;   // FIR presets of the batch (the most slots there can be)
    int cap;      // slots per window (their h and H_q buffers)
    const Fir64Rt* fr; int tmax, qmax, bmax;
    const int32_t* er_off; const double* er_gain; const double* irbank;
    float* h64; int64_t h_stride; double2* hs64; int64_t hs_stride;
    const Real64Plan* plans; int plan; int lds_bytes;
    const float* x; float* y;
};
void fir64_init_attrs();
// k_fir64_flag: the flagged presets into slot_preset / n_slots; then the windows
hipError_t launch_fir64_flag(const Fir64Launch& a, hipStream_t s);
hipError_t launch_fir64(const Fir64Launch& a, hipStream_t s);
hipError_t launch_ir_spec(unsigned grid, int lds_bytes, hipStream_t s, const int64_t* jobs, int n_jobs,
                          const RealPlan* fir_plans, const double* ir_bank, float2* ir_spec);
// h = (delta + ER) * IR in the time domain, one workgroup per H_TILE taps of a preset
// (tile_begin: first tile per preset, non-decreasing)
hipError_t launch_h_build(unsigned grid, hipStream_t s, const PresetRt* rt, const int32_t* tile_begin, int n_presets,
                          const int32_t* er_off, const double* er_gain, const double* ir_bank, float* hs);
constexpr int H_BUILD_TILE = 1024;   // kernels_fir.h H_TILE
hipError_t launch_fir_h(unsigned grid, int lds_bytes, hipStream_t s, const PresetRt* rt, const int32_t* hblk_begin,
                        int n_presets, const RealPlan* fir_plans, const int32_t* fir_plan_of, const float* hs,
                        float2* hspec);
// register-resident FIR with compile-time transform size M = N/2 in {1024..16384}
bool fir2_tables_host(int M, std::vector<float>& out);
// frequency-domain delay line (msg_fir with many partitions): segment spectra, then MAC + inverse
hipError_t launch_fdl(int M, unsigned grid, hipStream_t s, const PresetRt* rt, const int2* jobs, const float2* tables,
                      const float2* hspec, float2* xspec, const float* x_in, float* y_out);
hipError_t launch_fir2(int M, unsigned grid, hipStream_t s, const PresetRt* rt, const int2* jobs,
                       const float2* tables, const float2* hspec, const float* x_in, float* y_out);
// four-pass variant on 1024 threads (M = 16384 only; fir4_fft.h), same jobs and spectra as k_fir2
bool fir4_tables_host(int M, std::vector<float>& out);
hipError_t launch_fir4(int M, unsigned grid, hipStream_t s, const PresetRt* rt, const int2* jobs,
                       const float2* tables, const float2* hspec, const float* x_in, float* y_out);
// partition spectra on the k_fir4 engine (fir4_fft.h): k_fir4_hpart over the (preset, q) jobs
hipError_t launch_fir4_hpart(int M, unsigned n_parts, hipStream_t s, const PresetRt* rt, const int2* part_jobs,
                             const float2* tables, const float* hs, float2* hspec);
// one-partition spectra at N = 32768 from the taps (fir4_fft.h): S = rfft(IR) per job
// [src off, len, spec off, 0] of the float64 bank; H = rfft(delta + ER taps) . S per listed preset
hipError_t launch_fir4_hconv(unsigned n_presets, hipStream_t s, const PresetRt* rt, const int32_t* list,
                             const float2* tables, const int32_t* er_off, const double* er_gain, float2* hspec);
hipError_t launch_fir4_irspec(unsigned n_jobs, hipStream_t s, const int64_t* jobs, const float2* tables,
                              const double* src, float2* hspec);
// N = 65536 overlap-save, one partition (fir8_fft.h): blocks on the k_fir4 engine in
// two halves.  Spectra (even/odd bin layout, N/2 + 1 float2): k_fir8_hconv per listed
// ER preset (rfft(delta + taps) . S_IR), k_fir8_spec per job [src off, len, spec off, 0]
// of float64 (IR bank) or float32 samples.
constexpr int FIR8_N = 65536;
// float2 per filter spectrum on the N = 65536 engine: He (N / 4 + 1 bins) then Ho
// (N / 4) from a 128-byte-aligned offset (fir8::HO), a multiple of 16 float2
constexpr int FIR8_HSTRIDE = FIR8_N / 4 + 16 + FIR8_N / 4;
hipError_t launch_fir8(unsigned grid, hipStream_t s, const PresetRt* rt, const int2* jobs, const float2* tables,
                       const float2* hspec, const float* x_in, float* y_out);
hipError_t launch_fir8p(unsigned n_jobs, unsigned grid, hipStream_t s, const PresetRt* rt, const int2* jobs,
                        const float2* tables, const float2* hspec, const float* x_in, float* y_out, int32_t* ctr,
                        const msg_event* events, const int64_t* grain_off, const float* grain_pool,
                        const int32_t* ev_lo);   // events: null if no ola_fir preset; grain_off: per event
                                                 // slot, its grain in the pool; ev_lo: per job, the first
                                                 // event reaching its segment
// two partitions of N / 2 taps on the N = 65536 engine (fir8_fft.h k_fir8q): B = P = 32768,
// runs (signal, first block) of run_len blocks; the signal's PresetRt::fir_Q holds its block count
constexpr int FIR8Q_P = FIR8_N / 2;
hipError_t launch_fir8q(unsigned n_runs, int run_len, unsigned grid, hipStream_t s, const PresetRt* rt, const int2* runs,
                        const float2* tables, const float2* hspec, const float* x_in, float* y_out, float2* scratch,
                        int32_t* ctr);
int64_t fir8q_scratch_per_wg();
hipError_t launch_fir8_hconv(unsigned n_presets, hipStream_t s, const PresetRt* rt, const int32_t* list,
                             const float2* tables, const int32_t* er_off, const double* er_gain, float2* hspec);
hipError_t launch_fir8_spec64(unsigned n_jobs, hipStream_t s, const int64_t* jobs, const float2* tables,
                              const double* src, float2* hspec);
hipError_t launch_fir8_spec32(unsigned n_jobs, hipStream_t s, const int64_t* jobs, const float2* tables,
                              const float* src, float2* hspec);

void fft_bench_init_attrs();
hipError_t launch_fft_bench(bool po2, unsigned grid, int lds_bytes, hipStream_t s, const RealPlan* plans, int plan,
                            int reps, float* sink);

// float64 grain chain (kernels_grain64.h): one workgroup per event / per chained preset
constexpr int G64_THREADS = 512, G64_SLOTS = 8192, G64_MAXPAR_HOST = 256;   // must match kernels_grain64.h
// global-memory slots for grains beyond the LDS engine (persistent workgroups)
struct G64Global {
    double2* A;           // grain buffers, slot_cap double2 per workgroup
    double2* B;           // FFT ping-pong scratch, same size
    uint32_t* mask;       // partial-lock selection bits, mask_words per workgroup
    int64_t slot_cap, mask_words;
};
void grain64_init_attrs();
// the two k_grain64 instantiations live in their own TUs (k_grain64_lds.hip,
// k_grain64_glb.hip) so they compile in parallel; launch_grain64 picks one
void grain64_lds_init_attr();
hipError_t launch_grain64_lds(unsigned grid, int lds_bytes, hipStream_t s, const msg_preset* presets,
                              const Ev64* ev64, const PresetRt* rt, const Real64Plan* plans, const int32_t* list,
                              int n_list, const double* irbank, const uint8_t* imgbank, nprng::Zig z,
                              double* micro64, double* grain64, double2* save, float* grain_pool);
hipError_t launch_grain64_glb(const G64Global& g, unsigned grid, hipStream_t s, const msg_preset* presets,
                              const Ev64* ev64, const PresetRt* rt, const Real64Plan* plans, const int32_t* list,
                              int n_list, const double* irbank, const uint8_t* imgbank, nprng::Zig z,
                              double* micro64, double* grain64, double2* save, float* grain_pool);
hipError_t launch_grain64(const G64Global* g, unsigned grid, int lds_bytes, hipStream_t s, const msg_preset* presets,
                          const Ev64* ev64, const PresetRt* rt, const Real64Plan* plans, const int32_t* list,
                          int n_list, const double* irbank, const uint8_t* imgbank, nprng::Zig z, double* micro64,
                          double* grain64, double2* save, float* grain_pool);
hipError_t launch_chain64(const G64Global* g, unsigned grid, int lds_bytes, hipStream_t s, const msg_preset* presets,
                          const Ev64* ev64, const Chain64* chains, int n_chains, const Real64Plan* plans,
                          const double* grain64, double* state, float* grain_pool);
hipError_t launch_fft64_one(int lds_bytes, hipStream_t s, const Real64Plan* plans, int plan, int inverse,
                            double* io, double2* gA, double2* gB);

// stereo, tanh clip and peak normalisation (kernels_stereo.h)
hipError_t launch_stereo_max(unsigned n_tiles, hipStream_t s, const PresetRt* rt, const int32_t* st_begin, int n_presets,
                             const float* y, unsigned* maxbits, const StereoSync& sy);
// after k_stereo_max, with the float64 FIR on: per preset the predictor's sums (tile order) and flag64
hipError_t launch_stereo_pred(unsigned n_presets, hipStream_t s, const PresetRt* rt, const int32_t* st_begin,
                              int n_tiles, const unsigned* maxbits, const StereoSync& sy);
hipError_t launch_stereo_out(unsigned n_tiles, hipStream_t s, const PresetRt* rt, const int32_t* st_begin, int n_presets,
                             const float* y, const float* r2, const unsigned* maxbits, float* out);
hipError_t launch_stereo_remax(unsigned grid, hipStream_t s, const PresetRt* rt, const int32_t* st_count,
                               const int32_t* list, const int32_t* n_list, int tmax, const float* y, const float* r2,
                               unsigned* maxbits);

// odd-length stereo rotation (kernels_stereo_odd.h): Bluestein through M = pow2 >= 2n-1
void stereo_odd_init_attrs();
// row_max / col_max: transform-split limits (0: the defaults 4096 / 2048)
int64_t stereo_odd_len(int64_t n, int row_max, int col_max);   // M, or -1 when n is too long
hipError_t launch_stereo_odd_kernel(int64_t n, int row_max, int col_max, double2* Bp, double2* A, hipStream_t s);
hipError_t launch_stereo_odd(int64_t n, int row_max, int col_max, int dr, double width, const float* y,
                             const double2* Bp, double2* A, float* r2, hipStream_t s);
// the app's spectrogram (stft_mag_db, MS:197-212) on the float64 engine
hipError_t launch_stft64(unsigned frames, int lds_bytes, hipStream_t s, const Real64Plan* plans, int plan,
                         const void* x, int elem_bytes, int64_t n, int channels, int win, int hop, double* S);

// per-render summary and digest (kernels_digest.h): tiles of 2048 frames, then
// one fold per render into res (msg_digest_rec records); part holds one
// 48-byte partial per tile.
hipError_t launch_digest(int n, int n_tiles, hipStream_t s, const float* out, const int64_t* frame_off,
                         const int64_t* frames, const int32_t* tile_base, void* part, void* res);
int64_t digest_tiles(int64_t frames);

// polyphase resampler (kernels_resample.h): one workgroup per output tile of plan p;
// meta holds four int64 rows of n_sig (input offsets, input frames, output offsets,
// first tiles), tab the plan's tap table (rs_table)
hipError_t launch_resample(const RsPlan& p, int channels, unsigned tiles, hipStream_t s, const float* x, float* y,
                           const int64_t* meta, int n_sig, const float* tab, int up, int down, int64_t K);

// BS.1770 integrated loudness (kernels_loudness.h): two sweeps over the tiles with the
// tile scan between them, then one wave per signal into rec (msg_loudness_rec records).
// meta: three int64 rows (offsets, frames, n_sig + 1 first tiles); tab: ld_table of the
// rate; state: 4 * channels doubles per tile; part: 2 doubles per tile (energy, peak)
hipError_t launch_loudness(int n_sig, int channels, unsigned tiles, hipStream_t s, const float* x, const int64_t* meta,
                           int64_t hop, const double* tab, double* state, double* part, void* rec);
// The same measurement, then the hop sums and the loudness-range records (kernels_lrange.h):
// loud_rec may be null; meta carries two more rows of n_sig, each signal's first double in
// hops (n / hop sums) and in win (one double per short-term window); range_rec: msg_lrange_rec records
hipError_t launch_loudness_range(int n_sig, int channels, unsigned tiles, hipStream_t s, const float* x,
                                 const int64_t* meta, int64_t hop, const double* tab, double* state, double* part,
                                 void* loud_rec, double* hops, double* win, void* range_rec);
// x *= (float)g per signal, g from its record; meta as above with tiles of LD_GAIN_TILE frames
hipError_t launch_loudness_gain(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                                void* rec, double target, double ceiling);

// BS.1770 true peak (kernels_truepeak.h): one workgroup per tile of TP_TILE positions, then
// one wave per signal into rec (msg_truepeak_rec records).  meta as for the loudness
// (tiles: tp_tiles); tab: tp_table, uploaded once with the context; part: one uint2 per tile
hipError_t launch_truepeak(int n_sig, int channels, int os, unsigned tiles, hipStream_t s, const float* x,
                           const int64_t* meta, const float* tab, void* part, void* rec);
// x *= (float)g per signal, g from its records (loud_rec may be null); tiles of TP_GAIN_TILE frames
hipError_t launch_truepeak_gain(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                                void* loud_rec, void* tp_rec, double target, double ceil_tp, double ceil_pk);

// PCM quantiser (kernels_pcm.h): one workgroup per tile of PCM_TILE words, then one wave per
// signal into rec (msg_pcm_rec records).  meta: offsets, frames, n_sig + 1 first tiles
// (pcm_tiles of the words), stream keys, output byte offsets; part: one int4 per tile
hipError_t launch_pcm(int n_sig, int channels, int bits, int dither, unsigned tiles, hipStream_t s, const float* x,
                      const int64_t* meta, void* out, void* part, void* rec);
// noise-shaped quantiser (kernels_pcm_shape.h): one lane per signal, waves of PCM_SHAPE_T signals,
// each lane's record into rec.  meta as for launch_pcm (the tile bases unused); n_sig > 0
hipError_t launch_pcm_shape(int n_sig, int channels, int bits, int dither, int shape, hipStream_t s, const float* x,
                            const int64_t* meta, void* out, void* rec);

// look-ahead true-peak limiter (kernels_limit.h): the envelope over env_tiles tiles of LIM_ENV_TILE
// frames into rbuf and nanpart, one wave per signal into state, the apply over tiles of
// lim_tile(L) frames in place, then one wave per signal into rec (msg_limit_rec records).
// meta: offsets, frames, n_sig + 1 first apply tiles, n_sig first scratch floats, n_sig + 1
// first envelope tiles; tab: tp_table; w: lim_weights(L); tp_rec: measured records or null;
// part: one uint2 per apply tile
void limit_init_attrs();
hipError_t launch_limit(int n_sig, int channels, int os, unsigned env_tiles, unsigned tiles, hipStream_t s, float* x,
                        const int64_t* meta, const float* tab, float c32, int L, const float* w, const void* tp_rec,
                        float* rbuf, uint32_t* nanpart, int32_t* state, void* part, void* rec);

// edges pass (kernels_edges.h): with a trim the records' first / last reset and the find over
// find_tiles tiles of EDG_TILE frames, then one lane per signal forms the span, then the apply
// over apply_tiles tiles of EDG_APPLY_TILE frames of the fade or crossfade regions in place.
// meta: offsets, frames, n_sig + 1 first find tiles, n_sig + 1 first apply tiles
// (edg_apply_tiles); rec: msg_edges_rec records
struct EdgesPar;
hipError_t launch_edges(int n_sig, int channels, unsigned find_tiles, unsigned apply_tiles, hipStream_t s, float* x,
                        const int64_t* meta, const EdgesPar& par, void* rec);

// delivery filter (kernels_filter.h): the first sweep over tiles of FL_TILE frames writes every
// full tile's zero-state end state, the scan turns them into incoming states, the second sweep
// filters in place.  meta: offsets, frames, n_sig + 1 first tiles (fl_tiles); tab: fl_table of
// the cascade; state: 2 * n_sections * channels doubles per tile; reverse: from the last frame
hipError_t launch_filter(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                         int n_sections, int reverse, const double* tab, double* state);

// stereo meter (kernels_image.h): one sweep over tiles of IMG_TILE frames that never straddle a
// hop writes three float64 sums per tile, then one wave per signal folds them into the record.
// meta: offsets, frames, n_sig + 1 first tiles (img_tiles); part: 3 doubles per tile; rec:
// msg_stereo_rec records
hipError_t launch_image_meter(int n_sig, unsigned tiles, hipStream_t s, const float* x, const int64_t* meta, int64_t hop,
                              double* part, void* rec);
// stereo image: the 2 x 2 matrix m in place, or (fold not null) the fold row into y at the output
// offsets that follow the first tiles in meta (img_apply_tiles); rec: null, or the meter's
// records, whose corr < 0 inverts the right channel of that signal first
hipError_t launch_image_apply(int n_sig, unsigned tiles, hipStream_t s, float* x, const int64_t* meta, const float* m,
                              const float* fold, float* y, const void* rec);

// compressor (kernels_dynamics.h): the first sweep over tiles of DYN_TILE frames writes every tile's
// two summaries and its non-finite flag, the scan turns them into the carries that enter every tile,
// folds the flags into state and initialises rec (msg_dynamics_rec records), the second sweep
// compresses in place and folds the records.  meta: offsets, frames, n_sig + 1 first tiles
// (dyn_tiles); carry: 4 words per tile; flag: one word per tile; state: one word per signal; halo:
// with a hold, hold_frames words per tile (the demands before the tile, saved by the first sweep), else null
struct DynPar;
void dynamics_init_attrs();
hipError_t launch_dynamics(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                           const DynPar& par, int64_t* carry, uint32_t* flag, int32_t* state, void* rec, int64_t* halo);

// gate (kernels_gate.h): with hysteresis or a hold a read-only state sweep writes every tile's
// transfer and a scan turns them into the age that enters every tile; then, as the compressor, the
// first sweep writes every tile's two summaries and its non-finite flag, the scan turns them into
// the carries, folds the flags into state and initialises rec (msg_gate_rec records), the second
// sweep gates in place and folds the records.  meta: offsets, frames, n_sig + 1 first tiles
// (dyn_tiles); carry, trans: 4 words per tile each; flag: one word per tile; state: one word per signal
struct GatePar;
hipError_t launch_gate(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                       const GatePar& par, int64_t* carry, int64_t* trans, uint32_t* flag, int32_t* state, void* rec);

// FLAC encoder (kernels_flac.h): the plan sweep writes every block's FlacPlan (21 words) with its
// frame's bytes, a scan per signal turns them into the prefix pre (one word per block) and the
// records (msg_flac_rec) but for byte_off, which a scan over the signals sets; the pack sweep writes
// the frames into out, and with md5 a last launch hashes every signal's PCM.  meta: byte offsets,
// frames, n_sig + 1 first blocks
hipError_t launch_flac(int n_sig, int channels, int bits, int block, int sr, bool md5, unsigned tiles, hipStream_t s,
                       const void* pcm, const int64_t* meta, void* plan, int64_t* pre, void* rec, void* out, int64_t out_bytes);
