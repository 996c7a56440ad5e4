// kernels_gate.h — the device side of msg_gate_apply (TU k_gate.hip).  The definition, the age
// algebra (GateSeg, gate_join, gate_through) and the host loop are in gate.h, the max-plus algebra
// and the tile shape in dynamics.h; DESIGN.md "4m. Gate" explains the decomposition, which is the
// compressor's (kernels_dynamics.h) with a state scan in front of it.
//
//   k_gate_tiles<CH, GATE_SWEEP_STATE>   read-only, one workgroup per tile of DYN_TILE frames: the
//                              frames' classes (O, C, N) from two comparisons of bit patterns, and
//                              the tile's transfer, the GateSeg of its frames in order.
//   k_gate_scan_state          one workgroup per signal: the age that enters every tile, by a scan
//                              over blocks of DYN_T tiles (a wave scan, the waves through LDS, the
//                              blocks in order), from hold_frames + 1 in front of the signal.
//   k_gate_tiles<CH, GATE_SWEEP_SUM>     sweep 1: the ages of the tile's frames from the age that
//                              enters it, the openness o, and the tile's two summaries: Cf, the
//                              closing envelope at its last frame from a zero carry, and Cb, the
//                              opening envelope at its first frame from a zero carry; and whether
//                              it holds a NaN or an infinity.
//   k_gate_scan_env            one workgroup per signal and direction: the carries that enter
//                              every tile, as k_dynamics_scan; the forward workgroup also folds the
//                              non-finite flags into the signal's state and initialises its record.
//   k_gate_tiles<CH, GATE_SWEEP_APPLY>   sweep 2: ages and o again from the tile's own samples and
//                              the age that enters it, F and B from the carries, E = RANGE - max,
//                              the gain, the tile stored in place; frames whose gain is 1 are not
//                              written.  No sample outside the tile is read: the tile before is
//                              another workgroup's to overwrite.  The record's integers are folded
//                              over the workgroup and added with one integer atomic each.
//
// Without hysteresis and without a hold (par.local) a frame's state is its own class: the state
// sweep and its scan are not launched, sweep 1 takes sh from the class and leaves, for sweep 2's
// count of openings, the age that enters the next tile (0 or 1) where the state scan would.
//
// Inside a tile lane l owns frames [16 l, 16 l + 16).  The class and the reduction r are formed
// where the tile is loaded (frame k DYN_T + tid: coalesced) and go through LDS as one int64 word
// r << 2 | class in rows of DYN_C + 1 (dyn_pos), so a lane's chunk reads conflict-free.  The gains
// go back through the same LDS as floats to the coalesced layout for the store.
#pragma once
#include <hip/hip_runtime.h>
#include "gate.h"
#include "sig_tiles.h"

enum : int { GATE_SWEEP_STATE = 0, GATE_SWEEP_SUM = 1, GATE_SWEEP_APPLY = 2 };
constexpr int GATE_LDS_WORDS = DYN_TILE + DYN_TILE / DYN_C + 1;       // dyn_pos(DYN_TILE) + 1

MSG_DEV int64_t gate_shfl_up(int64_t v, int o) { return (int64_t)__shfl_up((long long)v, (unsigned)o, 64); }
MSG_DEV int64_t gate_shfl_down(int64_t v, int o) { return (int64_t)__shfl_down((long long)v, (unsigned)o, 64); }
MSG_DEV int64_t gate_shfl_xor(int64_t v, int o) { return (int64_t)__shfl_xor((long long)v, o, 64); }

// The inclusive scan of runs over a wave: lane l gets the runs of lanes 0 .. l in that order.
MSG_DEV GateSeg gate_wave_scan(GateSeg v, int lane, int32_t hold) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int o = 1 << j;
        GateSeg u;
        u.L = gate_shfl_up(v.L, o);
        u.K = gate_shfl_up(v.K, o);
        u.fixed = __shfl_up(v.fixed, (unsigned)o, 64);
        if (lane >= o) v = gate_join(u, v, hold);
    }
    return v;
}
// the runs before this lane's own (the empty run for lane 0)
MSG_DEV GateSeg gate_wave_before(const GateSeg& inc, int lane) {
    GateSeg u;
    u.L = gate_shfl_up(inc.L, 1);
    u.K = gate_shfl_up(inc.K, 1);
    u.fixed = __shfl_up(inc.fixed, 1u, 64);
    if (lane == 0) u = GateSeg{0, 0, 0};
    return u;
}
// The same for the envelope's runs.  FWD: lanes 0 .. l in that order; otherwise lanes 63 down to l.
template <bool FWD>
MSG_DEV DynSeg gate_env_scan(DynSeg v, int lane) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int o = 1 << j;
        DynSeg u;
        u.R = FWD ? gate_shfl_up(v.R, o) : gate_shfl_down(v.R, o);
        u.C = FWD ? gate_shfl_up(v.C, o) : gate_shfl_down(v.C, o);
        if (FWD ? lane >= o : lane + o < 64) v = dyn_join(u, v);
    }
    return v;
}
template <bool FWD>
MSG_DEV DynSeg gate_env_before(const DynSeg& inc, int lane) {
    DynSeg u;
    u.R = FWD ? gate_shfl_up(inc.R, 1) : gate_shfl_down(inc.R, 1);
    u.C = FWD ? gate_shfl_up(inc.C, 1) : gate_shfl_down(inc.C, 1);
    if (FWD ? lane == 0 : lane == 63) u = DynSeg{0, 0};
    return u;
}

template <int CH>
MSG_DEV uint32_t gate_load_level(const float* __restrict__ xs, int64_t f, float (&v)[CH]) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    if (CH == 2) {
        const v2f w = reinterpret_cast<const v2f*>(xs)[f];
        v[0] = w.x; v[CH - 1] = w.y;
    } else {
        v[0] = xs[f];
    }
    return dyn_level(v, CH);
}

// carry: four rows of n_tiles words, Cf, Cb, Fin, Bin.  trans: four rows of n_tiles words, the
// tile's transfer L, K, fixed, and the age that enters the tile.
template <int CH, int MODE>
__global__ void __launch_bounds__(DYN_T)
k_gate_tiles(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, GatePar par, int64_t* __restrict__ carry,
             int64_t* __restrict__ trans, uint32_t* __restrict__ flag, const int32_t* __restrict__ sig_state,
             GateRec* __restrict__ rec, int64_t n_tiles) {
    __shared__ __attribute__((aligned(16))) int64_t a[GATE_LDS_WORDS];
    __shared__ GateSeg wg[DYN_T / 64];
    __shared__ DynSeg wf[DYN_T / 64], wb[DYN_T / 64];
    __shared__ int64_t red[DYN_T / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t tile = blockIdx.x;
    const int p = sig_owner(tile_base, n_sig, tile);
    if (MODE == GATE_SWEEP_APPLY && sig_state[p] == 2) return;       // a NaN or an infinity: the signal stays as it was
    const int64_t n = meta[n_sig + p], f0 = (tile - tile_base[p]) * DYN_TILE;
    const int lt = (int)(n - f0 < DYN_TILE ? n - f0 : DYN_TILE);     // frames of the tile (1 .. DYN_TILE)
    const int32_t H = par.hold;
    float* xs = x + (meta[p] + f0) * CH;                // 64-bit from the buffer's base

    // the tile's frames, coalesced, every load in flight first; then class and reduction into LDS
    constexpr bool KEEP = MODE == GATE_SWEEP_APPLY;     // only sweep 2 multiplies the samples; the others keep the levels
    float ld[KEEP ? DYN_C : 1][CH];
    uint32_t lv[DYN_C];
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) {
        const int f = k * DYN_T + tid;
        float (&v)[CH] = ld[KEEP ? k : 0];
        lv[k] = 0;
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) v[ch] = 0.f;
        if (f < lt) lv[k] = gate_load_level<CH>(xs, f, v);
    }
    bool bad = false;                                   // a NaN or an infinity in the tile: sweep 1 alone reports it
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) {
        const int f = k * DYN_T + tid;
        if (MODE == GATE_SWEEP_SUM) bad = bad || lv[k] >= DYN_INF;
        if (f < lt) {
            const int c = gate_class(lv[k], par);
            int64_t w = c;
            if (MODE != GATE_SWEEP_STATE && c != GATE_O) w |= gate_reduction(lv[k], par) << 2;   // an O frame is open: no r
            a[dyn_pos(f)] = w;
        }
    }
    if (MODE == GATE_SWEEP_SUM) {
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (tid == 0) flag[tile] = any ? 1u : 0u;
    } else {
        __syncthreads();
    }

    const int left = lt - tid * DYN_C;
    const int cl = left < 0 ? 0 : (left > DYN_C ? DYN_C : left);     // frames of this lane's chunk
    int cls[DYN_C];
    int64_t o[DYN_C];                                   // r, then the openness
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) {
        const int64_t w = k < cl ? a[dyn_pos(tid * DYN_C + k)] : 0;
        cls[k] = (int)(w & 3);
        o[k] = w >> 2;
    }

    // sh of the chunk's frames as a bit mask, and sh of the frame before the chunk
    uint32_t open = 0, prev_open = 0;
    if (MODE == GATE_SWEEP_SUM && par.local) {
#pragma unroll
        for (int k = 0; k < DYN_C; ++k)
            if (k < cl && cls[k] == GATE_O) open |= 1u << k;
        // what the state scan would have left for sweep 2: the age that enters each tile, 0 or 1
        if (tid == ((lt - 1) >> 4) && tile + 1 < tile_base[p + 1])
            trans[3 * n_tiles + tile + 1] = (open >> ((lt - 1) & 15)) & 1u ? 0 : 1;
        if (tid == 0 && tile == tile_base[p]) trans[3 * n_tiles + tile] = 1;
    } else {
        GateSeg sg{0, 0, 0};
#pragma unroll
        for (int k = 0; k < DYN_C; ++k)
            if (k < cl) sg = gate_join(sg, gate_frame(cls[k]), H);
        const GateSeg inc = gate_wave_scan(sg, lane, H);
        const GateSeg ex = gate_wave_before(inc, lane);
        if (lane == 63) wg[wave] = inc;
        __syncthreads();
        if (MODE == GATE_SWEEP_STATE) {
            if (tid == 0) {
                GateSeg t{0, 0, 0};
#pragma unroll
                for (int w = 0; w < DYN_T / 64; ++w) t = gate_join(t, wg[w], H);
                trans[tile] = t.L;
                trans[n_tiles + tile] = t.K;
                trans[2 * n_tiles + tile] = t.fixed;
            }
            return;
        }
        GateSeg pre{0, 0, 0};
        for (int w = 0; w < wave; ++w) pre = gate_join(pre, wg[w], H);
        int64_t age = gate_through(ex, gate_through(pre, trans[3 * n_tiles + tile], H), H);
        prev_open = age <= H ? 1u : 0u;
#pragma unroll
        for (int k = 0; k < DYN_C; ++k)
            if (k < cl) {
                age = gate_age(age, cls[k], H);
                if (age <= H) open |= 1u << k;
            }
    }
    if (MODE == GATE_SWEEP_STATE) return;               // for the compiler: the state sweep left above
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) o[k] = k < cl ? ((open >> k) & 1u ? par.range : par.range - o[k]) : 0;

    // the chunk's runs from zero, the scans over the wave, the waves through LDS
    DynSeg sf{dyn_span(cl, par.rstep), 0}, sb{dyn_span(cl, par.astep), 0};
#pragma unroll
    for (int k = 0; k < DYN_C; ++k)
        if (k < cl) sf.C = dyn_step(sf.C, par.rstep, o[k]);
#pragma unroll
    for (int k = DYN_C - 1; k >= 0; --k)
        if (k < cl) sb.C = dyn_step(sb.C, par.astep, o[k]);
    const DynSeg incf = gate_env_scan<true>(sf, lane), incb = gate_env_scan<false>(sb, lane);
    const DynSeg exf = gate_env_before<true>(incf, lane), exb = gate_env_before<false>(incb, lane);
    if (lane == 63) wf[wave] = incf;
    if (lane == 0) wb[wave] = incb;
    __syncthreads();                                    // also: every read of a[] lies before it

    if (MODE == GATE_SWEEP_SUM) {
        if (tid == 0) {
            DynSeg tf{0, 0}, tb{0, 0};
#pragma unroll
            for (int w = 0; w < DYN_T / 64; ++w) {
                tf = dyn_join(tf, wf[w]);
                tb = dyn_join(tb, wb[DYN_T / 64 - 1 - w]);
            }
            carry[tile] = tf.C;                         // Cf
            carry[n_tiles + tile] = tb.C;               // Cb
        }
        return;
    }

    DynSeg pf{0, 0}, pb{0, 0};                          // the waves before this one, in each direction
    for (int w = 0; w < wave; ++w) pf = dyn_join(pf, wf[w]);
    for (int w = DYN_T / 64 - 1; w > wave; --w) pb = dyn_join(pb, wb[w]);
    int64_t e[DYN_C];
    int64_t y = dyn_carry(exf, dyn_carry(pf, carry[2 * n_tiles + tile]));          // Fin
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) {
        if (k < cl) y = dyn_step(y, par.rstep, o[k]);
        e[k] = y;
    }
    y = dyn_carry(exb, dyn_carry(pb, carry[3 * n_tiles + tile]));                  // Bin
    int64_t mx = 0, sum = 0, cnt = 0;
    float* gl = reinterpret_cast<float*>(a);
#pragma unroll
    for (int k = DYN_C - 1; k >= 0; --k)
        if (k < cl) {
            y = dyn_step(y, par.astep, o[k]);
            const int64_t v = par.range - dyn_max(e[k], y);
            mx = dyn_max(mx, v);
            sum += v >> 16;
            cnt += v > 0 ? 1 : 0;
            gl[dyn_pos(tid * DYN_C + k)] = gate_gain(v);
        }
    int64_t nopen = __popc(open), nopens = __popc(open & ~((open << 1) | prev_open));
    // the record's integers: over the wave, the waves through LDS, one atomic each
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        mx = dyn_max(mx, gate_shfl_xor(mx, s));
        sum += gate_shfl_xor(sum, s);
        cnt += gate_shfl_xor(cnt, s);
        nopen += gate_shfl_xor(nopen, s);
        nopens += gate_shfl_xor(nopens, s);
    }
    if (lane == 0) { red[wave][0] = mx; red[wave][1] = sum; red[wave][2] = cnt; red[wave][3] = nopen; red[wave][4] = nopens; }
    __syncthreads();                                    // the gains are staged too
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < DYN_T / 64; ++w) {
            mx = dyn_max(mx, red[w][0]);
            sum += red[w][1];
            cnt += red[w][2];
            nopen += red[w][3];
            nopens += red[w][4];
        }
        if (cnt > 0) {
            atomicMax(reinterpret_cast<unsigned long long*>(&rec[p].max_e), (unsigned long long)mx);
            atomicAdd(reinterpret_cast<unsigned long long*>(&rec[p].sum_e16), (unsigned long long)sum);
            atomicAdd(reinterpret_cast<unsigned long long*>(&rec[p].reduced_frames), (unsigned long long)cnt);
            atomicMax(&rec[p].state, 1);
        }
        if (nopen > 0) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&rec[p].open_frames), (unsigned long long)nopen);
            atomicAdd(reinterpret_cast<unsigned long long*>(&rec[p].opens), (unsigned long long)nopens);
        }
    }
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) {
        const int f = k * DYN_T + tid;
        if (f < lt) {
            const float g = gl[dyn_pos(f)];
            const float (&v)[CH] = ld[KEEP ? k : 0];    // sweep 2 alone comes here
            if (!dyn_is_one(g)) {
                typedef float v2f __attribute__((ext_vector_type(2)));
                if (CH == 2) {
                    v2f w;
                    w.x = v[0] * g; w.y = v[CH - 1] * g;
                    reinterpret_cast<v2f*>(xs)[f] = w;
                } else {
                    xs[f] = v[0] * g;
                }
            }
        }
    }
}

// The age that enters every tile of a signal, tiles in order, from hold_frames + 1 in front of
// the first: trans rows 0 .. 2 in, row 3 out.
__global__ void __launch_bounds__(DYN_T)
k_gate_scan_state(const int64_t* __restrict__ meta, int n_sig, GatePar par, int64_t* __restrict__ trans, int64_t n_tiles) {
    __shared__ GateSeg wt[DYN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t t0 = tile_base[p], T = tile_base[p + 1] - t0;
    const int32_t H = par.hold;
    int64_t c = (int64_t)H + 1;                         // the age that enters this block of tiles
    for (int64_t base = 0; base < T; base += DYN_T) {
        const int64_t u = base + tid;
        GateSeg s{0, 0, 0};
        if (u < T) s = GateSeg{trans[t0 + u], trans[n_tiles + t0 + u], (int32_t)trans[2 * n_tiles + t0 + u]};
        const GateSeg inc = gate_wave_scan(s, lane, H);
        const GateSeg ex = gate_wave_before(inc, lane);
        if (lane == 63) wt[wave] = inc;
        __syncthreads();
        GateSeg pre{0, 0, 0}, all{0, 0, 0};
#pragma unroll
        for (int w = 0; w < DYN_T / 64; ++w) {
            if (w < wave) pre = gate_join(pre, wt[w], H);
            all = gate_join(all, wt[w], H);
        }
        if (u < T) trans[3 * n_tiles + t0 + u] = gate_through(ex, gate_through(pre, c, H), H);
        c = gate_through(all, c, H);
        __syncthreads();                                // wt is written again
    }
}

// The carries that enter every tile of a signal: blockIdx.y = 0 the closing ramp (tiles in order,
// the value at the end of tile t - 1 enters tile t), 1 the opening ramp (tiles from the last to the
// first).  carry: four rows of n_tiles words, Cf, Cb, Fin, Bin.
__global__ void __launch_bounds__(DYN_T)
k_gate_scan_env(const int64_t* __restrict__ meta, int n_sig, GatePar par, int64_t* __restrict__ carry,
                const uint32_t* __restrict__ flag, int32_t* __restrict__ sig_state, GateRec* __restrict__ rec,
                int64_t n_tiles) {
    __shared__ DynSeg wt[DYN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const bool back = blockIdx.y != 0;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t t0 = tile_base[p], T = tile_base[p + 1] - t0, n = meta[n_sig + p];
    if (!back) {
        int bad = 0;
        for (int64_t i = tid; i < T; i += DYN_T) bad |= flag[t0 + i] ? 1 : 0;
        bad = __syncthreads_or(bad);
        if (tid == 0) {
            sig_state[p] = bad ? 2 : 0;
            rec[p] = GateRec{0, 0, 0, 0, 0, bad ? 2 : 0, par.hold};
        }
    }
    const int64_t step = back ? par.astep : par.rstep;
    const int64_t* in = carry + (back ? n_tiles : 0) + t0;
    int64_t* out = carry + (back ? 3 : 2) * n_tiles + t0;
    int64_t c = 0;                                      // the value that enters this block of tiles
    for (int64_t base = 0; base < T; base += DYN_T) {
        const int64_t u = base + tid, t = back ? T - 1 - u : u;      // u: the tile in time order
        DynSeg s{0, 0};
        if (u < T) {
            const int64_t len = n - t * DYN_TILE < DYN_TILE ? n - t * DYN_TILE : DYN_TILE;
            s = DynSeg{dyn_span(len, step), in[t]};
        }
        const DynSeg inc = gate_env_scan<true>(s, lane);
        const DynSeg ex = gate_env_before<true>(inc, lane);
        if (lane == 63) wt[wave] = inc;
        __syncthreads();
        DynSeg pre{0, 0}, all{0, 0};
#pragma unroll
        for (int w = 0; w < DYN_T / 64; ++w) {
            if (w < wave) pre = dyn_join(pre, wt[w]);
            all = dyn_join(all, wt[w]);
        }
        if (u < T) out[t] = dyn_carry(ex, dyn_carry(pre, c));
        c = dyn_carry(all, c);
        __syncthreads();                                // wt is written again
    }
}
