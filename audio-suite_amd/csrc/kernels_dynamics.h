// kernels_dynamics.h — the device side of msg_dynamics (TU k_dynamics.hip).  The definition,
// the max-plus algebra (DynSeg, dyn_join, dyn_carry) and the tile shapes are in dynamics.h;
// DESIGN.md "4l. Dynamics" explains the decomposition, which is the filter's (kernels_filter.h)
// with integer runs in place of float64 states.
//
//   k_dynamics_tiles<CH, HOLD, false>  sweep 1, one workgroup per tile of DYN_TILE frames counted
//                              from the signal's first frame: the tile's demands d (and, HOLD, the
//                              hold_frames before it), dh, and the tile's two summaries: Cf, the
//                              release envelope at its last frame from a zero carry, and Cb, the
//                              attack envelope at its first frame from a zero carry; and whether
//                              it holds a NaN or an infinity.
//   k_dynamics_scan            one workgroup per signal and direction: the carries that enter
//                              every tile, Fin from the left and Bin from the right, by a scan
//                              over blocks of DYN_T tiles (a wave scan, the waves through LDS, the
//                              blocks in order); the forward workgroup also folds the non-finite
//                              flags into the signal's state and initialises its record.
//   k_dynamics_tiles<CH, HOLD, true>   sweep 2: d of the tile's own frames again from the samples, F
//                              and B from the carries, E, the gain, the tile stored in place;
//                              frames whose gain is 1 are not written.  HOLD: the demands of the
//                              hold_frames before the tile are read back from the words sweep 1
//                              saved per tile and never from the samples, which lie in the tile
//                              before and which another workgroup of this launch overwrites.
//                              A signal flagged non-finite is skipped.  The record's integers are folded
//                              over the workgroup and added with one integer atomic each; integer
//                              max and + give the same bits in any order.
//
// Inside a tile lane l owns frames [16 l, 16 l + 16).  d is formed where the tile is loaded
// (frame k DYN_T + tid: coalesced) and goes through LDS as int64 words in rows of DYN_C + 1
// (dyn_pos), so a lane's chunk reads conflict-free.  HOLD: dh is the running maximum over
// hold_frames + 1 words, formed in place by doubling shifts (log2 passes over halo + tile).
// The gains go back through the same LDS as floats to the coalesced layout for the store.
#pragma once
#include <hip/hip_runtime.h>
#include "dynamics.h"
#include "sig_tiles.h"

MSG_DEV int64_t dyn_shfl_up(int64_t v, int o) { return (int64_t)__shfl_up((long long)v, (unsigned)o, 64); }
MSG_DEV int64_t dyn_shfl_down(int64_t v, int o) { return (int64_t)__shfl_down((long long)v, (unsigned)o, 64); }
MSG_DEV int64_t dyn_shfl_xor(int64_t v, int o) { return (int64_t)__shfl_xor((long long)v, o, 64); }

// The inclusive scan of runs over a wave.  FWD: lane l gets the runs of lanes 0 .. l in that
// order; otherwise the runs of lanes 63 down to l (time runs from the last frame to the first).
template <bool FWD>
MSG_DEV DynSeg dyn_wave_scan(DynSeg v, int lane) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int o = 1 << j;
        DynSeg u;
        u.R = FWD ? dyn_shfl_up(v.R, o) : dyn_shfl_down(v.R, o);
        u.C = FWD ? dyn_shfl_up(v.C, o) : dyn_shfl_down(v.C, o);
        if (FWD ? lane >= o : lane + o < 64) v = dyn_join(u, v);
    }
    return v;
}
// the runs before this lane's own (the empty run for the first lane in time order)
template <bool FWD>
MSG_DEV DynSeg dyn_wave_before(const DynSeg& inc, int lane) {
    DynSeg u;
    u.R = FWD ? dyn_shfl_up(inc.R, 1) : dyn_shfl_down(inc.R, 1);
    u.C = FWD ? dyn_shfl_up(inc.C, 1) : dyn_shfl_down(inc.C, 1);
    if (FWD ? lane == 0 : lane == 63) u = DynSeg{0, 0};
    return u;
}

template <int CH>
MSG_DEV uint32_t dyn_load_level(const float* __restrict__ xs, int64_t f, float (&v)[CH]) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    if (CH == 2) {
        const v2f w = reinterpret_cast<const v2f*>(xs)[f];
        v[0] = w.x; v[CH - 1] = w.y;
    } else {
        v[0] = xs[f];
    }
    return dyn_level(v, CH);
}

template <int CH, bool HOLD, bool APPLY>
__global__ void __launch_bounds__(DYN_T)
k_dynamics_tiles(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, DynPar par,
                 int64_t* __restrict__ carry, uint32_t* __restrict__ flag, const int32_t* __restrict__ sig_state,
                 DynRec* __restrict__ rec, int64_t n_tiles, int64_t* __restrict__ halo) {
    extern __shared__ __attribute__((aligned(16))) int64_t a[];     // dyn_lds_bytes(hold)
    __shared__ DynSeg wf[DYN_T / 64], wb[DYN_T / 64];
    __shared__ int64_t red[DYN_T / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t tile = blockIdx.x;
    const int p = sig_owner(tile_base, n_sig, tile);
    if (APPLY && sig_state[p] == 2) return;             // a NaN or an infinity: the signal stays as it was
    const int64_t n = meta[n_sig + p], f0 = (tile - tile_base[p]) * DYN_TILE;
    const int lt = (int)(n - f0 < DYN_TILE ? n - f0 : DYN_TILE);     // frames of the tile (1 .. DYN_TILE)
    const int H = HOLD ? par.hold : 0;
    float* xs = x + (meta[p] + f0) * CH;                // 64-bit from the buffer's base

    // the tile's frames, coalesced, every load in flight first; then their demands into LDS
    float ld[DYN_C][CH];
    uint32_t lv[DYN_C];
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) {
        const int f = k * DYN_T + tid;
        lv[k] = 0;
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) ld[k][ch] = 0.f;
        if (f < lt) lv[k] = dyn_load_level<CH>(xs, f, ld[k]);
    }
    bool bad = false;
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) {
        const int f = k * DYN_T + tid;
        bad = bad || lv[k] >= DYN_INF;
        if (f < lt) a[dyn_pos(H + f)] = dyn_demand(lv[k], par);
    }
    if (HOLD) {
        // the demands of the H frames before the tile (0 before the signal): sweep 1 forms them from
        // the samples, which nobody writes during its launch, and saves them; sweep 2 reads them back
        int64_t* hs = halo + tile * (int64_t)H;
        for (int j = tid; j < H; j += DYN_T) {
            int64_t v;
            if (APPLY) {
                v = hs[j];
            } else {
                const int64_t f = f0 - H + j;
                float w[CH];
                v = f >= 0 ? dyn_demand(dyn_load_level<CH>(xs, f - f0, w), par) : 0;
                hs[j] = v;
            }
            a[dyn_pos(j)] = v;
        }
    }
    if (!APPLY) {
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (tid == 0) flag[tile] = any ? 1u : 0u;
    } else {
        __syncthreads();
    }

    const int left = lt - tid * DYN_C;
    const int cl = left < 0 ? 0 : (left > DYN_C ? DYN_C : left);     // frames of this lane's chunk
    int64_t d[DYN_C], dh[DYN_C];
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) d[k] = k < cl ? a[dyn_pos(H + tid * DYN_C + k)] : 0;
    if (HOLD) {
        // a[i] <- max of a[i - W + 1 .. i], W = H + 1, by doubling: after a pass with shift s a word
        // covers `have + s` words; words before the halo are 0 and no window of the tile reaches them
        const int M = H + lt;
        for (int have = 1; have < H + 1;) {
            const int s = have < H + 1 - have ? have : H + 1 - have;
            int64_t t[2 * DYN_C];
            __syncthreads();                            // the chunk reads, or the pass before
#pragma unroll
            for (int q = 0; q < 2 * DYN_C; ++q) {
                const int i = q * DYN_T + tid;
                t[q] = 0;
                if (i < M) t[q] = dyn_max(a[dyn_pos(i)], i >= s ? a[dyn_pos(i - s)] : 0);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2 * DYN_C; ++q) {
                const int i = q * DYN_T + tid;
                if (i < M) a[dyn_pos(i)] = t[q];
            }
            have += s;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < DYN_C; ++k) dh[k] = k < cl ? a[dyn_pos(H + tid * DYN_C + k)] : 0;
    } else {
#pragma unroll
        for (int k = 0; k < DYN_C; ++k) dh[k] = d[k];
    }

    // the chunk's runs from zero, the scans over the wave, the waves through LDS
    DynSeg sf{dyn_span(cl, par.rstep), 0}, sb{dyn_span(cl, par.astep), 0};
#pragma unroll
    for (int k = 0; k < DYN_C; ++k)
        if (k < cl) sf.C = dyn_step(sf.C, par.rstep, dh[k]);
#pragma unroll
    for (int k = DYN_C - 1; k >= 0; --k)
        if (k < cl) sb.C = dyn_step(sb.C, par.astep, d[k]);
    const DynSeg incf = dyn_wave_scan<true>(sf, lane), incb = dyn_wave_scan<false>(sb, lane);
    const DynSeg exf = dyn_wave_before<true>(incf, lane), exb = dyn_wave_before<false>(incb, lane);
    if (lane == 63) wf[wave] = incf;
    if (lane == 0) wb[wave] = incb;
    __syncthreads();                                    // also: every read of a[] lies before it

    if (!APPLY) {
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
        if (k < cl) y = dyn_step(y, par.rstep, dh[k]);
        e[k] = y;
    }
    y = dyn_carry(exb, dyn_carry(pb, carry[3 * n_tiles + tile]));                  // Bin
    int64_t mx = 0, sum = 0, cnt = 0;
    float* gl = reinterpret_cast<float*>(a);
#pragma unroll
    for (int k = DYN_C - 1; k >= 0; --k)
        if (k < cl) {
            y = dyn_step(y, par.astep, d[k]);
            const int64_t v = dyn_max(e[k], y);
            mx = dyn_max(mx, v);
            sum += v >> 16;
            cnt += v > 0 ? 1 : 0;
            gl[dyn_pos(tid * DYN_C + k)] = dyn_gain(v, par.makeup);
        }
    // the record's integers: over the wave, the waves through LDS, one atomic each
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = dyn_max(mx, dyn_shfl_xor(mx, o));
        sum += dyn_shfl_xor(sum, o);
        cnt += dyn_shfl_xor(cnt, o);
    }
    if (lane == 0) { red[wave][0] = mx; red[wave][1] = sum; red[wave][2] = cnt; }
    __syncthreads();                                    // the gains are staged too
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < DYN_T / 64; ++w) {
            mx = dyn_max(mx, red[w][0]);
            sum += red[w][1];
            cnt += red[w][2];
        }
        if (cnt > 0) {
            atomicMax(reinterpret_cast<unsigned long long*>(&rec[p].max_e), (unsigned long long)mx);
            atomicAdd(reinterpret_cast<unsigned long long*>(&rec[p].sum_e16), (unsigned long long)sum);
            atomicAdd(reinterpret_cast<unsigned long long*>(&rec[p].reduced_frames), (unsigned long long)cnt);
        }
        if (cnt > 0 || par.makeup != 0.0) atomicMax(&rec[p].state, 1);
    }
#pragma unroll
    for (int k = 0; k < DYN_C; ++k) {
        const int f = k * DYN_T + tid;
        if (f < lt) {
            const float g = gl[dyn_pos(f)];
            if (!dyn_is_one(g)) {
                typedef float v2f __attribute__((ext_vector_type(2)));
                if (CH == 2) {
                    v2f w;
                    w.x = ld[k][0] * g; w.y = ld[k][CH - 1] * g;
                    reinterpret_cast<v2f*>(xs)[f] = w;
                } else {
                    xs[f] = ld[k][0] * g;
                }
            }
        }
    }
}

// The carries that enter every tile of a signal: blockIdx.y = 0 the release (tiles in order, the
// value at the end of tile t - 1 enters tile t), 1 the attack (tiles from the last to the first).
// carry: four rows of n_tiles words, Cf, Cb, Fin, Bin.
__global__ void __launch_bounds__(DYN_T)
k_dynamics_scan(const int64_t* __restrict__ meta, int n_sig, DynPar par, int64_t* __restrict__ carry,
                const uint32_t* __restrict__ flag, int32_t* __restrict__ sig_state, DynRec* __restrict__ rec,
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
            rec[p] = DynRec{0, 0, 0, bad ? 2 : 0, par.hold};
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
        const DynSeg inc = dyn_wave_scan<true>(s, lane);
        const DynSeg ex = dyn_wave_before<true>(inc, lane);
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
