// kernels_limit.h — the device side of msg_limit (TU k_limit.hip).  The definition, the
// tile shapes and the record are in limit.h; DESIGN.md "4f. Limiter" explains the lane mapping.
//
//   k_limit_env<CH, OS>   one workgroup per tile of LIM_ENV_TILE frames of one signal:
//                         k_truepeak's staging (a planar LDS row per channel through
//                         sig_piece) and register window (four positions per lane, 27 floats
//                         pinned by sig_pin), the maximum of every position over phases and
//                         channels left in LDS, then r of every frame from its sample and
//                         its two positions written to the scratch, and the tile's NaN flag
//                         (OS = 1: the plain per-frame sweep, no staging)
//   k_limit_state         one wave per signal: skipped (measured under the ceiling), NaN
//                         (the fold of its tiles' flags) or to be run
//   k_limit_apply<CH, T>  one workgroup per tile of lim_tile(L) frames: r staged with
//                         lim_halo(L) frames per side (1 outside the signal) and one bit
//                         per staged float for r < 1; a tile without such a bit returns.
//                         The hold is a sliding minimum in place by doubling shifts; the
//                         reach of a frame is a difference of prefix counts over the bits;
//                         a lane runs the FIR for four consecutive frames through a window
//                         of two 16-byte LDS reads, the weights wave-uniform 16-byte loads;
//                         then g x on the tile's own frames, and the tile's least gain
//                         and count
//   k_limit_fin           one wave per signal: the fold of its tiles, the record
//
// meta (int64): offsets, frames, n_sig + 1 first apply tiles, n_sig first scratch floats
// (multiples of 4), n_sig + 1 first envelope tiles.
#pragma once
#include <hip/hip_runtime.h>
#include "limit.h"
#include "sig_tiles.h"

template <int CH, int OS>
__global__ void __launch_bounds__(LIM_ENV_T)
k_limit_env(const float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, const float* __restrict__ tab,
            float c32, const TruePeakRec* __restrict__ tprec, float* __restrict__ rbuf, uint32_t* __restrict__ nanpart) {
    __shared__ float4 lim_x4[OS > 1 ? CH * LIM_ENV_ROW / 4 : 1];
    __shared__ uint32_t lim_pos[OS > 1 ? LIM_ENV_TILE + 4 : 1];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t* tile_base = meta + 4 * (int64_t)n_sig + 1;
    const int p = sig_owner(tile_base, n_sig, tile);
    if (tprec && tprec[p].true_peak <= (double)c32) return;       // measured under the ceiling: wave-uniform
    const int64_t off = meta[p], n = meta[n_sig + p], rb = meta[3 * (int64_t)n_sig + 1 + p];
    const int64_t f0 = (tile - tile_base[p]) * LIM_ENV_TILE;        // first frame and first position, f0 < n
    const int64_t left = n - f0;
    const int cnt = (int)(left < LIM_ENV_TILE ? left : LIM_ENV_TILE);   // frames of this tile
    float* rs = rbuf + rb + f0;
    int nan = 0;
    if constexpr (OS == 1) {
        const float* xs = x + (off + f0) * CH;                      // 64-bit from the buffer's base
        for (int i = tid; i < cnt; i += LIM_ENV_T) {
            uint32_t e;
            if (CH == 2) {
                typedef float v2f __attribute__((ext_vector_type(2)));
                const v2f v = reinterpret_cast<const v2f*>(xs)[i];
                e = lim_umax(tp_abs_bits(v.x), tp_abs_bits(v.y));
            } else {
                e = tp_abs_bits(xs[i]);
            }
            nan |= e > LIM_INF;
            rs[i] = lim_demand(e, c32);
        }
    } else {
        float* X = reinterpret_cast<float*>(lim_x4);
        const int64_t m_s = f0 - TP_Z;                              // frame of local frame 0
        constexpr int E = (LIM_ENV_TILE + 27) * CH;                 // staged floats: positions 0 .. TILE + 3
        const int64_t gbase = (off + m_s) * CH;
        const int a = (int)(((int64_t)(reinterpret_cast<uintptr_t>(x) >> 2) + gbase) & 3);
        const int64_t lo = m_s < 0 ? -m_s * CH : 0;                 // zeros outside the signal, by index
        const int64_t hi = (n - m_s) * CH < E ? (n - m_s) * CH : E;
        for (int c = tid; 4 * c - a < E; c += LIM_ENV_T) {
            const int e0 = 4 * c - a;
            const float4 v = sig_piece<true>(x, gbase, e0, lo, hi);
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int e = e0 + t;
                if (e >= 0 && e < E) X[(e % CH) * LIM_ENV_ROW + e / CH] = vv[t];
            }
        }
        if (tid < CH) X[tid * LIM_ENV_ROW + LIM_ENV_ROW - 1] = 0.0f;   // the last window's 28th float (read, not used)
        __syncthreads();

        // position i of the tile: y_p = sum over q of t_p[q] X[i + 23 - q], the value between frames
        // i - 1 and i; frame i is X[i + TP_Z].  Frames 0 .. cnt - 1 read positions 0 .. cnt, all of
        // them positions of the signal (f0 + cnt <= n); a group's later positions are never read.
        constexpr int GP = LIM_ENV_TILE / 4 + 1;                    // groups of four positions
        const float* __restrict__ taps = tab + tp_tab_at(OS);
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
#pragma unroll 1
            for (int g = tid; g < GP; g += LIM_ENV_T) {             // the same lane has group g in both channels
                const int i0 = 4 * g;
                if (i0 > cnt) continue;
                const float4* row = lim_x4 + ((ch * LIM_ENV_ROW + i0) >> 2);
                float w[28];
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    float4 v = row[k];
                    sig_pin(v);
                    w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
                }
                float acc[OS - 1][4];
#pragma unroll
                for (int ph = 0; ph < OS - 1; ++ph)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ph][r] = 0.0f;
#pragma unroll
                for (int q = 0; q < TP_TAPS; ++q)
#pragma unroll
                    for (int ph = 0; ph < OS - 1; ++ph) {
                        const float t = taps[ph * TP_TAPS + q];     // wave-uniform
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[ph][r] = fmaf(t, w[r + TP_TAPS - 1 - q], acc[ph][r]);
                    }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    uint32_t m = ch == 0 ? 0u : lim_pos[i0 + r];
#pragma unroll
                    for (int ph = 0; ph < OS - 1; ++ph) m = lim_umax(m, tp_abs_bits(acc[ph][r]));
                    lim_pos[i0 + r] = m;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < cnt; i += LIM_ENV_T) {
            uint32_t e = lim_umax(lim_pos[i], lim_pos[i + 1]);
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) e = lim_umax(e, tp_abs_bits(X[ch * LIM_ENV_ROW + TP_Z + i]));
            nan |= e > LIM_INF;
            rs[i] = lim_demand(e, c32);
        }
    }
    nan = __syncthreads_or(nan);
    if (tid == 0) nanpart[tile] = nan ? 1u : 0u;
}

// one wave per signal
__global__ void __launch_bounds__(LIM_FT)
k_limit_state(const int64_t* __restrict__ meta, int n_sig, float c32, const TruePeakRec* __restrict__ tprec,
              const uint32_t* __restrict__ nanpart, int32_t* __restrict__ state) {
    const int p = blockIdx.x, lane = threadIdx.x;
    if (tprec && tprec[p].true_peak <= (double)c32) {
        if (lane == 0) state[p] = LIM_SKIP;
        return;
    }
    const int64_t* tile_base = meta + 4 * (int64_t)n_sig + 1;
    uint32_t nan = 0;
    for (int64_t t = tile_base[p] + lane; t < tile_base[p + 1]; t += LIM_FT) nan |= nanpart[t];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nan |= (uint32_t)__shfl_xor((int)nan, o, 64);
    if (lane == 0) state[p] = nan ? LIM_NAN : LIM_RUN;
}

// A[j] = min(A[j], A[j + s]) for every j < W with j + s < W, in place: rounds of 8 T floats in
// ascending order, each reading before a barrier and writing after it.  A round reads nothing an
// earlier round wrote (its floats and their partners lie above) and a later round writes only
// after its own barrier, which every thread reaches after this round's reads.
template <int T>
MSG_DEV void lim_min_pass(float* A, int W, int s) {
    for (int base = 0; base < W; base += 8 * T) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j = base + k * T + (int)threadIdx.x;
            v[k] = 1.0f;
            if (j < W) {
                v[k] = A[j];
                if (j + s < W) v[k] = fminf(v[k], A[j + s]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j = base + k * T + (int)threadIdx.x;
            if (j < W) A[j] = v[k];
        }
    }
    __syncthreads();
}

// staged floats below index j with r < 1: the prefix count of j's word and the bits below j in it
MSG_DEV uint32_t lim_below(const uint64_t* bits, const uint32_t* pre, int j) {
    return pre[j >> 6] + (uint32_t)__popcll(bits[j >> 6] & ((1ull << (j & 63)) - 1ull));
}

template <int CH, int T>
__global__ void __launch_bounds__(T)
k_limit_apply(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, const float4* __restrict__ w4, int L,
              const int32_t* __restrict__ state, const float* __restrict__ rbuf, uint2* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char lim_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int p = sig_owner(tile_base, n_sig, tile);
    if (state[p] != LIM_RUN) return;                                // wave-uniform
    const int TILE = lim_tile(L), HALO = lim_halo(L), W = TILE + 2 * HALO, NW = (W + 63) / 64 + 1;
    float* A = reinterpret_cast<float*>(lim_smem);
    uint64_t* bits = reinterpret_cast<uint64_t*>(lim_smem + (size_t)W * 4);
    uint32_t* pre = reinterpret_cast<uint32_t*>(lim_smem + (size_t)W * 4 + (((size_t)NW * 8 + 15) & ~(size_t)15));
    uint32_t* red = reinterpret_cast<uint32_t*>(lim_smem + (size_t)W * 4 + 2 * (((size_t)NW * 8 + 15) & ~(size_t)15));
    const int64_t off = meta[p], n = meta[n_sig + p], rb = meta[3 * (int64_t)n_sig + 1 + p];
    const int64_t f0 = (tile - tile_base[p]) * TILE;                // f0 < n
    const int64_t left = n - f0;
    const int cnt = (int)(left < TILE ? left : TILE);
    const float* rs = rbuf + rb;

    // staged float a is r of frame f0 - HALO + a; every wave takes 64 consecutive floats and
    // writes their "r < 1" bits as one word (words past W hold zeros)
    int any = 0;
    for (int base = 0; base < 64 * NW; base += T) {
        const int a = base + tid;
        const int64_t f = f0 - HALO + a;
        float v = 1.0f;
        if (a < W) {
            if (f >= 0 && f < n) v = rs[f];
            A[a] = v;
        }
        const uint64_t m = __ballot(v < 1.0f);
        if (lane == 0 && (a >> 6) < NW) bits[a >> 6] = m;
        any |= m != 0;
    }
    if (!__syncthreads_or(any)) {                                   // nothing in reach of this tile
        if (tid == 0) part[tile] = make_uint2(LIM_ONE, 0u);
        return;
    }
    // pre[k]: the set bits of the words below k (NW <= T): a scan per wave, then the waves' totals
    {
        const uint32_t c = tid < NW ? (uint32_t)__popcll(bits[tid]) : 0u;
        uint32_t inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) red[wave] = inc;
        __syncthreads();
        uint32_t before = 0;
        for (int k = 0; k < wave; ++k) before += red[k];
        if (tid < NW) pre[tid] = before + inc - c;
        __syncthreads();
    }
    // the hold: A[a] = min of the staged r over [a, a + 2 (L + TP_Z)], which is h of frame f0 - L + a
    const int WN = 2 * (L + TP_Z) + 1;
    for (int len = 1; len < WN;) {
        const int s = len < WN - len ? len : WN - len;
        lim_min_pass<T>(A, W, s);
        len += s;
    }

    // frame i of the tile: s = sum over k of w[k] A[i + k]; in reach when a bit lies in staged
    // [i, i + 2 HALO].  A lane takes frames 4 g .. 4 g + 3 and slides two 16-byte reads.
    const float4* A4 = reinterpret_cast<const float4*>(A);
    const int K4 = (2 * L + 1 + 3) / 4;
    float* xs = x + (off + f0) * CH;                                // 64-bit from the buffer's base
    uint32_t g_min = LIM_ONE, count = 0;
    for (int g = tid; 4 * g < cnt; g += T) {
        const int i0 = 4 * g;
        if (lim_below(bits, pre, i0 + 3 + 2 * HALO + 1) == lim_below(bits, pre, i0)) continue;
        float4 a = A4[g];
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
#pragma unroll 2
        for (int k4 = 0; k4 < K4; ++k4) {
            const float4 b = A4[g + k4 + 1];
            const float4 ww = w4[k4];                               // wave-uniform
            acc0 = fmaf(ww.x, a.x, acc0); acc0 = fmaf(ww.y, a.y, acc0); acc0 = fmaf(ww.z, a.z, acc0); acc0 = fmaf(ww.w, a.w, acc0);
            acc1 = fmaf(ww.x, a.y, acc1); acc1 = fmaf(ww.y, a.z, acc1); acc1 = fmaf(ww.z, a.w, acc1); acc1 = fmaf(ww.w, b.x, acc1);
            acc2 = fmaf(ww.x, a.z, acc2); acc2 = fmaf(ww.y, a.w, acc2); acc2 = fmaf(ww.z, b.x, acc2); acc2 = fmaf(ww.w, b.y, acc2);
            acc3 = fmaf(ww.x, a.w, acc3); acc3 = fmaf(ww.y, b.x, acc3); acc3 = fmaf(ww.z, b.y, acc3); acc3 = fmaf(ww.w, b.z, acc3);
            a = b;
        }
        const float4 rv = *reinterpret_cast<const float4*>(rs + f0 + i0);   // the scratch is padded to whole pieces
        const float sv[4] = {acc0, acc1, acc2, acc3}, rr[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + r;
            if (i >= cnt || lim_below(bits, pre, i + 2 * HALO + 1) == lim_below(bits, pre, i)) continue;
            const float gf = lim_gain(sv[r], rr[r]);
            const uint32_t gb = tp_abs_bits(gf);
            g_min = gb < g_min ? gb : g_min;
            ++count;
            if (CH == 2) {
                typedef float v2f __attribute__((ext_vector_type(2)));
                v2f* q = reinterpret_cast<v2f*>(xs) + i;
                v2f v = *q;
                v.x *= gf; v.y *= gf;
                *q = v;
            } else {
                xs[i] *= gf;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t og = (uint32_t)__shfl_xor((int)g_min, o, 64);
        g_min = og < g_min ? og : g_min;
        count += (uint32_t)__shfl_xor((int)count, o, 64);
    }
    __syncthreads();                                                // red was the scan's
    if (lane == 0) { red[2 * wave] = g_min; red[2 * wave + 1] = count; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < T / 64; ++k) {
            g_min = red[2 * k] < g_min ? red[2 * k] : g_min;
            count += red[2 * k + 1];
        }
        part[tile] = make_uint2(g_min, count);
    }
}

// one wave per signal: lane i takes tiles i, i + 64, ..; then the xor-butterfly and the record
__global__ void __launch_bounds__(LIM_FT)
k_limit_fin(const int64_t* __restrict__ meta, int n_sig, int L, const int32_t* __restrict__ state,
            const uint2* __restrict__ part, LimitRec* __restrict__ rec) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int st = state[p];
    uint32_t g_min = LIM_ONE;
    uint64_t count = 0;
    if (st == LIM_RUN)
        for (int64_t t = tile_base[p] + lane; t < tile_base[p + 1]; t += LIM_FT) {
            const uint2 v = part[t];
            g_min = v.x < g_min ? v.x : g_min;
            count += v.y;
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t og = (uint32_t)__shfl_xor((int)g_min, o, 64);
        g_min = og < g_min ? og : g_min;
        count += sig_shfl64(count, o);
    }
    if (lane == 0) {
        LimitRec r;
        lim_finish(st, g_min, (int64_t)count, L, &r);
        rec[p] = r;
    }
}
