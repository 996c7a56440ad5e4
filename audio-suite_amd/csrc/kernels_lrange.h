// kernels_lrange.h — the device side of msg_loudness_range (TU k_loudness.hip), after the
// two sweeps of kernels_loudness.h have left one energy per tile in `part`.  The definition
// is in lrange.h; DESIGN.md "Loudness range" explains the select.
//
//   k_lrange_hops   one workgroup per signal: H_k, the tiles of hop k added in order
//                   (ld_block_z's fold), written at the signal's place in the hop buffer
//   k_lrange        one workgroup of LR_T threads per signal: the momentary maximum, the
//                   short-term windows (each the stated left fold of 30 hop sums, kept as
//                   one double per window), the absolute and the relative gate in the stated
//                   fold order, then both order statistics by a radix select over the raw
//                   bit patterns of the kept windows, and the record
//
// The select: a window outside the gates is overwritten by LR_DROPPED, which lies above
// every kept pattern (z >= 0, so unsigned order is numeric order), and the k-th smallest
// pattern, k < n_kept, is found byte by byte from the top: an LDS histogram of the byte
// among the windows that share the bytes found so far (integer atomics), a scan of the
// 256 counts by one wave, eight passes.  Both ranks run in one sweep with a histogram each.
// Exact for any number of windows; no floating-point atomics.
//
// meta: offsets, frames, n_sig + 1 first tiles (msg_loudness's rows), then per signal its
// first double in the hop buffer and its first double in the window scratch.
#pragma once
#include <hip/hip_runtime.h>
#include "lrange.h"
#include "sig_tiles.h"

__global__ void __launch_bounds__(LR_T)
k_lrange_hops(const int64_t* __restrict__ meta, int n_sig, int64_t hop, int tph, const double* __restrict__ part,
              double* __restrict__ hops_out) {
    const int p = blockIdx.x;
    const int64_t hops = meta[n_sig + p] / hop, t0 = meta[2 * (int64_t)n_sig + p];
    double* H = hops_out + meta[3 * (int64_t)n_sig + 1 + p];
    for (int64_t k = threadIdx.x; k < hops; k += LR_T) {
        const int64_t tb = t0 + k * tph;
        double a = part[2 * tb];
        for (int i = 1; i < tph; ++i) a += part[2 * (tb + i)];
        H[k] = a;
    }
}

// the inclusive scan of one wave's values, lane by lane upward
MSG_DEV uint32_t lr_wave_scan(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ void __launch_bounds__(LR_T)
k_lrange(const int64_t* __restrict__ meta, int n_sig, int64_t hop, const double* __restrict__ hops_in,
         double* __restrict__ win, LRangeRec* __restrict__ rec) {
    __shared__ double red_s[LR_T / 64], red_m[LR_T / 64], red_z[LR_T / 64];
    __shared__ int64_t red_c[LR_T / 64];
    __shared__ uint32_t hist[2][256];
    __shared__ uint64_t sel_prefix[2], sel_rank[2];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t hops = meta[n_sig + p] / hop;
    const double* H = hops_in + meta[3 * (int64_t)n_sig + 1 + p];
    double* Z = win + meta[4 * (int64_t)n_sig + 1 + p];
    uint64_t* ZB = reinterpret_cast<uint64_t*>(Z);
    const int64_t nb = lr_blocks(hops), ns = lr_windows(hops);

    // maxima, the windows, the absolute gate's sum and count
    double zm = 0.0, zsm = 0.0, s1 = 0.0;
    int64_t c1 = 0;
    for (int64_t j = tid; j < nb; j += LR_T) {
        const double z = lr_block_z(H, j, hop);
        zm = z > zm ? z : zm;
    }
    for (int64_t i = tid; i < ns; i += LR_T) {
        const double z = lr_window_z(H, i, hop);
        Z[i] = z;
        zsm = z > zsm ? z : zsm;
        if (ld_level(z) > LR_ABS) { s1 += z; ++c1; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        c1 += sig_shfl64(c1, o);
        const double a = __shfl_xor(zm, o, 64), b = __shfl_xor(zsm, o, 64);
        zm = zm > a ? zm : a;
        zsm = zsm > b ? zsm : b;
    }
    if (lane == 0) { red_s[wave] = s1; red_c[wave] = c1; red_m[wave] = zm; red_z[wave] = zsm; }
    __syncthreads();
    s1 = red_s[0]; c1 = red_c[0]; zm = red_m[0]; zsm = red_z[0];
    for (int w = 1; w < LR_T / 64; ++w) {                 // the waves in order
        s1 += red_s[w];
        c1 += red_c[w];
        zm = zm > red_m[w] ? zm : red_m[w];
        zsm = zsm > red_z[w] ? zsm : red_z[w];
    }
    const double gate = c1 ? ld_level(s1 / (double)c1) - LR_REL : -__builtin_inf();
    __syncthreads();                                      // red_c is written again below

    // the relative gate: a thread revisits its own windows and drops those outside
    int64_t c2 = 0;
    if (c1)
        for (int64_t i = tid; i < ns; i += LR_T) {
            const double l = ld_level(Z[i]);
            if (l > LR_ABS && l > gate) ++c2; else ZB[i] = LR_DROPPED;
        }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c2 += sig_shfl64(c2, o);
    if (lane == 0) red_c[wave] = c2;
    if (tid < 2) sel_prefix[tid] = 0;
    __syncthreads();                                      // and every thread's patterns are in place
    c2 = red_c[0];
    for (int w = 1; w < LR_T / 64; ++w) c2 += red_c[w];
    if (tid == 0) { sel_rank[0] = (uint64_t)lr_rank_lo(c2 ? c2 : 1); sel_rank[1] = (uint64_t)lr_rank_hi(c2 ? c2 : 1); }

    if (c2) {                                             // uniform over the workgroup
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[0][tid] = 0;
            hist[1][tid] = 0;
            __syncthreads();
            const uint64_t p0 = sel_prefix[0], p1 = sel_prefix[1];
            for (int64_t i = tid; i < ns; i += LR_T) {
                const uint64_t v = ZB[i], top = shift == 56 ? 0 : v >> (shift + 8);
                const uint32_t b = (uint32_t)(v >> shift) & 255u;
                if (top == p0) atomicAdd(&hist[0][b], 1u);
                if (top == p1) atomicAdd(&hist[1][b], 1u);
            }
            __syncthreads();
            if (wave < 2) {                               // wave q scans histogram q: lane l holds bins 4 l .. 4 l + 3
                const uint32_t h0 = hist[wave][4 * lane], h1 = hist[wave][4 * lane + 1], h2 = hist[wave][4 * lane + 2],
                               h3 = hist[wave][4 * lane + 3];
                const uint32_t incl = lr_wave_scan(h0 + h1 + h2 + h3, lane), excl = incl - (h0 + h1 + h2 + h3);
                const uint64_t k = sel_rank[wave];
                if (k >= excl && k < incl) {              // one lane: the counts below the rank end inside its bins
                    uint32_t r = (uint32_t)(k - excl);
                    int b = 4 * lane;
                    if (r >= h0) { r -= h0; ++b; if (r >= h1) { r -= h1; ++b; if (r >= h2) { r -= h2; ++b; } } }
                    sel_prefix[wave] = (sel_prefix[wave] << 8) | (uint64_t)b;
                    sel_rank[wave] = r;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        LRangeRec r;
        lr_finish(&r, zm, zsm, gate, __longlong_as_double((long long)sel_prefix[0]),
                  __longlong_as_double((long long)sel_prefix[1]), nb, ns, c1, c2);
        rec[p] = r;
    }
}
