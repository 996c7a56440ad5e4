// kernels_resample.h — the device side of msg_resample (TU k_resample.hip): a
// float32 polyphase FIR on ragged batches of mono or interleaved-stereo signals.
// Shapes, table layouts and the lane mappings are described in resample.h.
//
// meta: four rows of n_sig int64 — input frame offsets, input frames, output
// frame offsets, first tile of each signal.  One workgroup per output tile.
#pragma once
#include <hip/hip_runtime.h>
#include "resample.h"
#include "sig_tiles.h"

// The signal that owns `tile`: the last one whose first tile is <= tile (signals without
// output own no tile and are never the last such).  sig_owner's result by another form of
// the search, kept because the resampler's kernels compile differently through sig_owner.
__device__ inline int rs_signal(const int64_t* __restrict__ tile_base, int n_sig, int64_t tile) {
    int lo = 0, hi = n_sig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_base[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Integer decimation, up == 1.  Threads: RS_DTILE / RS_RB per channel.
template <int DOWN, int CH>
__global__ void __launch_bounds__(RS_DTILE / RS_RB * CH)
k_resample_dec(const float* __restrict__ x, float* __restrict__ y, const int64_t* __restrict__ meta, int n_sig,
               const float* __restrict__ trow, int A, int ROW, int half, int K) {
    extern __shared__ float4 rs_lds4[];
    float* X = reinterpret_cast<float*>(rs_lds4);
    constexpr int NT = RS_DTILE / RS_RB * CH;
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int s = rs_signal(meta + 3 * (int64_t)n_sig, n_sig, tile);
    const int64_t in_off = meta[s], n = meta[n_sig + s], out_off = meta[2 * (int64_t)n_sig + s];
    const int64_t k0 = (tile - meta[3 * (int64_t)n_sig + s]) * RS_DTILE;
    const int64_t m_s = k0 * DOWN + half - (K - 1);       // input frame of local frame 0
    const int E = (RS_DTILE + A) * DOWN * CH;             // staged floats: every column the FIR reads
    const int64_t gbase = (in_off + m_s) * CH;
    const int a = (int)(((int64_t)(reinterpret_cast<uintptr_t>(x) >> 2) + gbase) & 3);
    const int64_t lo = m_s < 0 ? -m_s * CH : 0;
    const int64_t hi = (n - m_s) * CH < E ? (n - m_s) * CH : E;
    for (int c = tid; 4 * c - a < E; c += NT) {
        const int e0 = 4 * c - a;
        const float4 v = sig_piece(x, gbase, e0, lo, hi);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int e = e0 + t;
            if (e >= 0 && e < E) {
                const int j = e / CH, ch = e % CH;
                X[(ch * DOWN + j % DOWN) * ROW + j / DOWN] = vv[t];
            }
        }
    }
    __syncthreads();
    const int ch = tid / (RS_DTILE / RS_RB), i0 = (tid % (RS_DTILE / RS_RB)) * RS_RB;
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, acc3 = 0.0f;
#pragma unroll
    for (int r = 0; r < DOWN; ++r) {
        const float4* row = rs_lds4 + (((ch * DOWN + r) * ROW + i0) >> 2);
        const float* tr = trow + r * A;                    // wave-uniform taps
        float4 w0 = row[0], w1;
        sig_pin(w0);
        // four taps against the window w0 | w1; the two halves swap roles (A is a multiple of 8)
#define RS_DEC_STEP(W0, W1, AT)                                                                                        \
        {                                                                                                              \
            W1 = row[((AT) >> 2) + 1];                                                                                 \
            sig_pin(W1);                                                                                                \
            const float t0 = tr[AT], t1 = tr[(AT) + 1], t2 = tr[(AT) + 2], t3 = tr[(AT) + 3];                          \
            acc0 = fmaf(t0, W0.x, acc0); acc1 = fmaf(t0, W0.y, acc1); acc2 = fmaf(t0, W0.z, acc2); acc3 = fmaf(t0, W0.w, acc3); \
            acc0 = fmaf(t1, W0.y, acc0); acc1 = fmaf(t1, W0.z, acc1); acc2 = fmaf(t1, W0.w, acc2); acc3 = fmaf(t1, W1.x, acc3); \
            acc0 = fmaf(t2, W0.z, acc0); acc1 = fmaf(t2, W0.w, acc1); acc2 = fmaf(t2, W1.x, acc2); acc3 = fmaf(t2, W1.y, acc3); \
            acc0 = fmaf(t3, W0.w, acc0); acc1 = fmaf(t3, W1.x, acc1); acc2 = fmaf(t3, W1.y, acc2); acc3 = fmaf(t3, W1.z, acc3); \
        }
        for (int a0 = 0; a0 < A; a0 += 8) {
            RS_DEC_STEP(w0, w1, a0)
            RS_DEC_STEP(w1, w0, a0 + 4)
        }
#undef RS_DEC_STEP
    }
    // outputs through LDS: interleaved frames leave in whole coalesced rows
    __syncthreads();
    X[(i0 + 0) * CH + ch] = acc0;
    X[(i0 + 1) * CH + ch] = acc1;
    X[(i0 + 2) * CH + ch] = acc2;
    X[(i0 + 3) * CH + ch] = acc3;
    __syncthreads();
    const int64_t n_out = rs_out_len(n, 1, DOWN);
    const int64_t left = n_out - k0;
    const int cnt = (int)(left < RS_DTILE ? left : RS_DTILE) * CH;
    float* yo = y + (out_off + k0) * CH;
    for (int e = tid; e < cnt; e += NT) yo[e] = X[e];
}

// Any ratio.  Threads: RS_LANES; lanes l < L in turns.
template <int CH>
__global__ void __launch_bounds__(RS_LANES)
k_resample_gen(const float* __restrict__ x, float* __restrict__ y, const int64_t* __restrict__ meta, int n_sig,
               const float* __restrict__ tab, int up, int down, int half, int Q4, int L, int step, int span) {
    extern __shared__ float4 rs_lds4[];
    float* X = reinterpret_cast<float*>(rs_lds4);
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int s = rs_signal(meta + 3 * (int64_t)n_sig, n_sig, tile);
    const int64_t in_off = meta[s], n = meta[n_sig + s], out_off = meta[2 * (int64_t)n_sig + s];
    const int64_t k0 = (tile - meta[3 * (int64_t)n_sig + s]) * ((int64_t)RS_RB * L);
    const int64_t m_s = (k0 * down + half) / up - (Q4 - 1);   // input frame of local frame 0
    const int E = span * CH;
    const int64_t gbase = (in_off + m_s) * CH;
    const int a = (int)(((int64_t)(reinterpret_cast<uintptr_t>(x) >> 2) + gbase) & 3);
    const int64_t lo = m_s < 0 ? -m_s * CH : 0;
    const int64_t hi = (n - m_s) * CH < E ? (n - m_s) * CH : E;
    // local float e lies at X[e + a]: piece c is the aligned float4 X[4c .. 4c + 3]
    for (int c = tid; 4 * c - a < E; c += RS_LANES) rs_lds4[c] = sig_piece(x, gbase, 4 * c - a, lo, hi);
    __syncthreads();
    const int64_t n_out = rs_out_len(n, up, down);
    for (int l = tid; l < L; l += RS_LANES) {
        const int64_t k = k0 + l;
        const int64_t num = k * down + half, m0 = num / up;
        const int ph = (int)(num - m0 * up);
        const int j0 = (int)(m0 - m_s);
        const float4* t4 = reinterpret_cast<const float4*>(tab + (int64_t)ph * Q4);
        float acc[RS_RB][CH];
#pragma unroll
        for (int r = 0; r < RS_RB; ++r)
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[r][c] = 0.0f;
        for (int q0 = 0; q0 < Q4; q0 += 4) {
            const float4 t = t4[q0 >> 2];
#pragma unroll
            for (int r = 0; r < RS_RB; ++r) {
                const float* xb = X + a + (j0 + r * step - q0) * CH;   // x[m0 - q0] of output r
                if (CH == 2) {
                    const float2 v0 = *reinterpret_cast<const float2*>(xb), v1 = *reinterpret_cast<const float2*>(xb - 2);
                    const float2 v2 = *reinterpret_cast<const float2*>(xb - 4), v3 = *reinterpret_cast<const float2*>(xb - 6);
                    acc[r][0] = fmaf(t.x, v0.x, acc[r][0]); acc[r][CH - 1] = fmaf(t.x, v0.y, acc[r][CH - 1]);
                    acc[r][0] = fmaf(t.y, v1.x, acc[r][0]); acc[r][CH - 1] = fmaf(t.y, v1.y, acc[r][CH - 1]);
                    acc[r][0] = fmaf(t.z, v2.x, acc[r][0]); acc[r][CH - 1] = fmaf(t.z, v2.y, acc[r][CH - 1]);
                    acc[r][0] = fmaf(t.w, v3.x, acc[r][0]); acc[r][CH - 1] = fmaf(t.w, v3.y, acc[r][CH - 1]);
                } else {
                    acc[r][0] = fmaf(t.x, xb[0], acc[r][0]);
                    acc[r][0] = fmaf(t.y, xb[-1], acc[r][0]);
                    acc[r][0] = fmaf(t.z, xb[-2], acc[r][0]);
                    acc[r][0] = fmaf(t.w, xb[-3], acc[r][0]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RS_RB; ++r) {
            const int64_t kr = k + (int64_t)r * L;
            if (kr < n_out) {
#pragma unroll
                for (int c = 0; c < CH; ++c) y[(out_off + kr) * CH + c] = acc[r][c];
            }
        }
    }
}
