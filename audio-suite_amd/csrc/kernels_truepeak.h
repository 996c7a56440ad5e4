// kernels_truepeak.h — the device side of msg_truepeak / msg_truepeak_gain (TU
// k_truepeak.hip).  The definition, the tile shape and the table layout are in
// truepeak.h; DESIGN.md "True peak" explains the lane mapping.
//
//   k_truepeak<CH, OS>   one workgroup per tile of TP_TILE positions m' = m + 1 of one
//                        signal: the tile's frames and TP_Z / TP_Z - 1 frames of halo
//                        staged planar per channel, every lane four consecutive
//                        positions of one channel at a time through a register window
//                        of 27 floats, the tile's two maxima (bit patterns) written
//                        (OS = 1: the plain max sweep, no staging)
//   k_truepeak_fin       one wave per signal: the maxima of its tiles, the record
//   k_truepeak_gain      g from the records in float64, x *= (float)g in place
//
// meta: offsets, frames, then n_sig + 1 first tiles (int64 rows).
#pragma once
#include <hip/hip_runtime.h>
#include "truepeak.h"
#include "loudness.h"
#include "sig_tiles.h"

MSG_DEV uint32_t tp_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

template <int CH, int OS>
__global__ void __launch_bounds__(TP_T)
k_truepeak(const float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, const float* __restrict__ tab,
           uint2* __restrict__ part) {
    __shared__ float4 tp_lds4[OS > 1 ? CH * TP_ROW / 4 : 1];
    __shared__ uint32_t red[TP_T / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int p = sig_owner(tile_base, n_sig, tile);
    const int64_t off = meta[p], n = meta[n_sig + p];
    const int64_t f0 = (tile - tile_base[p]) * TP_TILE;   // first position m' and first frame, 0 <= f0 <= n
    uint32_t pk = 0, tp = 0;
    if constexpr (OS == 1) {
        const int64_t left = n - f0;
        const int E = (int)(left < TP_TILE ? left : TP_TILE) * CH;
        const int64_t gbase = (off + f0) * CH;            // 64-bit from the buffer's base
        const int a = (int)(((int64_t)(reinterpret_cast<uintptr_t>(x) >> 2) + gbase) & 3);
        for (int c = tid; 4 * c - a < E; c += TP_T) {
            const float4 v = sig_piece<true, int64_t>(x, gbase, 4 * c - a, 0, E);
            pk = tp_umax(tp_umax(pk, tp_abs_bits(v.x)), tp_abs_bits(v.y));
            pk = tp_umax(tp_umax(pk, tp_abs_bits(v.z)), tp_abs_bits(v.w));
        }
    } else {
        float* X = reinterpret_cast<float*>(tp_lds4);
        const int64_t m_s = f0 - TP_Z;                    // frame of local frame 0
        constexpr int E = (TP_TILE + TP_TAPS - 1) * CH;   // staged floats: every frame the tile's windows read
        const int64_t gbase = (off + m_s) * CH;
        const int a = (int)(((int64_t)(reinterpret_cast<uintptr_t>(x) >> 2) + gbase) & 3);
        const int64_t lo = m_s < 0 ? -m_s * CH : 0;       // zeros outside the signal, by index
        const int64_t hi = (n - m_s) * CH < E ? (n - m_s) * CH : E;
        for (int c = tid; 4 * c - a < E; c += TP_T) {
            const int e0 = 4 * c - a;
            const float4 v = sig_piece<true>(x, gbase, e0, lo, hi);
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int e = e0 + t;
                if (e >= 0 && e < E) X[(e % CH) * TP_ROW + e / CH] = vv[t];
            }
        }
        if (tid < CH) X[tid * TP_ROW + TP_ROW - 1] = 0.0f;   // the last window's 28th float (read, not used)
        __syncthreads();

        // position i of the tile: y_p = sum over q of t_p[q] X[i + 23 - q]; its frame is X[i + TP_Z]
        const int64_t left = n - f0;                       // positions i <= left exist (m <= n - 1)
        const int lim = (int)(left < TP_TILE ? left : TP_TILE);
        constexpr int GPC = TP_TILE / 4;                   // groups of four positions per channel
        const float* __restrict__ taps = tab + tp_tab_at(OS);
#pragma unroll 1
        for (int g = tid; g < GPC * CH; g += TP_T) {
            const int ch = g / GPC, i0 = (g % GPC) * 4;    // ch is uniform over the workgroup
            if (i0 > lim) continue;
            const float4* row = tp_lds4 + ((ch * TP_ROW + i0) >> 2);
            float w[28];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                float4 v = row[k];
                sig_pin(v);
                w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) pk = tp_umax(pk, tp_abs_bits(w[TP_Z + r]));
            float acc[OS - 1][4];
#pragma unroll
            for (int ph = 0; ph < OS - 1; ++ph)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[ph][r] = 0.0f;
#pragma unroll
            for (int q = 0; q < TP_TAPS; ++q)
#pragma unroll
                for (int ph = 0; ph < OS - 1; ++ph) {
                    const float t = taps[ph * TP_TAPS + q];   // wave-uniform
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ph][r] = fmaf(t, w[r + TP_TAPS - 1 - q], acc[ph][r]);
                }
#pragma unroll
            for (int ph = 0; ph < OS - 1; ++ph)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (i0 + r <= lim) tp = tp_umax(tp, tp_abs_bits(acc[ph][r]));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        pk = tp_umax(pk, (uint32_t)__shfl_xor((int)pk, o, 64));
        tp = tp_umax(tp, (uint32_t)__shfl_xor((int)tp, o, 64));
    }
    if (lane == 0) { red[wave][0] = pk; red[wave][1] = tp; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < TP_T / 64; ++w) { pk = tp_umax(pk, red[w][0]); tp = tp_umax(tp, red[w][1]); }
        part[tile] = make_uint2(pk, tp);
    }
}

// one wave per signal: lane i takes tiles i, i + 64, ..; then the xor-butterfly and the record
__global__ void __launch_bounds__(TP_FT)
k_truepeak_fin(const int64_t* __restrict__ meta, int n_sig, const uint2* __restrict__ part, int os,
               TruePeakRec* __restrict__ rec) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t t0 = tile_base[p], t1 = tile_base[p + 1];
    uint32_t pk = 0, tp = 0;
    for (int64_t t = t0 + lane; t < t1; t += TP_FT) {
        const uint2 v = part[t];
        pk = tp_umax(pk, v.x);
        tp = tp_umax(tp, v.y);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        pk = tp_umax(pk, (uint32_t)__shfl_xor((int)pk, o, 64));
        tp = tp_umax(tp, (uint32_t)__shfl_xor((int)tp, o, 64));
    }
    if (lane == 0) {
        TruePeakRec r;
        tp_finish(pk, tp, os, &r);
        rec[p] = r;
    }
}

// step 1 is k_loud_gain's expression (ld_gain_of): with no ceiling binding the scaled
// samples are msg_loudness_gain's to the bit
MSG_DEV double tp_gain_of(const LoudRec* lr, const TruePeakRec* tr, double target, double ceil_tp, double ceil_pk) {
    double g = 1.0;
    if (lr) {
        const double lufs = lr->lufs;
        if (lufs > -__builtin_inf()) g = exp10((target - lufs) / 20.0);
    }
    const double tpk = tr->true_peak, pk = tr->peak;
    if (ceil_tp > 0.0 && g * tpk > ceil_tp) g = ceil_tp / tpk;
    if (ceil_pk > 0.0 && g * pk > ceil_pk) g = ceil_pk / pk;
    return g;
}

// meta: offsets, frames, then n_sig + 1 first tiles of TP_GAIN_TILE frames; grid max(1, tiles)
template <int CH>
__global__ void __launch_bounds__(TP_T)
k_truepeak_gain(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, LoudRec* lrec, TruePeakRec* trec,
                double target, double ceil_tp, double ceil_pk) {
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t tile = blockIdx.x;
    if (tile == 0)                                       // signals without a tile get their gain here
        for (int q = threadIdx.x; q < n_sig; q += TP_T)
            if (tile_base[q + 1] == tile_base[q]) {
                const double g = tp_gain_of(lrec ? lrec + q : nullptr, trec + q, target, ceil_tp, ceil_pk);
                trec[q].gain = g;
                if (lrec) lrec[q].gain = g;
            }
    if (tile >= tile_base[n_sig]) return;
    const int p = sig_owner(tile_base, n_sig, tile);
    const double g = tp_gain_of(lrec ? lrec + p : nullptr, trec + p, target, ceil_tp, ceil_pk);
    if (tile == tile_base[p] && threadIdx.x == 0) {
        trec[p].gain = g;
        if (lrec) lrec[p].gain = g;
    }
    sig_scale<CH, TP_T, TP_GAIN_PER>(x, meta, n_sig, p, tile, (float)g);
}
