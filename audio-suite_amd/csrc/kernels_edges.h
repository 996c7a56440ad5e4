// kernels_edges.h — the device side of msg_edges (TU k_edges.hip).  The definition, the
// tile shapes and the record are in edges.h; DESIGN.md "4i. Edges".
//
//   k_edges_init        one lane per signal: first = EDG_NO_FIRST, last = -1 (only with a trim)
//   k_edges_find<CH>    one workgroup per tile of EDG_TILE frames of one signal (only with a
//                       trim): 16-byte pieces through sig_piece, per lane the least and
//                       greatest sound frame of its pieces, a min / max butterfly per wave, the
//                       waves folded in LDS, then one atomic min and one atomic max per tile
//                       on the signal's record.  Minimum and maximum are free of order, so the
//                       record is exact whatever order the tiles finish in; a silent tile
//                       issues no atomic.
//   k_edges_span        one lane per signal: start, end and the clipped lengths (edg_span)
//   k_edges_apply<CH>   one workgroup per tile of EDG_APPLY_TILE frames of a fade-in, a
//                       fade-out or a crossfade.  The host sizes the grid from bounds that
//                       need no measurement (edg_apply_tiles); the lengths and places come
//                       from the device record, and a tile past them returns.
//
// meta (int64): offsets, frames, n_sig + 1 first find tiles, n_sig + 1 first apply tiles.
#pragma once
#include <hip/hip_runtime.h>
#include "edges.h"
#include "sig_tiles.h"

__global__ void __launch_bounds__(EDG_T)
k_edges_init(int n_sig, EdgesRec* __restrict__ rec) {
    const int p = blockIdx.x * EDG_T + threadIdx.x;
    if (p < n_sig) {
        rec[p].first = EDG_NO_FIRST;
        rec[p].last = -1;
    }
}

template <int CH>
__global__ void __launch_bounds__(EDG_T)
k_edges_find(const float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, float thr,
             EdgesRec* __restrict__ rec) {
    __shared__ int edg_mn[EDG_T / 64], edg_mx[EDG_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int p = sig_owner(tile_base, n_sig, tile);
    const int64_t off = meta[p], n = meta[n_sig + p];
    const int64_t f0 = (tile - tile_base[p]) * EDG_TILE;            // f0 < n
    const int64_t left = n - f0;
    const int cnt = (int)(left < EDG_TILE ? left : EDG_TILE);       // frames of this tile
    const int E = cnt * CH;                                         // its floats: local float e is frame e / CH
    const int64_t gbase = (off + f0) * CH;
    const int a = (int)(((int64_t)(reinterpret_cast<uintptr_t>(x) >> 2) + gbase) & 3);
    int mn = INT32_MAX, mx = -1;
    for (int c = tid; 4 * c - a < E; c += EDG_T) {
        const int e0 = 4 * c - a;
        const float4 v = sig_piece(x, gbase, e0, 0, E);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int e = e0 + t;
            // by index as well: a float outside the tile reads as zero, and thr may be zero
            if (e >= 0 && e < E && fabsf(vv[t]) >= thr) {
                const int f = e / CH;
                mn = f < mn ? f : mn;
                mx = f > mx ? f : mx;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int on = __shfl_xor(mn, o, 64), ox = __shfl_xor(mx, o, 64);
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
    }
    if (lane == 0) { edg_mn[wave] = mn; edg_mx[wave] = mx; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < EDG_T / 64; ++k) {
            mn = edg_mn[k] < mn ? edg_mn[k] : mn;
            mx = edg_mx[k] > mx ? edg_mx[k] : mx;
        }
        if (mx >= 0) {
            atomicMin(reinterpret_cast<long long*>(&rec[p].first), (long long)(f0 + mn));
            atomicMax(reinterpret_cast<long long*>(&rec[p].last), (long long)(f0 + mx));
        }
    }
}

__global__ void __launch_bounds__(EDG_T)
k_edges_span(const int64_t* __restrict__ meta, int n_sig, EdgesPar par, EdgesRec* __restrict__ rec) {
    const int p = blockIdx.x * EDG_T + threadIdx.x;
    if (p >= n_sig) return;
    int64_t first = 0, last = -1;
    if (par.sides) {
        first = rec[p].first;
        last = rec[p].last;
    }
    rec[p] = edg_span(meta[n_sig + p], first, last, par);
}

template <int CH>
__global__ void __launch_bounds__(EDG_T)
k_edges_apply(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, EdgesPar par,
              const EdgesRec* __restrict__ rec) {
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t* tile_base = meta + 3 * (int64_t)n_sig + 1;
    const int p = sig_owner(tile_base, n_sig, tile);
    const int64_t off = meta[p], n = meta[n_sig + p];
    const EdgesRec r = rec[p];
    int64_t j = tile - tile_base[p];
    const int64_t tin = edg_in_tiles(par, n);
    const bool fade_out = j >= tin;                                 // wave-uniform
    if (fade_out) j -= tin;
    // the region's frames as applied and its first frame, [at, at + F) inside [start, end)
    const int64_t F = par.loop >= 0 ? r.loop : (fade_out ? r.fade_out : r.fade_in);
    const int64_t at = fade_out ? r.end - F : r.start;
    float* xs = x + off * CH;                                       // 64-bit from the buffer's base
#pragma unroll
    for (int i = 0; i < EDG_APPLY_TILE / EDG_T; ++i) {
        const int64_t k = j * EDG_APPLY_TILE + i * EDG_T + tid;
        if (k >= F) continue;
        const int64_t f = at + k;
        if (par.loop >= 0) {
            float ga, gb;
            edg_loop_gains(par.curve, k, F, &ga, &gb);
            const int64_t s = r.end + k;                            // end is the span's end less X'
            if (CH == 2) {
                typedef float v2f __attribute__((ext_vector_type(2)));
                v2f* q = reinterpret_cast<v2f*>(xs) + f;
                const v2f b = reinterpret_cast<const v2f*>(xs)[s];
                v2f v = *q;
                v.x = edg_mix(v.x, ga, b.x, gb);
                v.y = edg_mix(v.y, ga, b.y, gb);
                *q = v;
            } else {
                xs[f] = edg_mix(xs[f], ga, xs[s], gb);
            }
        } else {
            const float g = edg_gain(par.curve, fade_out ? 2 * (F - k) - 1 : 2 * k + 1, F);
            if (CH == 2) {
                typedef float v2f __attribute__((ext_vector_type(2)));
                v2f* q = reinterpret_cast<v2f*>(xs) + f;
                v2f v = *q;
                v.x = edg_fade(v.x, g);
                v.y = edg_fade(v.y, g);
                *q = v;
            } else {
                xs[f] = edg_fade(xs[f], g);
            }
        }
    }
}
