// sig_tiles.h — what the passes over a ragged batch of signals share on the device
// (kernels_digest.h, kernels_resample.h, kernels_loudness.h, kernels_truepeak.h,
// kernels_pcm.h): the tile lookup, the 16-byte piece loader and its register pin, the
// 64-bit lane exchange and the in-place scale sweep.  DESIGN.md "Signal passes".
//
// meta of a pass: int64 rows of offsets and frames, then n_sig + 1 first tiles (the
// digest keeps int32 tile bases); one workgroup per tile.
#pragma once
#include <hip/hip_runtime.h>
#include "msg_common.h"

// The signal holding a tile: the last p with tile_base[p] <= tile.  Signals without a
// tile share their successor's first tile and are never that one.  Wave-uniform.
// (k_digest_tiles and k_loud_gain write this search out: through the function the compiler
// orders one add's operands the other way, and the kernels are pinned as they are.)
template <class TB>
MSG_DEV int sig_owner(const TB* __restrict__ tile_base, int n_sig, TB tile) {
    int lo = 0, hi = n_sig;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_base[mid] <= tile) lo = mid; else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// Keeps four floats together as they were read: a 16-byte LDS read stays one
// ds_read_b128 whose window slides through registers (without it the compiler re-reads
// the window's odd pairs, 8-byte reads at a lane stride of 16 bytes, 4-way conflicts,
// to feed packed FMAs), and a 16-byte global load is not cut into the parts each later
// use needs.  A pin waits for its load: pin once every load wanted in flight is issued.
MSG_DEV void sig_pin(float4& w) { asm volatile("" : "+v"(w.x), "+v"(w.y), "+v"(w.z), "+v"(w.w)); }

// One 16-byte piece of a tile's span.  Local float e of the span is float gbase + e of x;
// pieces are cut at 16-byte addresses.  Floats outside [lo, hi) read as zero and are never
// loaded; a piece wholly inside is one wide load, an edge piece (odd mono offsets, odd
// frame offsets, the signal's ends) loads float by float.  B: the bounds' type, int where
// the span starts inside the signal.  PIN: the wide load is pinned here, for a caller that
// keeps one piece in flight (the true-peak sweep); otherwise the caller pins, or does not.
template <bool PIN = false, class B>
MSG_DEV float4 sig_piece(const float* __restrict__ x, int64_t gbase, int e0, B lo, B hi) {
    float4 v;
    if (e0 >= lo && e0 + 4 <= hi) {
        v = *reinterpret_cast<const float4*>(x + gbase + e0);
        if (PIN) sig_pin(v);
        return v;
    }
    v.x = (e0 + 0 >= lo && e0 + 0 < hi) ? x[gbase + e0 + 0] : 0.0f;
    v.y = (e0 + 1 >= lo && e0 + 1 < hi) ? x[gbase + e0 + 1] : 0.0f;
    v.z = (e0 + 2 >= lo && e0 + 2 < hi) ? x[gbase + e0 + 2] : 0.0f;
    v.w = (e0 + 3 >= lo && e0 + 3 < hi) ? x[gbase + e0 + 3] : 0.0f;
    return v;
}

MSG_DEV uint64_t sig_shfl64(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

// x *= gf over tile `tile` of signal p in place: tiles of T * PER frames, T threads, each
// thread PER frames T apart.  meta: offsets, frames, then the n_sig + 1 first tiles.
template <int CH, int T, int PER>
MSG_DEV void sig_scale(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, int p, int64_t tile, float gf) {
    const int64_t n = meta[n_sig + p], f0 = (tile - meta[2 * (int64_t)n_sig + p]) * (T * PER);
    float* xs = x + meta[p] * CH;                        // 64-bit from the buffer's base
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int64_t f = f0 + k * T + threadIdx.x;
        if (f < n) {
            if (CH == 2) {
                typedef float v2f __attribute__((ext_vector_type(2)));
                v2f* q = reinterpret_cast<v2f*>(xs) + f;
                v2f w = *q;
                w.x *= gf; w.y *= gf;
                *q = w;
            } else {
                xs[f] *= gf;
            }
        }
    }
}
