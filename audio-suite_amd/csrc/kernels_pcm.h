// kernels_pcm.h — the device side of msg_quantize (TU k_pcm.hip).  The definition, the
// tile shape and the host loop are in pcm.h; DESIGN.md §4e explains the lane mapping.
//
//   k_pcm<BITS, DITHER>   one workgroup per tile of PCM_TILE words of one signal.  A wave
//                         owns PCM_WAVE consecutive words; in each of its PCM_TURNS turns a
//                         lane quantises four consecutive words and stores them as one
//                         dwordx2 (16 bits) or dwordx3 (24 bits), so every store
//                         instruction of a wave writes one contiguous run of 512 or 768
//                         bytes.  Three paths, chosen per tile: a whole tile at a 16-byte
//                         address, a whole tile off one (two pieces per four words), the
//                         signal's last tile.  The tile's counts, minimum and maximum go
//                         to part[tile].
//   k_pcm_fin             one wave per signal: the fold of its tiles, the record
//
// meta (int64 rows): offsets, frames, n_sig + 1 first tiles, stream keys k, output byte offsets.
#pragma once
#include <hip/hip_runtime.h>
#include "pcm.h"
#include "pcm_store.h"                     // pcm_store4: a lane's four packed words, the signal's end byte-exact
#include "sig_tiles.h"

// Four consecutive words of one lane, the first m of them inside the signal, quantised
// and packed as they lie in the file (arg: k + (w + 1) G of the first).
template <int BITS, int DITHER>
MSG_DEV void pcm_quant4(float4 v, int m, double S, uint64_t arg, PcmAcc& acc, uint32_t pk[3]) {
    const float xv[4] = {v.x, v.y, v.z, v.w};
    int32_t q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = 0;
        if (j < m) q[j] = pcm_word<DITHER != 0>(xv[j], S, arg + (uint64_t)j * PCM_G, acc);
    }
    pcm_pack4<BITS>(q, pk);
}

// A lane's four words from the two pieces they lie in: v at e0 - a, u at e0 - a + 4, a = 1 .. 3
MSG_DEV float4 pcm_shifted(float4 v, float4 u, int a) {
    if (a == 1) return make_float4(v.y, v.z, v.w, u.x);
    if (a == 2) return make_float4(v.z, v.w, u.x, u.y);
    return make_float4(v.w, u.x, u.y, u.z);
}

MSG_DEV void pcm_acc_add(PcmAcc& a, const PcmAcc& b) {
    a.clipped += b.clipped;
    a.nan += b.nan;
    a.q_min = a.q_min < b.q_min ? a.q_min : b.q_min;
    a.q_max = a.q_max > b.q_max ? a.q_max : b.q_max;
}

template <int BITS, int DITHER>
__global__ void __launch_bounds__(PCM_T)
k_pcm(const float* __restrict__ x, int channels, const int64_t* __restrict__ meta, int n_sig,
      unsigned char* __restrict__ out, int4* __restrict__ part) {
    constexpr int BY = BITS / 8;
    __shared__ int4 red[PCM_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int p = sig_owner(tile_base, n_sig, tile);
    const int64_t words = meta[n_sig + p] * channels;
    const int64_t w0 = (tile - tile_base[p]) * PCM_TILE;      // the tile's first word, 0 <= w0 < words
    const int64_t left = words - w0;
    const int E = (int)(left < PCM_TILE ? left : PCM_TILE);   // words of this tile
    const int64_t gbase = meta[p] * channels + w0;            // 64-bit from the buffer's base
    const int a = (int)(((int64_t)(reinterpret_cast<uintptr_t>(x) >> 2) + gbase) & 3);   // uniform over the tile
    const uint64_t k = (uint64_t)meta[3 * (int64_t)n_sig + 1 + p];
    unsigned char* o = out + meta[4 * (int64_t)n_sig + 1 + p] + w0 * BY;   // 16-byte aligned
    const double S = (double)(1 << (BITS - 1));
    // k + (w + 1) G of this lane's first word: one 64-bit multiply from the tile's base, adds from there
    const int e_first = wave * PCM_WAVE + 4 * lane;
    uint64_t arg = pcm_arg(k, (uint64_t)w0) + (uint64_t)e_first * PCM_G;
    PcmAcc acc = pcm_acc_zero();
    if (a == 0 && E == PCM_TILE) {
        // a whole tile at a 16-byte address: every load issued before the first word is formed
        float4 v[PCM_TURNS];
#pragma unroll
        for (int t = 0; t < PCM_TURNS; ++t)
            v[t] = *reinterpret_cast<const float4*>(x + gbase + e_first + t * 256);
#pragma unroll
        for (int t = 0; t < PCM_TURNS; ++t) sig_pin(v[t]);    // pinned once all are in flight: a pin waits for its load
#pragma unroll
        for (int t = 0; t < PCM_TURNS; ++t) {
            uint32_t pk[3];
            pcm_quant4<BITS, DITHER>(v[t], 4, S, arg + (uint64_t)(t * 256) * PCM_G, acc, pk);
            pcm_store4<BITS>(pk, 4, o + (e_first + t * 256) * BY);
        }
    } else if (E == PCM_TILE) {
        // a whole tile that starts off a 16-byte address (mono at an odd float, stereo at an odd
        // frame): the lane's words e0 .. e0 + 3 lie in the pieces at e0 - a and e0 - a + 4; only
        // the tile's first and last piece reach outside it: those two lanes load a neighbouring
        // piece with the others, so that again every wide load goes out first with no branch
        // between them, and fetch their own piece float by float afterwards.
        float4 v[PCM_TURNS], u[PCM_TURNS];
#pragma unroll
        for (int t = 0; t < PCM_TURNS; ++t) {
            const int ev = e_first + t * 256 - a;
            v[t] = *reinterpret_cast<const float4*>(x + gbase + (ev < 0 ? ev + 4 : ev));
            u[t] = *reinterpret_cast<const float4*>(x + gbase + (ev + 8 > PCM_TILE ? ev : ev + 4));
        }
#pragma unroll
        for (int t = 0; t < PCM_TURNS; ++t) { sig_pin(v[t]); sig_pin(u[t]); }
        if (e_first == 0) v[0] = sig_piece(x, gbase, -a, 0, E);
        if (e_first + (PCM_TURNS - 1) * 256 + 4 == PCM_TILE) u[PCM_TURNS - 1] = sig_piece(x, gbase, PCM_TILE - a, 0, E);
#pragma unroll
        for (int t = 0; t < PCM_TURNS; ++t) {
            uint32_t pk[3];
            pcm_quant4<BITS, DITHER>(pcm_shifted(v[t], u[t], a), 4, S, arg + (uint64_t)(t * 256) * PCM_G, acc, pk);
            pcm_store4<BITS>(pk, 4, o + (e_first + t * 256) * BY);
        }
    } else {
        // the signal's last tile: turn by turn, words past the end neither loaded nor stored
#pragma unroll 1
        for (int t = 0; t < PCM_TURNS; ++t) {
            const int e0 = e_first + t * 256;
            if (e0 < E) {
                float4 v = sig_piece(x, gbase, e0 - a, 0, E);
                sig_pin(v);
                if (a != 0) {
                    float4 u = sig_piece(x, gbase, e0 - a + 4, 0, E);
                    sig_pin(u);
                    v = pcm_shifted(v, u, a);
                }
                const int m = E - e0 < 4 ? E - e0 : 4;        // words of the signal among the four
                uint32_t pk[3];
                pcm_quant4<BITS, DITHER>(v, m, S, arg, acc, pk);
                pcm_store4<BITS>(pk, m, o + e0 * BY);
            }
            arg += 256ull * PCM_G;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        PcmAcc b;
        b.clipped = __shfl_xor(acc.clipped, s, 64);
        b.nan = __shfl_xor(acc.nan, s, 64);
        b.q_min = __shfl_xor(acc.q_min, s, 64);
        b.q_max = __shfl_xor(acc.q_max, s, 64);
        pcm_acc_add(acc, b);
    }
    if (lane == 0) red[wave] = make_int4(acc.clipped, acc.nan, acc.q_min, acc.q_max);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < PCM_T / 64; ++w) {
            const int4 r = red[w];
            pcm_acc_add(acc, PcmAcc{r.x, r.y, r.z, r.w});
        }
        part[tile] = make_int4(acc.clipped, acc.nan, acc.q_min, acc.q_max);
    }
}

// one wave per signal: lane i takes tiles i, i + 64, ..; then the xor-butterfly and the record
__global__ void __launch_bounds__(PCM_FT)
k_pcm_fin(const int64_t* __restrict__ meta, int n_sig, const int4* __restrict__ part, int bits, int dither,
          PcmRec* __restrict__ rec) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t t0 = tile_base[p], t1 = tile_base[p + 1];
    int64_t clipped = 0, nan = 0;
    int32_t q_min = INT32_MAX, q_max = INT32_MIN;
    for (int64_t t = t0 + lane; t < t1; t += PCM_FT) {
        const int4 v = part[t];
        clipped += v.x;
        nan += v.y;
        q_min = q_min < v.z ? q_min : v.z;
        q_max = q_max > v.w ? q_max : v.w;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        clipped += __shfl_xor((long long)clipped, s, 64);
        nan += __shfl_xor((long long)nan, s, 64);
        const int32_t lo = __shfl_xor(q_min, s, 64), hi = __shfl_xor(q_max, s, 64);
        q_min = q_min < lo ? q_min : lo;
        q_max = q_max > hi ? q_max : hi;
    }
    if (lane == 0) {
        PcmRec r;
        pcm_finish(clipped, nan, q_min, q_max, t1 > t0, bits, dither, &r);
        rec[p] = r;
    }
}
