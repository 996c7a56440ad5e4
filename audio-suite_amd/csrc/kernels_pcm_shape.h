// kernels_pcm_shape.h — the device side of msg_quantize_shaped (TU k_pcm_shape.hip).  The
// definition, the step function and the host loop are in pcm_shape.h; DESIGN.md §4h
// explains the kernel's shape.
//
//   k_pcm_shape<BITS, DITHER, SHAPE, CH>   one lane per signal, one wave per workgroup.  The
//                         error feedback makes a channel one chain from its first word to
//                         its last, so the only parallelism is across signals: a lane walks
//                         its signal's words in order and keeps CH histories, the two
//                         chains of a stereo signal interleaved word by word.  It loads
//                         PCM_SHAPE_CHUNK words ahead of their use as 16-byte pieces,
//                         quantises four words at a time and stores them as one dwordx2
//                         (16 bits) or dwordx3 (24 bits); a signal's last words go out
//                         byte-exact (pcm_store4).  Signals of unequal length share a wave:
//                         a lane whose signal has ended idles.  The lane has seen the whole
//                         signal, so it writes the record itself: no partials, no atomics.
//
// meta (int64 rows) as for k_pcm: offsets, frames, n_sig + 1 unused tile bases, stream keys k,
// output byte offsets.
#pragma once
#include <hip/hip_runtime.h>
#include "pcm_shape.h"
#include "pcm_store.h"

// sixteen bytes at a 4-byte address (mono signals start at any float): one dwordx4
struct alignas(4) PcmShapePiece { float a, b, c, d; };

// four words from w on, those past the signal's end read as zero and never loaded
MSG_DEV float4 pcm_shape_piece(const float* __restrict__ xs, int64_t w, int64_t words) {
    if (w + 4 <= words) {
        const PcmShapePiece t = *reinterpret_cast<const PcmShapePiece*>(xs + w);
        return make_float4(t.a, t.b, t.c, t.d);
    }
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (w + 0 < words) v.x = xs[w + 0];
    if (w + 1 < words) v.y = xs[w + 1];
    if (w + 2 < words) v.z = xs[w + 2];
    return v;
}

// Four consecutive words of one signal from a word index that is a multiple of four, the
// first m of them inside the signal: word j belongs to channel j % CH (arg: k + (w + 1) G of the first).
template <int BITS, int DITHER, int SHAPE, int CH, bool FULL>
MSG_DEV void pcm_shape_quant4(float4 v, int m, double S, uint64_t arg, PcmShapeState<SHAPE> (&st)[CH], PcmAcc& acc,
                              uint32_t pk[3]) {
    const float xv[4] = {v.x, v.y, v.z, v.w};
    int32_t q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = 0;
        if (FULL || j < m) {
            const int32_t D = DITHER ? pcm_dither_int(arg + (uint64_t)j * PCM_G) : 0;
            q[j] = pcm_shape_word<SHAPE>(xv[j], S, D, st[j % CH], acc);
        }
    }
    pcm_pack4<BITS>(q, pk);
}

template <int BITS, int DITHER, int SHAPE, int CH>
__global__ void __launch_bounds__(PCM_SHAPE_T)
k_pcm_shape(const float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, unsigned char* __restrict__ out,
            PcmRec* __restrict__ rec) {
    constexpr int BY = BITS / 8, NP = PCM_SHAPE_CHUNK / 4;
    const int p = blockIdx.x * PCM_SHAPE_T + threadIdx.x;
    const bool live = p < n_sig;
    const int ps = live ? p : 0;
    const int64_t words = live ? meta[n_sig + ps] * CH : 0;  // a lane past the batch has no words
    const float* xs = x + meta[ps] * CH;                      // 64-bit from the buffer's base
    const uint64_t k = (uint64_t)meta[3 * (int64_t)n_sig + 1 + ps];
    unsigned char* o = out + meta[4 * (int64_t)n_sig + 1 + ps];   // 16-byte aligned
    const double S = (double)(1 << (BITS - 1));
    PcmShapeState<SHAPE> st[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) pcm_shape_reset(st[c]);
    PcmAcc acc = pcm_acc_zero();
    int64_t clipped = 0, nan = 0;
    uint64_t arg = pcm_arg(k, 0);                             // of the chunk's first word
    float4 cur[NP], nxt[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) cur[i] = nxt[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (PCM_SHAPE_CHUNK <= words) {
#pragma unroll
        for (int i = 0; i < NP; ++i) cur[i] = pcm_shape_piece(xs, 4 * i, words);
    }
    for (int64_t c0 = 0; __any(c0 < words); c0 += PCM_SHAPE_CHUNK) {
        // the next whole chunk, in flight while this one is quantised (a last partial chunk loads its own)
        if (c0 + 2 * PCM_SHAPE_CHUNK <= words) {
#pragma unroll
            for (int i = 0; i < NP; ++i) nxt[i] = pcm_shape_piece(xs, c0 + PCM_SHAPE_CHUNK + 4 * i, words);
        }
        if (c0 + PCM_SHAPE_CHUNK <= words) {
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                uint32_t pk[3];
                pcm_shape_quant4<BITS, DITHER, SHAPE, CH, true>(cur[i], 4, S, arg + (uint64_t)(4 * i) * PCM_G, st, acc, pk);
                pcm_store4<BITS>(pk, 4, o + (c0 + 4 * i) * BY);
            }
        } else if (c0 < words) {
            // the signal's last, partial chunk: piece by piece, words past the end neither loaded nor stored
            uint64_t a = arg;
#pragma unroll 1
            for (int64_t w = c0; w < words; w += 4) {
                const float4 v = pcm_shape_piece(xs, w, words);
                const int m = words - w < 4 ? (int)(words - w) : 4;
                uint32_t pk[3];
                pcm_shape_quant4<BITS, DITHER, SHAPE, CH, false>(v, m, S, a, st, acc, pk);
                pcm_store4<BITS>(pk, m, o + w * BY);
                a += 4ull * PCM_G;
            }
        }
        arg += (uint64_t)PCM_SHAPE_CHUNK * PCM_G;
        clipped += acc.clipped;                               // a chunk's counts fit 32 bits, a signal's need 64
        nan += acc.nan;
        acc.clipped = acc.nan = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i) cur[i] = nxt[i];
    }
    if (live) {
        PcmRec r;
        pcm_finish(clipped, nan, acc.q_min, acc.q_max, words > 0, BITS, DITHER, &r);
        rec[p] = r;
    }
}
