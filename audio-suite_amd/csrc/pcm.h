// pcm.h — fixed-point PCM export with TPDF dither (msg_quantize / msg_quantize_host):
// the definition, shared by the device kernels (kernels_pcm.h), the host planning in
// msgpu.hip and the host loop below (built into libmsgpu and into the host sanitizer
// build).  Plain C++.
//
// A signal of n frames of `channels` interleaved float32 words has W = n channels words;
// word w = frame channels + c (64-bit).  bits is 16 or 24, S = 2^(bits - 1).
//
// Dither stream: a function of (seed, key, w) alone, never of the batch, the tile, the
// lane or the device.  G = 0x9E3779B97F4A7C15, fmix64 = dg_fmix64 (digest.h), mod 2^64:
//   k    = fmix64(seed ^ fmix64(key + G))          once per signal, on the host in both paths
//   h(w) = fmix64(k + (w + 1) G)
//   a = h & 0xFFFFFF,  b = (h >> 32) & 0xFFFFFF,  d = (a - b) 2^-24
// d has a triangular density on (-1, 1) LSB with variance 1/6; a - b fits 25 signed
// bits, so d is exact in float32 and float64.
//
// Quantiser: v = (double)x S (exact, S is a power of two); with PCM_DITHER_TPDF
// v = v + d, one float64 add (contracted into a fused step it gives the same bits: the
// product is exact); r = rint(v), ties to even; q = clamp(r, -S, S - 1).  A word whose r
// lies outside that range counts in `clipped` (+-inf included); a NaN word writes 0 and
// counts in `nan`, not in `clipped`.
//
// Packing: little-endian two's complement, 2 or 3 bytes per word, no padding, in word
// order; a signal writes exactly W bits / 8 bytes.
//
// Record: clipped, nan, the minimum and maximum written value (0, 0 for an empty
// signal), bits, dither: integer sums, minima and maxima, so free of order.
//
// The device cuts a signal's words into tiles of PCM_TILE; DESIGN.md §4e has the lane mapping.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstring>
#include "msg_common.h"
#include "digest.h"

constexpr int PCM_T = 256;                 // threads per tile workgroup (4 waves)
constexpr int PCM_TILE = 4096;             // words per tile: 8192 or 12 288 output bytes, multiples of 16
constexpr int PCM_WAVE = PCM_TILE / (PCM_T / 64);   // consecutive words of the tile one wave owns
constexpr int PCM_TURNS = PCM_WAVE / (4 * 64);      // turns of four words per lane
constexpr int PCM_FT = 64;                 // threads of the per-signal fold (one wave)
constexpr int PCM_DITHER_NONE = 0, PCM_DITHER_TPDF = 1;   // MSG_DITHER_* of msgpu.h
constexpr uint64_t PCM_G = 0x9E3779B97F4A7C15ull;

struct PcmRec {                            // layout of msg_pcm_rec
    int64_t clipped, nan;
    int32_t q_min, q_max;
    int32_t bits, dither;
};

// what a lane, a tile or the host loop has seen so far
struct PcmAcc {
    int32_t clipped, nan, q_min, q_max;    // a tile holds at most PCM_TILE words; the host loop widens
};
MSG_HD PcmAcc pcm_acc_zero() { return PcmAcc{0, 0, INT32_MAX, INT32_MIN}; }

MSG_HD bool pcm_bits_ok(int bits) { return bits == 16 || bits == 24; }
MSG_HD bool pcm_dither_ok(int dither) { return dither == PCM_DITHER_NONE || dither == PCM_DITHER_TPDF; }
inline int64_t pcm_tiles(int64_t words) { return (words + PCM_TILE - 1) / PCM_TILE; }
inline int64_t pcm_bytes(int64_t words, int bits) { return words * (bits / 8); }

MSG_HD uint64_t pcm_stream_key(uint64_t seed, uint64_t key) { return dg_fmix64(seed ^ dg_fmix64(key + PCM_G)); }
// the argument of h at word w; consecutive words differ by G
MSG_HD uint64_t pcm_arg(uint64_t k, uint64_t w) { return k + (w + 1) * PCM_G; }
// d from k + (w + 1) G
MSG_HD double pcm_dither_at(uint64_t arg) {
    const uint64_t h = dg_fmix64(arg);
    const int32_t a = (int32_t)(h & 0xFFFFFFu), b = (int32_t)((h >> 32) & 0xFFFFFFu);
    return (double)(a - b) * 0x1p-24;
}

// one word: d is 0 without dither (v + 0 rounds as v does)
template <bool DITHER>
MSG_HD int32_t pcm_word(float x, double S, uint64_t arg, PcmAcc& acc) {
    double v = (double)x * S;
    if (DITHER) v = v + pcm_dither_at(arg);
    // selects, not branches: the lanes of a wave stay together
    const bool isnan = !(v == v);
    double r = __builtin_rint(v);
    const bool under = r < -S, over = r > S - 1.0;           // both false for a NaN
    r = under ? -S : (over ? S - 1.0 : r);
    r = isnan ? 0.0 : r;
    const int32_t q = (int32_t)r;
    acc.clipped += (under || over) ? 1 : 0;
    acc.nan += isnan ? 1 : 0;
    acc.q_min = acc.q_min < q ? acc.q_min : q;
    acc.q_max = acc.q_max > q ? acc.q_max : q;
    return q;
}

// four words packed as they lie in the file: 2 dwords at 16 bits, 3 at 24
template <int BITS>
MSG_HD void pcm_pack4(const int32_t q[4], uint32_t p[3]) {
    if (BITS == 16) {
        p[0] = ((uint32_t)q[0] & 0xFFFFu) | ((uint32_t)q[1] << 16);
        p[1] = ((uint32_t)q[2] & 0xFFFFu) | ((uint32_t)q[3] << 16);
        p[2] = 0;
    } else {
        const uint32_t a = (uint32_t)q[0] & 0xFFFFFFu, b = (uint32_t)q[1] & 0xFFFFFFu;
        const uint32_t c = (uint32_t)q[2] & 0xFFFFFFu, d = (uint32_t)q[3] & 0xFFFFFFu;
        p[0] = a | (b << 24);
        p[1] = (b >> 8) | (c << 16);
        p[2] = (c >> 16) | (d << 8);
    }
}

MSG_HD void pcm_finish(int64_t clipped, int64_t nan, int32_t q_min, int32_t q_max, bool any, int bits, int dither,
                       PcmRec* rec) {
    rec->clipped = clipped;
    rec->nan = nan;
    rec->q_min = any ? q_min : 0;
    rec->q_max = any ? q_max : 0;
    rec->bits = bits;
    rec->dither = dither;
}

// ---- the host loop: the definition word by word ----------------------------------------------
// x: n frames of `channels` interleaved words; out: exactly n channels bits / 8 bytes
template <int BITS, bool DITHER>
inline void pcm_host_loop(const float* x, int64_t words, uint64_t k, unsigned char* out, PcmRec* rec) {
    const double S = (double)(1 << (BITS - 1));
    int64_t clipped = 0, nan = 0;
    PcmAcc acc = pcm_acc_zero();
    for (int64_t w = 0; w < words; ++w) {
        const int32_t q = pcm_word<DITHER>(x[w], S, pcm_arg(k, (uint64_t)w), acc);
        clipped += acc.clipped; nan += acc.nan;
        acc.clipped = acc.nan = 0;
        unsigned char* o = out + w * (BITS / 8);
        o[0] = (unsigned char)((uint32_t)q & 0xFF);
        o[1] = (unsigned char)(((uint32_t)q >> 8) & 0xFF);
        if (BITS == 24) o[2] = (unsigned char)(((uint32_t)q >> 16) & 0xFF);
    }
    pcm_finish(clipped, nan, acc.q_min, acc.q_max, words > 0, BITS, DITHER ? PCM_DITHER_TPDF : PCM_DITHER_NONE, rec);
}

inline void pcm_host(const float* x, int channels, int64_t n, int bits, int dither, uint64_t seed, uint64_t key,
                     void* out, PcmRec* rec) {
    const uint64_t k = pcm_stream_key(seed, key);
    const int64_t words = n * channels;
    unsigned char* o = static_cast<unsigned char*>(out);
    if (bits == 16) {
        if (dither == PCM_DITHER_TPDF) pcm_host_loop<16, true>(x, words, k, o, rec);
        else pcm_host_loop<16, false>(x, words, k, o, rec);
    } else {
        if (dither == PCM_DITHER_TPDF) pcm_host_loop<24, true>(x, words, k, o, rec);
        else pcm_host_loop<24, false>(x, words, k, o, rec);
    }
}
