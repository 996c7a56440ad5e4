// image.h — the stereo image of a signal (msg_stereo_meter / msg_stereo and their host
// references): the definition, shared by the device kernels (kernels_image.h), the entry
// points in signal_abi.inc and the host loops below (built into libmsgpu and into the host
// sanitizer build).  Plain C++.  DESIGN.md "4k. Stereo".
//
// The meter.  A signal is n interleaved L/R float32 frames.  Every product and every sum is
// float64 on the float32 samples, so the products are exact:
//   SLL = sum L^2,  SRR = sum R^2,  SLR = sum L R   over all frames.
// Blocks are loudness.h's: hop = sr / 10 (sr % 10 == 0, sr >= 4000); block j is the frames
// [j hop, j hop + 4 hop); only complete blocks count (0 for n < 4 hop, else (n - 4 hop) / hop + 1).
//   rho_j = SLR_j / sqrt(SLL_j SRR_j)
// A block is kept when SLL_j > 0, SRR_j > 0 and SLL_j + SRR_j > 8 hop 1e-7: a mean square
// per channel above -70 dBFS.  The record is 8 float64:
//   sll, srr, slr   the whole-signal sums
//   corr            slr / sqrt(sll srr); 0 when either sum is 0
//   corr_min        the smallest kept rho_j; corr when no block is kept
//   corr_min_block  its index, the lowest on a tie; -1 when no block is kept
//   blocks_kept, blocks
// The order of the sums (no float atomics anywhere).  The device cuts every hop into tiles of
// IMG_TILE frames with a shorter last one, and the tail after the last full hop likewise, so a
// tile never straddles a hop.  A hop sum is its tiles in order; a block is ((h0 + h1) + h2) + h3;
// a whole-signal sum is the hops in order, then the tail's tiles in order.  Inside a tile frame
// pair q (frames 2 q, 2 q + 1 of the tile) belongs to lane q % IMG_T, which adds its pairs in
// ascending order from +0; a wave folds by the xor butterfly, the waves fold in order.  Every
// step depends on the signal's own frames and length only, never on where the signal lies, so
// a record is the same bits from run to run, alone or in any batch.  The host reference is the
// sequential loop: it differs by float64 roundings of the sums.
//
// The image.  One float32 2 x 2 matrix m = (m00 m01 m10 m11) per call, in place,
//   L' = fma(m00, L, m01 R),  R' = fma(m10, L, m11 R)
// or one fold row f = (f0 f1) into a mono buffer, y = fma(f0, L, f1 R), the input unchanged.
// The product m01 R is rounded to float32, then comes one fused multiply-add: img_mix spells
// both roundings out, so host and device give the same bits whatever contraction a compiler
// is set to.  With a meter record a signal whose corr < 0 has m01, m11 and f1 negated: the
// right channel inverted before everything else, exactly.
#pragma once
#include <stdint.h>
#include <cmath>
#include <vector>
#include "msg_common.h"

constexpr int IMG_T = 256;                  // threads per tile workgroup (4 waves)
constexpr int IMG_PER = 8;                  // 16-byte pieces (frame pairs) per lane
constexpr int IMG_TILE = IMG_T * IMG_PER * 2;   // 4096 frames
constexpr int IMG_GT = 64;                  // threads of the record workgroup (one wave)
constexpr int64_t IMG_SR_MIN = 4000;

struct ImageRec {                           // layout of msg_stereo_rec
    double sll, srr, slr, corr, corr_min, corr_min_block, blocks_kept, blocks;
};

inline bool img_rate_ok(int64_t sr) { return sr >= IMG_SR_MIN && sr % 10 == 0; }

// ---- tiles of a signal: loudness.h's cut ---------------------------------------------
inline int64_t img_tiles_per_hop(int64_t hop) { return (hop + IMG_TILE - 1) / IMG_TILE; }
inline int64_t img_tiles(int64_t n, int64_t hop) {
    const int64_t full = n / hop, tail = n - full * hop;
    return full * img_tiles_per_hop(hop) + (tail + IMG_TILE - 1) / IMG_TILE;
}
inline int64_t img_apply_tiles(int64_t n) { return (n + IMG_TILE - 1) / IMG_TILE; }
MSG_HD int64_t img_blocks(int64_t n, int64_t hop) { return n < 4 * hop ? 0 : (n - 4 * hop) / hop + 1; }

// ---- what host and device share --------------------------------------------------------
MSG_HD double img_gate(int64_t hop) { return 8.0 * (double)hop * 1e-7; }
MSG_HD bool img_kept(double sll, double srr, int64_t hop) { return sll > 0.0 && srr > 0.0 && sll + srr > img_gate(hop); }
MSG_HD double img_corr(double sll, double srr, double slr) {
    return sll > 0.0 && srr > 0.0 ? slr / sqrt(sll * srr) : 0.0;
}

// a l + round32(b r), one rounding each
MSG_HD float img_mix(float a, float l, float b, float r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, l, __fmul_rn(b, r));
#else
    volatile float t = b * r;               // the float32 product, kept from any contraction
    return std::fmaf(a, l, t);
#endif
}

inline bool img_identity(const float* m) { return m[0] == 1.0f && m[1] == 0.0f && m[2] == 0.0f && m[3] == 1.0f; }

// ---- the host references ---------------------------------------------------------------
// the meter as one sequential float64 loop over n interleaved stereo frames
inline void img_meter_host(const float* x, int64_t n, int64_t sr, ImageRec* rec) {
    const int64_t hop = sr / 10, hops = n / hop, nb = img_blocks(n, hop);
    std::vector<double> hs((size_t)hops * 3, 0.0);
    double tail[3] = {0.0, 0.0, 0.0};
    for (int64_t f = 0; f < n; ++f) {
        const double l = (double)x[2 * f], r = (double)x[2 * f + 1];
        double* s = f < hops * hop ? hs.data() + (size_t)(f / hop) * 3 : tail;
        s[0] += l * l;
        s[1] += r * r;
        s[2] += l * r;
    }
    double w[3] = {0.0, 0.0, 0.0};
    for (int64_t h = 0; h < hops; ++h)
        for (int q = 0; q < 3; ++q) w[q] += hs[(size_t)h * 3 + q];
    if (n > hops * hop)
        for (int q = 0; q < 3; ++q) w[q] += tail[q];
    double best = 0.0;
    int64_t at = -1, kept = 0;
    for (int64_t j = 0; j < nb; ++j) {
        double b[3];
        for (int q = 0; q < 3; ++q) {
            const double* h = hs.data() + (size_t)j * 3 + q;
            b[q] = ((h[0] + h[3]) + h[6]) + h[9];
        }
        if (!img_kept(b[0], b[1], hop)) continue;
        ++kept;
        const double rho = b[2] / sqrt(b[0] * b[1]);
        if (at < 0 || rho < best) { best = rho; at = j; }
    }
    rec->sll = w[0];
    rec->srr = w[1];
    rec->slr = w[2];
    rec->corr = img_corr(w[0], w[1], w[2]);
    rec->corr_min = at < 0 ? rec->corr : best;
    rec->corr_min_block = (double)at;
    rec->blocks_kept = (double)kept;
    rec->blocks = (double)nb;
}

// the image over n stereo frames: in place (fold null) or folded into y; flip: the right channel inverted first
inline void img_host(float* x, int64_t n, const float* m, const float* fold, float* y, bool flip) {
    const float sg = flip ? -1.0f : 1.0f;
    if (fold) {
        const float f0 = fold[0], f1 = sg * fold[1];
        for (int64_t f = 0; f < n; ++f) y[f] = img_mix(f0, x[2 * f], f1, x[2 * f + 1]);
        return;
    }
    const float m00 = m[0], m01 = sg * m[1], m10 = m[2], m11 = sg * m[3];
    for (int64_t f = 0; f < n; ++f) {
        const float l = x[2 * f], r = x[2 * f + 1];
        x[2 * f] = img_mix(m00, l, m01, r);
        x[2 * f + 1] = img_mix(m10, l, m11, r);
    }
}
