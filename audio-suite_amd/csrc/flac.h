// flac.h — FLAC delivery (msg_flac / msg_flac_host): lossless frames with fixed predictors.  The
// definition, shared by the device kernels (kernels_flac.h), the entry points in signal_abi.inc and
// host_abi.inc and the host loop below (built into libmsgpu and into the host sanitizer build).
// Plain C++, integers only.  DESIGN.md "4n. FLAC".
//
// Input: what msg_quantize leaves behind, packed little-endian PCM of `bits` in {16, 24} and
// `channels` in {1, 2}, one signal of n frames.  Output: the signal's FLAC frames back to back; the
// 42-byte stream header is the host's (msgpu/flac.py) from the record.  Every field is MSB-first.
//
// Blocks.  B in {256 .. 4096}; block j covers frames [jB, min((j + 1)B, n)).
// Frame header.  FF F8, block-size code | rate code, assignment | sample size, the frame number in
//   the extended UTF-8 coding, the block-size bytes and rate bytes if any, CRC-8 (flac_header).
// Channels of a stereo block: 0 left, 1 right, 2 mid = (L + R) >> 1, 3 side = L - R at bits + 1.
// Subframe of n samples at depth d: constant (all equal, 8 + d bits), verbatim (8 + n d), or, for
//   n > 4, fixed of the order 0 .. 4 with the smallest sum over i >= 4 of |r_o[i]| (ties low).  Its
//   residual section: u = fold(r); per partition of c residuals with S = sum u the parameter is
//   the cheapest of k0 - 1, k0, k0 + 1 in exact bits c (k + 1) + sum(u >> k), k0 the smallest k
//   with (c << k) >= S capped at 14 (16 bits) or 30 (24 bits), ties to the smaller k; the partition
//   order is the cheapest of p in 0 .. 6 with 2^p | n and (n >> p) > o, ties low.  Fixed is kept
//   when its exact cost is under the verbatim cost.
// Assignment of a stereo block: the cheapest of L+R, L+side, side+R, mid+side, ties in that order.
// Frame end: zero bits to a byte, CRC-16 of the frame so far, high byte first.
//
// The device forms the same decisions from sums over lanes' chunks (the flac_chunk_* helpers
// below, integer adds in any order) and packs a frame by OR-ing each sample's one bit and k low
// bits into a zeroed buffer (flac_put), which is order-free; tests/flac_check.cpp runs those
// helpers on the host in shuffled order against the sequential loop.
#pragma once
#include <cstdint>
#include <cstring>
#include "msg_common.h"
#include <vector>
#if defined(__clang__)
#define FLAC_UNROLL _Pragma("unroll")
#else
#define FLAC_UNROLL
#endif

constexpr int FLAC_T = 256;                     // lanes of a workgroup of the plan and pack sweeps
constexpr int FLAC_MAXB = 4096;
constexpr int64_t FLAC_MAX_FRAMES = ((int64_t)1 << 31) - ((int64_t)1 << 20);      // the library's limit of a signal
constexpr int FLAC_C = FLAC_MAXB / FLAC_T;      // a lane's chunk: at most 16 samples
constexpr int FLAC_XS = FLAC_MAXB + FLAC_MAXB / 16 + 1;     // flac_pos(FLAC_MAXB) + 1
constexpr int FLAC_HDR_MAX = 16;
constexpr int FLAC_FRAME_WORDS = (FLAC_HDR_MAX + 2 * (1 + FLAC_MAXB * 3) + 2 + 3) / 4 + 2;
constexpr int FLAC_TYPE_CONSTANT = 0, FLAC_TYPE_VERBATIM = 1, FLAC_TYPE_FIXED = 2;

struct FlacRec {                                // layout of msg_flac_rec
    int64_t byte_off, bytes, frames, samples;
    int32_t min_frame, max_frame;
    uint8_t md5[16];
    int32_t constant, verbatim, fixed, flags;   // flags bit 0: the MD5 was computed
    int32_t assign[4];                          // stereo frames as L+R, L+side, side+R, mid+side
};
struct FlacBest {                               // the best subframe of one channel of one block
    int64_t cost;                               // exact bits, the 8 header bits included
    uint8_t type, order, porder, pad;
    uint8_t k[64];
};
struct FlacPlan {                               // one block: what the pack sweep needs
    int32_t bytes, assign;                      // the whole frame, CRC-16 included; 0 .. 3, -1 mono
    FlacBest sub[2];
};
// the sums of one channel of one block the lanes add into; level p's partition q is entry (1 << p) - 1 + q
struct FlacWork {
    unsigned long long abs[5];
    unsigned long long S[128];
    unsigned long long E[128][3];
    long long cost[128];
    long long total[8];
    int32_t mn, mx;
    uint8_t k0[128], kb[128];
};

MSG_HD int flac_pos(int i) { return i + (i >> 4); }          // rows of 16 + 1 words: a lane's chunk reads conflict-free
MSG_HD int flac_kmax(int bits) { return bits == 16 ? 14 : 30; }
MSG_HD int flac_pbits(int bits) { return bits == 16 ? 4 : 5; }
MSG_HD bool flac_block_ok(int B) { return B == 256 || B == 512 || B == 1024 || B == 2048 || B == 4096; }
MSG_HD int64_t flac_blocks(int64_t n, int B) { return (n + B - 1) / B; }
MSG_HD int64_t flac_frame_bound(int n, int channels, int bits) { return FLAC_HDR_MAX + (int64_t)channels * (1 + (int64_t)n * bits / 8) + 2; }
MSG_HD int64_t flac_bound(int64_t n, int channels, int bits, int B) {
    const int64_t full = n / B;
    const int last = (int)(n - full * B);
    return full * flac_frame_bound(B, channels, bits) + (last ? flac_frame_bound(last, channels, bits) : 0);
}

// sample word w of packed little-endian PCM, sign-extended
MSG_HD int32_t flac_load(const uint8_t* p, int bits, int64_t w) {
    if (bits == 16) {
        const uint8_t* q = p + 2 * w;
        return (int16_t)(uint16_t)(q[0] | (q[1] << 8));
    }
    const uint8_t* q = p + 3 * w;
    return (int32_t)(((uint32_t)q[0] << 8) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 24)) >> 8;
}
MSG_HD int32_t flac_chan(int32_t l, int32_t r, int c) { return c == 0 ? l : c == 1 ? r : c == 2 ? (l + r) >> 1 : l - r; }
MSG_HD int flac_assign_code(int a) { return a < 0 ? 0 : a == 0 ? 1 : 7 + a; }
MSG_HD int flac_assign_chan(int a, int s) { return a < 0 ? 0 : a == 0 ? s : a == 1 ? (s ? 3 : 0) : a == 2 ? (s ? 1 : 3) : (s ? 3 : 2); }
MSG_HD uint32_t flac_fold(int64_t r) { return (uint32_t)(r >= 0 ? 2 * r : -2 * r - 1); }
MSG_HD int flac_k0(int64_t c, unsigned long long S, int kmax) {
    int k = 0;
    while (k < kmax && ((unsigned long long)c << k) < S) ++k;
    return k;
}
// the largest partition order of a block of n samples at predictor order o
MSG_HD int flac_pmax(int n, int o) {
    int p = 0;
    while (p < 6 && !((n >> p) & 1) && (n >> (p + 1)) > o) ++p;
    return p;
}
MSG_HD int flac_order(const unsigned long long* abs) {
    int o = 0;
    for (int t = 1; t < 5; ++t)
        if (abs[t] < abs[o]) o = t;
    return o;
}

// a block's two channels in rows of 16 + 1 words (flac_pos), and one of its four channels
struct FlacX {
    const int32_t* l;
    const int32_t* r;                           // mono: l again
    int c;
    MSG_HD int32_t operator()(int i) const { return flac_chan(l[flac_pos(i)], r[flac_pos(i)], c); }
};
template <class X>
MSG_HD int64_t flac_resid_at(const X& x, int i, int o) {
    const int64_t a = x(i);
    if (o == 0) return a;
    const int64_t b = x(i - 1);
    if (o == 1) return a - b;
    const int64_t c = x(i - 2);
    if (o == 2) return a - 2 * b + c;
    const int64_t d = x(i - 3);
    if (o == 3) return a - 3 * b + 3 * c - d;
    return a - 4 * b + 6 * c - 4 * d + x(i - 4);
}

// ---- the rate and the frame header ----
MSG_HD bool flac_rate_ok(int64_t sr) { return sr >= 1 && sr <= 655350; }
MSG_HD int flac_rate_code(int64_t sr, int* nbytes, int* val) {
    *nbytes = 0; *val = 0;
    switch (sr) {
        case 88200: return 1; case 176400: return 2; case 192000: return 3; case 8000: return 4;
        case 16000: return 5; case 22050: return 6; case 24000: return 7; case 32000: return 8;
        case 44100: return 9; case 48000: return 10; case 96000: return 11;
        default: break;
    }
    if (sr % 1000 == 0 && sr <= 255000) { *nbytes = 1; *val = (int)(sr / 1000); return 12; }
    if (sr <= 65535) { *nbytes = 2; *val = (int)sr; return 13; }
    if (sr % 10 == 0 && sr <= 655350) { *nbytes = 2; *val = (int)(sr / 10); return 14; }
    return 0;
}
MSG_HD uint32_t flac_crc8(uint32_t crc, uint32_t byte) {
    crc ^= byte;
    for (int i = 0; i < 8; ++i) crc = ((crc << 1) ^ ((crc & 0x80) ? 0x07 : 0)) & 0xFF;
    return crc;
}
MSG_HD uint32_t flac_crc16(uint32_t crc, uint32_t byte) {
    crc ^= byte << 8;
    for (int i = 0; i < 8; ++i) crc = ((crc << 1) ^ ((crc & 0x8000) ? 0x8005 : 0)) & 0xFFFF;
    return crc;
}
// a b mod x^16 + x^15 + x^2 + 1, carry-less
MSG_HD uint32_t flac_mulmod16(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; --i) {
        r = ((r << 1) ^ ((r & 0x8000) ? 0x8005 : 0)) & 0xFFFF;
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
// x^(8 m) mod the same: crc16(A | B) = crc16(A) x^(8 |B|) ^ crc16(B)
MSG_HD uint32_t flac_xpow16(uint32_t m) {
    uint32_t r = 1, b = 0x0100;                 // x^8
    for (; m; m >>= 1) {
        if (m & 1) r = flac_mulmod16(r, b);
        b = flac_mulmod16(b, b);
    }
    return r;
}
// the header of frame j of n samples (block size B) into h; returns its bytes, the CRC-8 included
MSG_HD int flac_header(uint8_t* h, int B, int n, int64_t sr, int assign, int bits, int64_t j) {
    int rb, rv, len = 0;
    const int rc = flac_rate_code(sr, &rb, &rv);
    int bc;
    if (n == B) {
        bc = 8;
        for (int b = B; b > 256; b >>= 1) ++bc;
    } else {
        bc = n <= 256 ? 6 : 7;
    }
    h[len++] = 0xFF;
    h[len++] = 0xF8;
    h[len++] = (uint8_t)((bc << 4) | rc);
    h[len++] = (uint8_t)((flac_assign_code(assign) << 4) | ((bits == 16 ? 4 : 6) << 1));
    if (j < (1 << 7)) {
        h[len++] = (uint8_t)j;
    } else {
        int cont = j < (1 << 11) ? 1 : j < (1 << 16) ? 2 : j < (1 << 21) ? 3 : j < (1 << 26) ? 4 : 5;
        h[len++] = (uint8_t)(((0xFF00 >> (cont + 1)) & 0xFF) | (int)(j >> (6 * cont)));
        for (int c = cont - 1; c >= 0; --c) h[len++] = (uint8_t)(0x80 | ((j >> (6 * c)) & 0x3F));
    }
    if (bc == 6) h[len++] = (uint8_t)(n - 1);
    if (bc == 7) { h[len++] = (uint8_t)((n - 1) >> 8); h[len++] = (uint8_t)(n - 1); }
    if (rb == 1) h[len++] = (uint8_t)rv;
    if (rb == 2) { h[len++] = (uint8_t)(rv >> 8); h[len++] = (uint8_t)rv; }
    uint32_t crc = 0;
    for (int i = 0; i < len; ++i) crc = flac_crc8(crc, h[i]);
    h[len++] = (uint8_t)crc;
    return len;
}

// ---- the frame as 32-bit words, stream bit 32 w at word w's top bit ----
struct FlacOrPlain {
    MSG_HD void operator()(uint32_t* p, uint32_t v) const { *p |= v; }
};
struct FlacAddPlain {
    MSG_HD void add(unsigned long long* p, unsigned long long v) const { *p += v; }
    MSG_HD void lo(int32_t* p, int32_t v) const { if (v < *p) *p = v; }
    MSG_HD void hi(int32_t* p, int32_t v) const { if (v > *p) *p = v; }
};
// nb <= 32 bits of v (v < 2^nb) at stream bit pos
template <class O>
MSG_HD void flac_put(O orr, uint32_t* w, int64_t pos, uint32_t v, int nb) {
    if (nb == 0 || v == 0) return;
    const int64_t wi = pos >> 5;
    const int room = 32 - (int)(pos & 31);
    if (nb <= room) {
        orr(&w[wi], v << (room - nb));
    } else {
        orr(&w[wi], v >> (nb - room));
        orr(&w[wi + 1], v << (32 - (nb - room)));
    }
}
MSG_HD uint32_t flac_byte(const uint32_t* w, int b) { return (w[b >> 2] >> (24 - 8 * (b & 3))) & 0xFF; }
MSG_HD uint32_t flac_mask(int d) { return d >= 32 ? 0xFFFFFFFFu : (1u << d) - 1u; }

// ---- the plan of one channel from chunk sums ----
MSG_HD void flac_work_init(FlacWork* W) {
    for (int t = 0; t < 5; ++t) W->abs[t] = 0;
    W->mn = INT32_MAX;
    W->mx = INT32_MIN;
}
MSG_HD void flac_work_zero(FlacWork* W, int idx) {         // idx 0 .. 127
    W->S[idx] = 0;
    W->E[idx][0] = W->E[idx][1] = W->E[idx][2] = 0;
}
// samples [i0, i1): the range and the five sums over i >= 4
template <class X, class A>
MSG_HD void flac_chunk_abs(const X& x, int i0, int i1, FlacWork* W, A add) {
    if (i0 >= i1) return;
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    unsigned long long s[5] = {0, 0, 0, 0, 0};
    int64_t a1 = i0 >= 1 ? x(i0 - 1) : 0, a2 = i0 >= 2 ? x(i0 - 2) : 0, a3 = i0 >= 3 ? x(i0 - 3) : 0, a4 = i0 >= 4 ? x(i0 - 4) : 0;
FLAC_UNROLL
    for (int j = 0; j < FLAC_C; ++j) {
        const int i = i0 + j;
        if (i < i1) {
            const int32_t v = x(i);
            const int64_t a0 = v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
            if (i >= 4) {
                const int64_t r1 = a0 - a1, r2 = a0 - 2 * a1 + a2, r3 = a0 - 3 * a1 + 3 * a2 - a3,
                              r4 = a0 - 4 * a1 + 6 * a2 - 4 * a3 + a4;
                s[0] += (unsigned long long)(a0 < 0 ? -a0 : a0);
                s[1] += (unsigned long long)(r1 < 0 ? -r1 : r1);
                s[2] += (unsigned long long)(r2 < 0 ? -r2 : r2);
                s[3] += (unsigned long long)(r3 < 0 ? -r3 : r3);
                s[4] += (unsigned long long)(r4 < 0 ? -r4 : r4);
            }
            a4 = a3; a3 = a2; a2 = a1; a1 = a0;
        }
    }
    add.lo(&W->mn, mn);
    add.hi(&W->mx, mx);
    for (int t = 0; t < 5; ++t) add.add(&W->abs[t], s[t]);
}
// samples [i0, i1) at order o: u of each (0 for a warm-up sample) and the sums of the finest partitions
template <class X, class A>
MSG_HD void flac_chunk_S(const X& x, int i0, int i1, int o, int pm, int n, uint32_t (&u)[FLAC_C], FlacWork* W, A add) {
    if (i0 >= i1) return;
    const int plen = n >> pm, base = (1 << pm) - 1;
    int q = i0 / plen, rem = i0 - q * plen;
    unsigned long long acc = 0;
FLAC_UNROLL
    for (int j = 0; j < FLAC_C; ++j) {
        const int i = i0 + j;
        u[j] = 0;
        if (i < i1) {
            if (i >= o) u[j] = flac_fold(flac_resid_at(x, i, o));
            acc += u[j];
            if (++rem == plen || i + 1 == i1) {
                add.add(&W->S[base + q], acc);
                acc = 0;
                if (rem == plen) { rem = 0; ++q; }
            }
        }
    }
}
// entry idx = (1 << p) - 1 + q, p <= pm: its sum from the finest level's, and k0
MSG_HD void flac_entry_k0(FlacWork* W, int n, int o, int pm, int bits, int idx) {
    int p = 0;
    while ((2 << p) - 1 <= idx) ++p;
    if (p > pm) return;
    const int q = idx - ((1 << p) - 1), span = 1 << (pm - p), base = (1 << pm) - 1;
    unsigned long long s = 0;
    if (p < pm) {
        for (int t = 0; t < span; ++t) s += W->S[base + q * span + t];
        W->S[idx] = s;
    } else {
        s = W->S[idx];
    }
    W->k0[idx] = (uint8_t)flac_k0((n >> p) - (q == 0 ? o : 0), s, flac_kmax(bits));
}
// samples [i0, i1): sum(u >> k) for k0 - 1, k0, k0 + 1 of the partition each lies in, at every level
template <class A>
MSG_HD void flac_chunk_E(const uint32_t (&u)[FLAC_C], int i0, int i1, int pm, int n, FlacWork* W, A add) {
    if (i0 >= i1) return;
    const int plen = n >> pm, qf0 = i0 / plen, rem0 = i0 - qf0 * plen;
    for (int p = 0; p <= pm; ++p) {
        const int sh = pm - p, base = (1 << p) - 1;
        int qf = qf0, rem = rem0;
        int k0 = W->k0[base + (qf >> sh)];
        unsigned long long a0 = 0, a1 = 0, a2 = 0;
FLAC_UNROLL
        for (int j = 0; j < FLAC_C; ++j) {
            const int i = i0 + j;
            if (i < i1) {
                const uint32_t v = u[j];
                a0 += k0 > 0 ? v >> (k0 - 1) : 0;
                a1 += v >> k0;
                a2 += v >> (k0 + 1);
                const int cur = qf >> sh;
                if (++rem == plen) { rem = 0; ++qf; }
                if ((qf >> sh) != cur || i + 1 == i1) {
                    add.add(&W->E[base + cur][0], a0);
                    add.add(&W->E[base + cur][1], a1);
                    add.add(&W->E[base + cur][2], a2);
                    a0 = a1 = a2 = 0;
                    if (i + 1 < i1) k0 = W->k0[base + (qf >> sh)];
                }
            }
        }
    }
}
// entry idx: the cheapest of its three parameters and its bits without the parameter's own
MSG_HD void flac_entry_pick(FlacWork* W, int n, int o, int pm, int bits, int idx) {
    int p = 0;
    while ((2 << p) - 1 <= idx) ++p;
    if (p > pm) return;
    const int q = idx - ((1 << p) - 1), kmax = flac_kmax(bits), k0 = W->k0[idx];
    const long long c = (n >> p) - (q == 0 ? o : 0);
    long long best = INT64_MAX;
    int kb = 0;
    for (int t = 0; t < 3; ++t) {
        const int k = k0 - 1 + t;
        if (k < 0 || k > kmax) continue;
        const long long b = c * (k + 1) + (long long)W->E[idx][t];
        if (b < best) { best = b; kb = k; }
    }
    W->kb[idx] = (uint8_t)kb;
    W->cost[idx] = best;
}
// one lane: the channel's best subframe
MSG_HD void flac_finish(const FlacWork* W, int n, int d, int bits, int o, int pm, FlacBest* b) {
    b->pad = 0;
    b->order = b->porder = 0;
    const long long verb = 8 + (long long)n * d;
    if (W->mn == W->mx) { b->type = FLAC_TYPE_CONSTANT; b->cost = 8 + d; return; }
    b->type = FLAC_TYPE_VERBATIM;
    b->cost = verb;
    if (n <= 4) return;
    long long best = INT64_MAX;
    int pb = 0;
    for (int p = 0; p <= pm; ++p) {
        long long t = (long long)flac_pbits(bits) << p;
        for (int q = 0; q < (1 << p); ++q) t += W->cost[(1 << p) - 1 + q];
        if (t < best) { best = t; pb = p; }
    }
    const long long fixed = 8 + (long long)o * d + 6 + best;
    if (fixed >= verb) return;
    b->type = FLAC_TYPE_FIXED;
    b->cost = fixed;
    b->order = (uint8_t)o;
    b->porder = (uint8_t)pb;
    for (int q = 0; q < (1 << pb); ++q) b->k[q] = W->kb[(1 << pb) - 1 + q];
}
// the assignment and the frame's bytes from the channels' best subframes (stereo: best[0 .. 3])
MSG_HD void flac_assign(const FlacBest* best, int channels, int hdr_bytes, FlacPlan* plan) {
    int a = -1;
    long long bits = best[0].cost;
    if (channels == 2) {
        a = 0;
        bits = best[0].cost + best[1].cost;
        for (int t = 1; t < 4; ++t) {
            const long long c = best[flac_assign_chan(t, 0)].cost + best[flac_assign_chan(t, 1)].cost;
            if (c < bits) { bits = c; a = t; }
        }
    }
    plan->assign = a;
    plan->bytes = hdr_bytes + (int32_t)((bits + 7) >> 3) + 2;
    plan->sub[0] = best[flac_assign_chan(a, 0)];
    plan->sub[1] = best[channels == 2 ? flac_assign_chan(a, 1) : 0];
}

// ---- the pack of a fixed subframe from chunks ----
// samples [i0, i1): u of each and the chunk's bits, a partition's parameter counted with its first residual
template <class X>
MSG_HD int32_t flac_chunk_len(const X& x, int i0, int i1, const FlacBest& s, int n, int bits, uint32_t (&u)[FLAC_C]) {
    int32_t len = 0;
    if (i0 >= i1) return 0;
    const int o = s.order, plen = n >> s.porder;
    int q = i0 / plen, rem = i0 - q * plen;
FLAC_UNROLL
    for (int j = 0; j < FLAC_C; ++j) {
        const int i = i0 + j;
        u[j] = 0;
        if (i < i1) {
            if (i >= o) {
                const int k = s.k[q];
                u[j] = flac_fold(flac_resid_at(x, i, o));
                len += (int32_t)(u[j] >> k) + 1 + k;
                if (i == (q == 0 ? o : q * plen)) len += flac_pbits(bits);
            }
            if (++rem == plen) { rem = 0; ++q; }
        }
    }
    return len;
}
// the same samples into the frame: pos is the stream bit of the chunk's first code (or parameter)
template <class O>
MSG_HD void flac_chunk_pack(const uint32_t (&u)[FLAC_C], int i0, int i1, const FlacBest& s, int n, int bits, int64_t pos,
                            uint32_t* w, O orr) {
    if (i0 >= i1) return;
    const int o = s.order, plen = n >> s.porder;
    int q = i0 / plen, rem = i0 - q * plen;
FLAC_UNROLL
    for (int j = 0; j < FLAC_C; ++j) {
        const int i = i0 + j;
        if (i < i1) {
            if (i >= o) {
                const int k = s.k[q];
                if (i == (q == 0 ? o : q * plen)) {
                    flac_put(orr, w, pos, (uint32_t)k, flac_pbits(bits));
                    pos += flac_pbits(bits);
                }
                const uint32_t hi = u[j] >> k;
                flac_put(orr, w, pos + hi, (1u << k) | (u[j] & ((1u << k) - 1u)), k + 1);
                pos += hi + 1 + k;
            }
            if (++rem == plen) { rem = 0; ++q; }
        }
    }
}
// what one lane writes in front of the samples of subframe s at stream bit pos: the subframe header,
// a constant's sample, a fixed subframe's method and partition order; returns the subframe's first sample bit
template <class X, class O>
MSG_HD int64_t flac_sub_head(const X& x, const FlacBest& s, int d, int bits, int64_t pos, uint32_t* w, O orr, bool write) {
    const uint32_t type = s.type == FLAC_TYPE_CONSTANT ? 0 : s.type == FLAC_TYPE_VERBATIM ? 1 : 8 + s.order;
    if (write) flac_put(orr, w, pos, type << 1, 8);
    pos += 8;
    if (s.type == FLAC_TYPE_CONSTANT && write) flac_put(orr, w, pos, (uint32_t)x(0) & flac_mask(d), d);
    if (s.type == FLAC_TYPE_FIXED && write)
        flac_put(orr, w, pos + (int64_t)s.order * d, ((bits == 16 ? 0u : 1u) << 4) | s.porder, 6);
    return pos;
}

// ---- MD5 ----
MSG_HD uint32_t flac_rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
MSG_HD void flac_md5_block(uint32_t* st, const uint32_t* m) {
    constexpr uint32_t K[64] = {
        0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501, 0x698098d8, 0x8b44f7af,
        0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821, 0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa,
        0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8,
        0x676f02d9, 0x8d2a4c8a, 0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
        0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665, 0xf4292244, 0x432aff97,
        0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1, 0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1,
        0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
    constexpr int R[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
FLAC_UNROLL
    for (int i = 0; i < 64; ++i) {
        uint32_t f;
        int g;
        if (i < 16) { f = (b & c) | (~b & d); g = i; }
        else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
        else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
        else { f = c ^ (b | ~d); g = (7 * i) & 15; }
        const uint32_t t = d;
        d = c;
        c = b;
        b = b + flac_rotl(a + f + K[i] + m[g], R[(i >> 4) * 4 + (i & 3)]);
        a = t;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}
MSG_HD void flac_md5_init(uint32_t* st) { st[0] = 0x67452301; st[1] = 0xefcdab89; st[2] = 0x98badcfe; st[3] = 0x10325476; }
// the last blocks of a message of `total` bytes whose final `rest` (< 64) bytes are in tail
MSG_HD void flac_md5_finish(uint32_t* st, const uint8_t* tail, int rest, uint64_t total, uint8_t* out) {
    uint32_t m[16];
    uint8_t buf[128];
    for (int i = 0; i < 128; ++i) buf[i] = i < rest ? tail[i] : 0;
    buf[rest] = 0x80;
    const int blocks = rest < 56 ? 1 : 2;
    const uint64_t nbits = total * 8;
    for (int i = 0; i < 8; ++i) buf[64 * blocks - 8 + i] = (uint8_t)(nbits >> (8 * i));
    for (int b = 0; b < blocks; ++b) {
        for (int i = 0; i < 16; ++i)
            m[i] = (uint32_t)buf[64 * b + 4 * i] | ((uint32_t)buf[64 * b + 4 * i + 1] << 8) |
                   ((uint32_t)buf[64 * b + 4 * i + 2] << 16) | ((uint32_t)buf[64 * b + 4 * i + 3] << 24);
        flac_md5_block(st, m);
    }
    for (int i = 0; i < 16; ++i) out[i] = (uint8_t)(st[i >> 2] >> (8 * (i & 3)));
}

// ---- the host loop: the definition, one sequential bit writer over one signal ----
inline void flac_md5_host(const uint8_t* p, uint64_t n, uint8_t* out) {
    uint32_t st[4], m[16];
    flac_md5_init(st);
    uint64_t at = 0;
    for (; at + 64 <= n; at += 64) {
        for (int i = 0; i < 16; ++i)
            m[i] = (uint32_t)p[at + 4 * i] | ((uint32_t)p[at + 4 * i + 1] << 8) | ((uint32_t)p[at + 4 * i + 2] << 16) |
                   ((uint32_t)p[at + 4 * i + 3] << 24);
        flac_md5_block(st, m);
    }
    flac_md5_finish(st, p + at, (int)(n - at), n, out);
}

struct FlacWriter {
    uint8_t* p;
    int64_t n = 0;
    uint64_t acc = 0;
    int cnt = 0;
    void put(uint32_t v, int nb) {              // nb <= 32
        if (!nb) return;
        acc = (acc << nb) | v;
        cnt += nb;
        while (cnt >= 8) { p[n++] = (uint8_t)(acc >> (cnt - 8)); cnt -= 8; }
        acc &= (1ull << cnt) - 1;
    }
    void zeros(uint32_t q) { for (; q > 32; q -= 32) put(0, 32); put(0, (int)q); }
    void align() { if (cnt) put(0, 8 - cnt); }
};

// the best subframe of x[0 .. n) at depth d, by the definition's loops
inline void flac_best_seq(const int32_t* x, int n, int d, int bits, FlacBest* b) {
    std::memset(b, 0, sizeof(*b));
    bool same = true;
    for (int i = 1; i < n; ++i) same = same && x[i] == x[0];
    if (same) { b->type = FLAC_TYPE_CONSTANT; b->cost = 8 + d; return; }
    const long long verb = 8 + (long long)n * d;
    b->type = FLAC_TYPE_VERBATIM;
    b->cost = verb;
    if (n <= 4) return;
    auto resid = [&](int i, int o) -> int64_t {
        const int64_t a = x[i];
        switch (o) {
            case 0: return a;
            case 1: return a - x[i - 1];
            case 2: return a - 2 * (int64_t)x[i - 1] + x[i - 2];
            case 3: return a - 3 * (int64_t)x[i - 1] + 3 * (int64_t)x[i - 2] - x[i - 3];
            default: return a - 4 * (int64_t)x[i - 1] + 6 * (int64_t)x[i - 2] - 4 * (int64_t)x[i - 3] + x[i - 4];
        }
    };
    int o = 0;
    unsigned long long best_abs = 0;
    for (int t = 0; t < 5; ++t) {
        unsigned long long s = 0;
        for (int i = 4; i < n; ++i) { const int64_t r = resid(i, t); s += (unsigned long long)(r < 0 ? -r : r); }
        if (t == 0 || s < best_abs) { best_abs = s; o = t; }
    }
    std::vector<uint32_t> u((size_t)n, 0);
    for (int i = o; i < n; ++i) u[(size_t)i] = flac_fold(resid(i, o));
    const int kmax = flac_kmax(bits), pb = flac_pbits(bits);
    long long best = INT64_MAX;
    for (int p = 0; p <= 6; ++p) {
        if ((n & ((1 << p) - 1)) || (n >> p) <= o) continue;
        const int plen = n >> p;
        long long total = 0;
        uint8_t ks[64];
        for (int q = 0; q < (1 << p); ++q) {
            const int i0 = q == 0 ? o : q * plen, i1 = (q + 1) * plen;
            const long long c = i1 - i0;
            unsigned long long S = 0;
            for (int i = i0; i < i1; ++i) S += u[(size_t)i];
            const int k0 = flac_k0(c, S, kmax);
            long long bq = INT64_MAX;
            for (int k = k0 - 1; k <= k0 + 1; ++k) {
                if (k < 0 || k > kmax) continue;
                long long e = c * (k + 1);
                for (int i = i0; i < i1; ++i) e += u[(size_t)i] >> k;
                if (e < bq) { bq = e; ks[q] = (uint8_t)k; }
            }
            total += pb + bq;
        }
        if (total < best) {
            best = total;
            b->porder = (uint8_t)p;
            std::memcpy(b->k, ks, (size_t)1 << p);
        }
    }
    const long long fixed = 8 + (long long)o * d + 6 + best;
    if (fixed >= verb) { b->porder = 0; std::memset(b->k, 0, sizeof(b->k)); return; }
    b->type = FLAC_TYPE_FIXED;
    b->cost = fixed;
    b->order = (uint8_t)o;
}

inline void flac_sub_seq(FlacWriter& w, const int32_t* x, int n, int d, int bits, const FlacBest& s) {
    const uint32_t m = flac_mask(d);
    w.put(s.type == FLAC_TYPE_CONSTANT ? 0 : s.type == FLAC_TYPE_VERBATIM ? 2 : (8u + s.order) << 1, 8);
    if (s.type == FLAC_TYPE_CONSTANT) { w.put((uint32_t)x[0] & m, d); return; }
    if (s.type == FLAC_TYPE_VERBATIM) {
        for (int i = 0; i < n; ++i) w.put((uint32_t)x[i] & m, d);
        return;
    }
    const int o = s.order, plen = n >> s.porder;
    for (int i = 0; i < o; ++i) w.put((uint32_t)x[i] & m, d);
    w.put(bits == 16 ? 0 : 1, 2);
    w.put(s.porder, 4);
    for (int q = 0; q < (1 << s.porder); ++q) {
        const int k = s.k[q];
        w.put((uint32_t)k, flac_pbits(bits));
        for (int i = q == 0 ? o : q * plen; i < (q + 1) * plen; ++i) {
            int64_t r;
            const int64_t a = x[i];
            switch (o) {
                case 0: r = a; break;
                case 1: r = a - x[i - 1]; break;
                case 2: r = a - 2 * (int64_t)x[i - 1] + x[i - 2]; break;
                case 3: r = a - 3 * (int64_t)x[i - 1] + 3 * (int64_t)x[i - 2] - x[i - 3]; break;
                default: r = a - 4 * (int64_t)x[i - 1] + 6 * (int64_t)x[i - 2] - 4 * (int64_t)x[i - 3] + x[i - 4];
            }
            const uint32_t uu = flac_fold(r);
            w.zeros(uu >> k);
            w.put(1, 1);
            w.put(uu & ((1u << k) - 1u), k);
        }
    }
}

// One signal: pcm, n frames; out has room for flac_bound bytes.  rec->byte_off is left 0.
inline void flac_host(const uint8_t* pcm, int channels, int bits, int64_t n, int B, int64_t sr, bool md5, uint8_t* out,
                      FlacRec* rec) {
    std::memset(rec, 0, sizeof(*rec));
    rec->samples = n;
    std::vector<int32_t> ch[4];
    for (auto& v : ch) v.resize((size_t)B);
    FlacWriter w{out};
    for (int64_t j = 0; j * B < n; ++j) {
        const int bn = (int)(n - j * B < B ? n - j * B : B);
        const int64_t start = w.n;
        for (int i = 0; i < bn; ++i) {
            const int64_t f = j * B + i;
            const int32_t l = flac_load(pcm, bits, f * channels), r = channels == 2 ? flac_load(pcm, bits, f * channels + 1) : l;
            for (int c = 0; c < 4; ++c) ch[c][(size_t)i] = flac_chan(l, r, c);
        }
        FlacBest best[4];
        for (int c = 0; c < (channels == 2 ? 4 : 1); ++c) flac_best_seq(ch[c].data(), bn, bits + (c == 3), bits, &best[c]);
        uint8_t hdr[FLAC_HDR_MAX];
        FlacPlan plan;
        // the header's length does not depend on the assignment
        const int hb = flac_header(hdr, B, bn, sr, channels == 2 ? 0 : -1, bits, j);
        flac_assign(best, channels, hb, &plan);
        flac_header(hdr, B, bn, sr, plan.assign, bits, j);
        for (int i = 0; i < hb; ++i) w.put(hdr[i], 8);
        for (int s = 0; s < channels; ++s) {
            const int c = flac_assign_chan(plan.assign, s);
            flac_sub_seq(w, ch[c].data(), bn, bits + (c == 3), bits, plan.sub[s]);
            const int t = plan.sub[s].type;
            (t == FLAC_TYPE_CONSTANT ? rec->constant : t == FLAC_TYPE_VERBATIM ? rec->verbatim : rec->fixed) += 1;
        }
        w.align();
        uint32_t crc = 0;
        for (int64_t i = start; i < w.n; ++i) crc = flac_crc16(crc, out[i]);
        w.put(crc, 16);
        const int32_t fb = (int32_t)(w.n - start);
        if (channels == 2) rec->assign[plan.assign] += 1;
        rec->min_frame = rec->frames == 0 || fb < rec->min_frame ? fb : rec->min_frame;
        rec->max_frame = fb > rec->max_frame ? fb : rec->max_frame;
        rec->frames += 1;
    }
    rec->bytes = w.n;
    if (md5) {
        flac_md5_host(pcm, (uint64_t)n * channels * (bits / 8), rec->md5);
        rec->flags |= 1;
    }
}
