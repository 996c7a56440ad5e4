// limit.h — the look-ahead true-peak limiter (msg_limit / msg_limit_host): the
// definition, shared by the device kernels (kernels_limit.h), the host planning in
// signal_abi.inc and the host reference below (built into libmsgpu and into the host
// sanitizer build).  Plain C++.  The interpolator, its table and the bit-pattern maxima
// are truepeak.h's.
//
// Inputs: one signal x of n frames, CH in {1, 2} interleaved float32 channels at sr Hz,
// OS = tp_os(sr), a linear ceiling c32 = (float)c > 0 and a look-ahead of L >= 1 frames.
// Everything below is float32 in one fixed order, so the host and the device agree to
// the bit.
//
// 1. Envelope.  y_p[m] as in truepeak.h (acc = fmaf(t_p[q], x[m + Z - q], acc), q = 0 .. 23,
//    zeros outside [0, n)), the value between frames m and m + 1.  e[m], m = 0 .. n - 1, is
//    the maximum over the channels of |x[m]|, |y_p[m - 1]| and |y_p[m]|, p = 1 .. OS - 1,
//    taken over bit patterns (tp_abs_bits): every oversampled value belongs to both of its
//    neighbouring frames, the channels share one gain, and a NaN is carried through.
// 2. Demand.  r[m] = e[m] > c32 ? c32 / e[m] : 1, and r = 1 outside [0, n).  The quotient is
//    IEEE correctly rounded on both sides: the plain `/` of the language.  The device TU is
//    built with -fhip-fp32-correctly-rounded-divide-sqrt spelled out (build.py) and without
//    any fast-math flag, so `/` is the v_div_scale / v_div_fmas / v_div_fixup sequence, which
//    rounds to nearest even and keeps subnormal quotients; no reciprocal, no __fdividef.
// 3. Hold.  h[j] = min of r[k] over |k - j| <= L + TP_Z.  A minimum is free of order.  The
//    extra TP_Z keeps the gain flat over the interpolator's whole window around an
//    isolated peak.
// 4. Smooth.  w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (2 L + 2)), k = 0 .. 2 L, in float64,
//    divided by their float64 sum and rounded once to float32 (lim_weights; the host
//    builds the table for every call and uploads it, so both sides read the same bits).
//    s[m]: acc = 0; acc = fmaf(w[k], h[m - L + k], acc) for k = 0, 1, .. 2 L.  The table is
//    padded with zeros to a multiple of four taps: fmaf(0, h, acc) = acc for the finite h.
// 5. Apply.  Frame m is in reach when some frame k with r[k] < 1 has |k - m| <= 2 L + TP_Z
//    (equally: some h of its window is below 1).
//      in reach:      g[m] = min(s[m], r[m], 1 - 2^-24)
//      out of reach:  g[m] = 1
//    Where g[m] < 1 every channel of frame m becomes g[m] * x in one float32 multiply; where
//    g[m] = 1 the frame is not written and keeps its bits.
//    Why the reach is part of the definition and not left to s[m] < 1: the float32 weights'
//    chained sum over an all-ones window is 1 only to within (2 L + 1) 2^-25 and may fall
//    below it, which would rewrite frames nothing reaches; and at the edge of the reach
//    the Hann weights are so small that s rounds to that same all-ones value, so "g < 1"
//    would depend on float32 resolution.  With the rule, the frames with g < 1 are exactly
//    the frames in reach; the cap costs such an edge frame one unit in the last place.
//
// NaN rule: a signal with a NaN in its envelope (a NaN sample, or an oversampled value of
// infinities that cancel) is left untouched, state 2.  It is decided per signal before
// anything is written.  e = +inf gives r = 0.
//
// Guarantees.
//  a. Sample peak <= c32 (1 + 2^-22).  g <= r and |x[m]| <= e[m].  Where e > c32:
//     r = c32 / e (1 + d1), |d1| <= 2^-24, and the written sample is g x (1 + d2), so
//     |g x| (1 + d2) <= (c32 / e)(1 + d1) e (1 + d2) <= c32 (1 + 2^-24)^2 < c32 (1 + 2^-22)
//     (the third rounding, of c to c32, is inside c32; the margin covers a subnormal
//     quotient's coarser rounding).  Where e <= c32 the sample was under the ceiling and only shrinks.
//  b. An isolated peak, no other over-ceiling frame within 2 L + 2 TP_Z frames of frame k,
//     comes out at the ceiling to within rounding.  r = 1 except at k and at the neighbours
//     that share its oversampled values; r_min, the least of them, is c32 / tp to one
//     rounding, tp the peak's true peak.  h = r_min on |j - k| <= L + TP_Z, so every s[m] with
//     |m - k| <= TP_Z sums r_min alone: s = r_min S with S the chained sum of the weights,
//     |S - 1| <= (2 L + 1) 2^-25, and g = min(s, r) is r_min S or r_min.  Every frame of the
//     interpolator's 24-tap windows around the peak is scaled by that g to 2^-24, so the
//     limited true peak is g tp = c32 (1 + d), |d| <= (2 L + 4) 2^-24, and far less in
//     practice (the chain's roundings do not all point one way).
//
// Not guaranteed: on dense over-ceiling material g moves inside the interpolator's window
// and the re-interpolated peak can overshoot c; the export chain closes that
// with a static trim (msg_truepeak + msg_truepeak_gain) after the limiter.
//
// Record (msg_limit_rec): min_gain, the minimum of g as a bit pattern of positive floats
// (1 if nothing was limited); reduction_db = 0 - tp_db(min_gain); limited_frames, the
// frames with g < 1; lookahead = L; state 0 untouched, 1 limited, 2 NaN: left as it was.
//
// The device: k_limit_env over tiles of LIM_ENV_TILE frames writes r, k_limit_apply over
// tiles of lim_tile(L) frames stages r with a halo of lim_halo(L) frames per side.
#pragma once
#include <stdint.h>
#include <cmath>
#include <vector>
#include "truepeak.h"

constexpr int LIM_L_MAX = 4096;                 // 10 ms at 384 kHz
constexpr int LIM_ENV_T = 256;                  // threads of k_limit_env
constexpr int LIM_ENV_TILE = TP_TILE;           // frames per envelope tile
constexpr int LIM_ENV_ROW = LIM_ENV_TILE + 28;  // LDS floats per staged channel: positions 0 .. TILE + 3 read 27 more
constexpr int LIM_FT = 64;                      // threads of the per-signal folds (one wave)
constexpr uint32_t LIM_ONE = 0x3f800000u, LIM_BELOW_ONE = 0x3f7fffffu, LIM_INF = 0x7f800000u;
// the per-signal state between the kernels (the record's state is 0 for LIM_SKIP)
constexpr int LIM_RUN = 0, LIM_NAN = 2, LIM_SKIP = 3;

struct LimitRec {                               // layout of msg_limit_rec
    double min_gain, reduction_db;
    int64_t limited_frames;
    int32_t lookahead, state;
};

// the apply kernel's tile, its halo per side, its threads and its staged floats
MSG_HD int lim_halo(int L) { return 2 * L + TP_Z; }
MSG_HD int lim_tile(int L) { return L <= 256 ? 2048 : (L <= 512 ? 4096 : (L <= 1024 ? 8192 : 16384)); }
MSG_HD int lim_threads(int L) { return L <= 512 ? 256 : 1024; }
MSG_HD int lim_staged(int L) { return lim_tile(L) + 2 * lim_halo(L); }   // a multiple of 4
inline int64_t lim_tiles(int64_t n, int L) { return (n + lim_tile(L) - 1) / lim_tile(L); }
inline int64_t lim_env_tiles(int64_t n) { return (n + LIM_ENV_TILE - 1) / LIM_ENV_TILE; }
inline int lim_taps4(int L) { return (2 * L + 1 + 3) / 4 * 4; }
// LDS bytes of one apply workgroup: the staged r, one 64-bit word of "r < 1" bits and one
// prefix count per 64 staged floats (each rounded up to 16 bytes), the reduction's 32 words
inline int lim_words64(int L) { return (lim_staged(L) + 63) / 64 + 1; }
inline size_t lim_lds_bytes(int L) {
    return (size_t)lim_staged(L) * 4 + 2 * (((size_t)lim_words64(L) * 8 + 15) & ~(size_t)15) + 64 * 4;
}

MSG_HD float lim_from_bits(uint32_t b) {
    float v;
#if defined(__HIP_DEVICE_COMPILE__)
    v = __uint_as_float(b);
#else
    std::memcpy(&v, &b, 4);
#endif
    return v;
}
MSG_HD uint32_t lim_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// step 2 from the envelope's bit pattern; a NaN envelope (bits above infinity's) demands nothing
MSG_HD float lim_demand(uint32_t e_bits, float c32) {
    const float e = lim_from_bits(e_bits);
    if (!(e > c32)) return 1.0f;
    return c32 / e;
}

// step 5 for a frame in reach
MSG_HD float lim_gain(float s, float r) {
    const float cap = lim_from_bits(LIM_BELOW_ONE);
    float g = s < r ? s : r;
    return g < cap ? g : cap;
}

// the record from the per-signal state, the least gain's bits and the count
MSG_HD void lim_finish(int state, uint32_t g_bits, int64_t count, int L, LimitRec* rec) {
    const bool ran = state == LIM_RUN && count > 0;
    rec->min_gain = ran ? (double)lim_from_bits(g_bits) : 1.0;
    rec->reduction_db = 0.0 - tp_db(rec->min_gain);
    rec->limited_frames = ran ? count : 0;
    rec->lookahead = L;
    rec->state = state == LIM_NAN ? 2 : (ran ? 1 : 0);
}

// step 4's table: lim_taps4(L) floats, the 2 L + 1 weights and the zero padding
inline void lim_weights(int L, float* w) {
    const double pi = 3.14159265358979323846;
    const int K = 2 * L + 1;
    std::vector<double> d((size_t)K);
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        d[k] = 0.5 - 0.5 * std::cos(2.0 * pi * (double)(k + 1) / (double)(2 * L + 2));
        sum += d[k];
    }
    for (int k = 0; k < K; ++k) w[k] = (float)(d[k] / sum);
    for (int k = K; k < lim_taps4(L); ++k) w[k] = 0.0f;
}

// ---- the host reference: the definition as one loop, x limited in place ----------------
inline void lim_host(float* x, int channels, int64_t n, int64_t sr, float c32, int L, LimitRec* rec) {
    lim_finish(LIM_RUN, LIM_ONE, 0, L, rec);
    if (n <= 0) return;
    const int os = tp_os(sr);
    float tab[TP_TAB_N];
    tp_table(tab);
    const float* taps = tab + tp_tab_at(os);
    // pos[i]: the maximum over channels and phases of |y_p[i - 1]|, i = 0 .. n
    std::vector<uint32_t> pos((size_t)n + 1, 0u);
    for (int ch = 0; ch < channels; ++ch)
        for (int64_t i = 0; i <= n; ++i)
            for (int p = 1; p < os; ++p) {
                const float* t = taps + (p - 1) * TP_TAPS;
                float acc = 0.0f;
                for (int q = 0; q < TP_TAPS; ++q) {
                    const int64_t f = i - 1 + TP_Z - q;
                    const float v = f >= 0 && f < n ? x[f * channels + ch] : 0.0f;
                    acc = __builtin_fmaf(t[q], v, acc);
                }
                pos[(size_t)i] = lim_umax(pos[(size_t)i], tp_abs_bits(acc));
            }
    std::vector<float> r((size_t)n);
    std::vector<int64_t> below((size_t)n + 1, 0);          // below[m]: frames k < m with r[k] < 1
    bool nan = false;
    for (int64_t m = 0; m < n; ++m) {
        uint32_t e = lim_umax(pos[(size_t)m], pos[(size_t)m + 1]);
        for (int ch = 0; ch < channels; ++ch) e = lim_umax(e, tp_abs_bits(x[m * channels + ch]));
        nan = nan || e > LIM_INF;
        r[(size_t)m] = lim_demand(e, c32);
        below[(size_t)m + 1] = below[(size_t)m] + (r[(size_t)m] < 1.0f ? 1 : 0);
    }
    if (nan) {
        lim_finish(LIM_NAN, LIM_ONE, 0, L, rec);
        return;
    }
    if (below[(size_t)n] == 0) return;
    auto any_below = [&](int64_t lo, int64_t hi) {        // some r < 1 on frames lo .. hi
        lo = lo < 0 ? 0 : lo;
        hi = hi > n - 1 ? n - 1 : hi;
        return lo <= hi && below[(size_t)hi + 1] - below[(size_t)lo] > 0;
    };
    // h[j], j = -L .. n + L - 1, at index j + L
    const int R = L + TP_Z, reach = lim_halo(L);
    std::vector<float> h((size_t)(n + 2 * (int64_t)L), 1.0f);
    for (int64_t j = -L; j < n + L; ++j) {
        if (!any_below(j - R, j + R)) continue;
        const int64_t lo = j - R < 0 ? 0 : j - R, hi = j + R > n - 1 ? n - 1 : j + R;
        float v = 1.0f;
        for (int64_t k = lo; k <= hi; ++k) v = r[(size_t)k] < v ? r[(size_t)k] : v;
        h[(size_t)(j + L)] = v;
    }
    std::vector<float> w((size_t)lim_taps4(L));
    lim_weights(L, w.data());
    uint32_t g_min = LIM_ONE;
    int64_t count = 0;
    for (int64_t m = 0; m < n; ++m) {
        if (!any_below(m - reach, m + reach)) continue;
        float acc = 0.0f;
        for (int k = 0; k <= 2 * L; ++k) acc = __builtin_fmaf(w[(size_t)k], h[(size_t)(m + k)], acc);
        const float g = lim_gain(acc, r[(size_t)m]);
        const uint32_t gb = tp_abs_bits(g);
        g_min = gb < g_min ? gb : g_min;
        ++count;
        for (int ch = 0; ch < channels; ++ch) x[m * channels + ch] = g * x[m * channels + ch];
    }
    lim_finish(LIM_RUN, g_min, count, L, rec);
}
