// truepeak.h — ITU-R BS.1770-4 Annex 2 true peak (msg_truepeak / msg_truepeak_host):
// the definition, shared by the device kernels (kernels_truepeak.h), the host
// planning in msgpu.hip and the host reference below (built into libmsgpu and
// into the host sanitizer build).  Plain C++.
//
// Oversampling: OS(sr) = 4 for sr < 96 000, 2 for 96 000 <= sr < 192 000, 1 from
// 192 000 on (Annex 2 asks for 4 x at 48 kHz and proportionally less above).
//
// Interpolator: a Nyquist (L-band) filter, TP_Z = 12 zero crossings per side, Kaiser
// window with beta = 7, designed in float64:
//   g[i]   = sinc(i / OS) kaiser(2 Z OS + 1, 7)[i + Z OS],  i = -Z OS .. Z OS
//   t_p[q] = g[p + q OS - Z OS],  q = 0 .. 23,  p = 1 .. OS - 1,
// each phase divided by its own sum (unit DC gain), then rounded once to float32.
// Phase 0 is the identity and is not evaluated (the sample peak covers it); phases
// p and OS - p are mirror images, and the table is built that way.
//
// Oversampled values of one channel, x zero outside [0, n):
//   y_p[m] = sum over q = 0 .. 23 of t_p[q] x[m + Z - q],  m = -1 .. n - 1
// (y_p[m] lies between frames m and m + 1), in float32 in this order:
//   acc = 0;  acc = fmaf(t_p[q], x[m + Z - q], acc)  for q = 0, 1, .. 23.
// A zero of the extension may be multiplied or skipped: it changes at most the sign
// of a zero, which |.| removes.
//
// Record: peak = max |x|, true_peak = max(peak, max |y_p[m]|) over channels, phases
// and m, dbtp = 20 log10(true_peak) (-inf for 0).  Every max is taken over the bit
// patterns of |v| as unsigned integers: free of order, and a NaN anywhere (its bits
// lie above infinity's) gives a NaN peak and true peak on the host and the device
// alike.  dbtp is tp_db below on both sides, so the records agree to the bit.
//
// The device cuts m' = m + 1 = 0 .. n into tiles of TP_TILE values; tile t stages
// frames [t TP_TILE - Z, t TP_TILE + TP_TILE + Z - 1) and takes the sample peak of
// frames [t TP_TILE, t TP_TILE + TP_TILE); DESIGN.md "True peak" has the lane mapping.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstring>
#include "msg_common.h"

constexpr int TP_Z = 12;                  // zero crossings per side
constexpr int TP_TAPS = 2 * TP_Z;         // taps of a phase
constexpr int TP_T = 256;                 // threads per tile workgroup (4 waves)
constexpr int TP_TILE = 2048;             // oversampled positions m' (and frames) per tile
constexpr int TP_ROW = TP_TILE + TP_TAPS; // LDS floats per staged channel (TP_TILE + 23 used)
constexpr int TP_FT = 64;                 // threads of the per-signal fold (one wave)
constexpr int TP_GAIN_PER = 16;           // k_truepeak_gain: frames per thread
constexpr int TP_GAIN_TILE = TP_T * TP_GAIN_PER;
// the table uploaded once with the context (floats): phase p of OS at TP_TAB_OSx + (p - 1) TP_TAPS
constexpr int TP_TAB_OS2 = 0;
constexpr int TP_TAB_OS4 = TP_TAPS;
constexpr int TP_TAB_N = TP_TAPS + 3 * TP_TAPS;

struct TruePeakRec {                      // layout of msg_truepeak_rec
    double true_peak, peak, dbtp, gain;
    int32_t os, pad;
};

MSG_HD int tp_os(int64_t sr) { return sr < 96000 ? 4 : (sr < 192000 ? 2 : 1); }
MSG_HD int tp_tab_at(int os) { return os == 2 ? TP_TAB_OS2 : TP_TAB_OS4; }
// tiles of a signal: m' = 0 .. n, none for an empty signal
inline int64_t tp_tiles(int64_t n) { return n > 0 ? n / TP_TILE + 1 : 0; }

// ---- bit patterns --------------------------------------------------------------------
MSG_HD uint32_t tp_abs_bits(float v) {
    uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = __float_as_uint(v);
#else
    std::memcpy(&b, &v, 4);
#endif
    return b & 0x7fffffffu;
}
MSG_HD double tp_from_bits(uint32_t b) {
    float v;
#if defined(__HIP_DEVICE_COMPILE__)
    v = __uint_as_float(b);
#else
    std::memcpy(&v, &b, 4);
#endif
    return (double)v;
}

// ---- dbtp: 20 log10(v), correctly rounded ---------------------------------------------
// Host and device must give the same bits, so this is no library log10: it is
// evaluated in double-double arithmetic (about 100 bits) from float64 sums, quotients
// and explicit fused multiply-adds only (no plain product, see tp_dd_mul), which both
// compilers keep as written, and rounded once.  v = 2^e m with m in [2^-1/2, 2^1/2), s = (m - 1) / (m + 1),
// ln m = 2 s (1 + s^2 / 3 + s^4 / 5 + ..) with s^2 <= 0.0295 (24 terms: 0.0295^24 < 2^-120),
// 20 log10 v = 20 (e log10 2 + ln m log10 e).
struct TpDD { double hi, lo; };
MSG_HD TpDD tp_dd_sum(double a, double b) {           // a + b exactly (Knuth)
    const double s = a + b, bb = s - a;
    return TpDD{s, (a - (s - bb)) + (b - bb)};
}
MSG_HD TpDD tp_dd_fast(double a, double b) {          // a + b exactly, |a| >= |b|
    const double s = a + b;
    return TpDD{s, b - (s - a)};
}
MSG_HD TpDD tp_dd_add(TpDD a, TpDD b) {
    const TpDD s = tp_dd_sum(a.hi, b.hi), t = tp_dd_sum(a.lo, b.lo);
    const TpDD u = tp_dd_fast(s.hi, s.lo + t.hi);
    return tp_dd_fast(u.hi, u.lo + t.lo);
}
MSG_HD TpDD tp_dd_mul(TpDD a, TpDD b) {
    // the product as a fused step too: a plain a.hi * b.hi may be contracted by the device
    // compiler into the sums that use it (p + c, s - p), which then count its rounding error twice
    const double p = __builtin_fma(a.hi, b.hi, 0.0);
    const double e = __builtin_fma(a.hi, b.hi, -p);
    const double c = __builtin_fma(a.hi, b.lo, __builtin_fma(a.lo, b.hi, e));
    return tp_dd_fast(p, c);
}
MSG_HD TpDD tp_dd_div(TpDD a, TpDD b) {
    const double q1 = a.hi / b.hi;
    const TpDD r = tp_dd_add(a, tp_dd_mul(TpDD{-q1, 0.0}, b));
    const double q2 = r.hi / b.hi;
    const TpDD r2 = tp_dd_add(r, tp_dd_mul(TpDD{-q2, 0.0}, b));
    const double q3 = r2.hi / b.hi;
    const TpDD q = tp_dd_fast(q1, q2);
    return tp_dd_add(q, TpDD{q3, 0.0});
}
MSG_HD double tp_db(double v) {
    if (!(v == v)) return v;                                            // NaN stays
    if (v <= 0.0) return -__builtin_inf();
    if (v > 1.7976931348623157e308) return v;                           // +inf
    uint64_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = (uint64_t)__double_as_longlong(v);
#else
    std::memcpy(&u, &v, 8);
#endif
    int e = (int)((u >> 52) & 0x7ff) - 1023;                            // v comes from a float32: normal here
    u = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
#if defined(__HIP_DEVICE_COMPILE__)
    m = __longlong_as_double((long long)u);
#else
    std::memcpy(&m, &u, 8);
#endif
    if (m > 1.4142135623730951) { m *= 0.5; ++e; }                      // m in (2^-1/2, 2^1/2]
    const TpDD s = tp_dd_div(TpDD{m - 1.0, 0.0}, tp_dd_sum(m, 1.0));    // m - 1 is exact
    const TpDD s2 = tp_dd_mul(s, s);
    TpDD acc{0.0, 0.0};
    for (int k = 23; k >= 1; --k) {                                     // Horner in s^2 over 1 / (2k + 1)
        const double d = (double)(2 * k + 1), h = 1.0 / d;
        const TpDD c{h, __builtin_fma(-h, d, 1.0) / d};
        acc = tp_dd_mul(tp_dd_add(acc, c), s2);
    }
    acc = tp_dd_add(acc, TpDD{1.0, 0.0});
    const TpDD lnm = tp_dd_mul(tp_dd_mul(s, TpDD{2.0, 0.0}), acc);
    const TpDD log10_2{0x1.34413509f79ffp-2, -0x1.9dc1da994fd21p-59};
    const TpDD log10_e{0x1.bcb7b1526e50ep-2, 0x1.95355baaafad3p-57};
    const TpDD l = tp_dd_add(tp_dd_mul(TpDD{(double)e, 0.0}, log10_2), tp_dd_mul(lnm, log10_e));
    const TpDD r = tp_dd_mul(l, TpDD{20.0, 0.0});
    return r.hi + r.lo;
}

// ---- the interpolator (host) ------------------------------------------------------------
inline double tp_i0(double x) {                       // modified Bessel function I0 by its series
    const double h = 0.5 * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; ++k) {
        term *= (h / k) * (h / k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}
// phase p of OS in float64, 24 taps with unit sum; p <= OS / 2 (the others are mirror images)
inline void tp_phase(int os, int p, double* t) {
    const double pi = 3.14159265358979323846, beta = 7.0;
    double sum = 0.0;
    for (int q = 0; q < TP_TAPS; ++q) {
        const int i = p + (q - TP_Z) * os;
        const double a = pi * (double)i / (double)os, r = (double)i / (double)(TP_Z * os);
        t[q] = std::sin(a) / a * (tp_i0(beta * std::sqrt(1.0 - r * r)) / tp_i0(beta));
        sum += t[q];
    }
    for (int q = 0; q < TP_TAPS; ++q) t[q] /= sum;
}
// the table of both factors in float32 (TP_TAB_N floats)
inline void tp_table(float* tab) {
    double t[TP_TAPS];
    tp_phase(2, 1, t);
    for (int q = 0; q < TP_TAPS; ++q) tab[TP_TAB_OS2 + q] = (float)t[q];
    tp_phase(4, 1, t);
    for (int q = 0; q < TP_TAPS; ++q) {
        tab[TP_TAB_OS4 + q] = (float)t[q];
        tab[TP_TAB_OS4 + 2 * TP_TAPS + q] = (float)t[TP_TAPS - 1 - q];
    }
    tp_phase(4, 2, t);
    for (int q = 0; q < TP_TAPS; ++q) tab[TP_TAB_OS4 + TP_TAPS + q] = (float)t[q];
}

// the record from the two maxima (bit patterns)
MSG_HD void tp_finish(uint32_t peak_bits, uint32_t over_bits, int os, TruePeakRec* rec) {
    const uint32_t tb = over_bits > peak_bits ? over_bits : peak_bits;
    rec->peak = tp_from_bits(peak_bits);
    rec->true_peak = tp_from_bits(tb);
    rec->dbtp = tp_db(rec->true_peak);
    rec->gain = 0.0;
    rec->os = os;
    rec->pad = 0;
}

// ---- the host reference: the definition as one loop ---------------------------------------
// x: n frames of `channels` interleaved float32 words
inline void tp_host(const float* x, int channels, int64_t n, int64_t sr, TruePeakRec* rec) {
    const int os = tp_os(sr);
    float tab[TP_TAB_N];
    tp_table(tab);
    const float* taps = tab + tp_tab_at(os);
    uint32_t pk = 0, tp = 0;
    for (int64_t i = 0; i < n * channels; ++i) {
        const uint32_t b = tp_abs_bits(x[i]);
        pk = b > pk ? b : pk;
    }
    if (n > 0)
        for (int ch = 0; ch < channels; ++ch)
            for (int64_t m = -1; m < n; ++m)
                for (int p = 1; p < os; ++p) {
                    const float* t = taps + (p - 1) * TP_TAPS;
                    float acc = 0.0f;
                    for (int q = 0; q < TP_TAPS; ++q) {
                        const int64_t f = m + TP_Z - q;
                        const float v = f >= 0 && f < n ? x[f * channels + ch] : 0.0f;
                        acc = __builtin_fmaf(t[q], v, acc);
                    }
                    const uint32_t b = tp_abs_bits(acc);
                    tp = b > tp ? b : tp;
                }
    tp_finish(pk, tp, os, rec);
}
