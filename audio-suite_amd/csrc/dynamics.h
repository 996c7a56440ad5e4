// dynamics.h — the delivery compressor (msg_dynamics / msg_dynamics_host): the definition,
// shared by the device kernels (kernels_dynamics.h), the entry points in signal_abi.inc and
// host_abi.inc and the host reference below (built into libmsgpu and into the host sanitizer
// build).  Plain C++.  DESIGN.md "4l. Dynamics".
//
// Inputs: one signal x of n frames, CH in {1, 2} interleaved float32 channels, linked (one
// gain per frame serves both).  Every envelope value is an int64 in [0, 2^40] in units of
// u = 2^-32 dB.
//
// 1. Level.  p[f] = max over the channels of |x|, taken over bit patterns (a NaN or an
//    infinity has the largest pattern and marks the signal, see below).
// 2. Demand.  d[f] = 0 when p <= p0, p0 the float32 at or just under the linear level of
//    threshold_db - knee_db / 2 (dyn_p0, formed once per call on the host).  Otherwise, in
//    float64 with contraction off: lev = (20 log10 2) dyn_log2(p), over = lev - threshold_db,
//    s = 1 - 1 / ratio (1 for ratio = +inf), W = knee_db, and the soft knee of Giannoulis,
//    Massberg and Reiss (JAES 2012)
//        curve = s over                      2 over >  W
//              = s (over + W / 2)^2 / (2 W)  2 |over| <= W  (never at W = 0)
//              = 0                           2 over < -W
//    d = (int64) floor(curve 2^32 + 0.5) clamped to [0, 2^40].
// 3. Hold.  dh[f] = max of d[f - k], 0 <= k <= hold_frames, frames before the signal 0.
// 4. Release, forward.   F[f] = max(F[f - 1] - release_step, dh[f]), F[-1] = 0.
// 5. Attack, backward.   B[f] = max(B[f + 1] - attack_step, d[f]),   B[n] = 0: the gain comes
//    down along a straight line in dB ahead of a peak and has fully arrived at it.
// 6. Envelope.  E[f] = max(F[f], B[f]) >= d[f]: a peak is never under-compressed.
// 7. Gain.  g = (float) dyn_exp2((makeup_db - E 2^-32) (log2 10 / 20)), the float64 rounded
//    once; y = x g in float32 per channel, in place.  dyn_exp2(0) is exactly 1: a frame with
//    g = 1 is not written and keeps its bits.
//
// Steps 4 and 5 are max-plus recurrences over integers: y <- max(y - step, d) with the
// subtraction clamped at 0 (dyn_dec), so no intermediate leaves [0, 2^40].  A run of L frames
// acts on its incoming value c as c -> max(c - R, C) with R = min(L step, 2^40) and C the run's
// result from c = 0 (DynSeg); two runs in a row compose to (R1 + R2, max(C1 - R2, C2)) with the
// same clamps (dyn_join).  Integer max and + are associative and exact, so the envelope may be
// evaluated per lane chunk, per wave, per tile and over tiles in any grouping and is the same
// bits as the sequential loop below, for any tiling and any batch.
//
// dyn_log2 and dyn_exp2 are float64 adds, multiplies and one IEEE division in one written
// order, contraction off, no libm and no ocml call: the host and the device agree to the bit.
// dyn_log2 is within 2^-40 (absolute) of log2 over every positive float32, dyn_exp2 within
// 2^-40 (relative) of 2^x over [-60, 60]; that puts their error 2^8 under the half-unit
// rounding of d.
//
// Non-finite input: a signal with a NaN or an infinity anywhere is left as it was in every
// frame, state 2 (the limiter's rule).
//
// Record (msg_dynamics_rec), integers only, so any folding order gives the same bits:
// max_e, sum_e16 = sum over frames of E >> 16, reduced_frames = frames with E > 0,
// state 0 untouched, 1 compressed (some E > 0, or a makeup gain over a signal with frames),
// 2 non-finite; hold_frames.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "msg_common.h"

constexpr int DYN_T = 256;                      // threads per tile workgroup (4 waves)
constexpr int DYN_C = 16;                       // frames per lane chunk
constexpr int DYN_TILE = DYN_T * DYN_C;         // 4096 frames
constexpr int DYN_HOLD_MAX = 4096;              // 10 ms at 384 kHz; at most one tile of halo
constexpr int64_t DYN_MAX = (int64_t)1 << 40;   // 256 dB: the largest envelope value and step
constexpr uint32_t DYN_INF = 0x7f800000u;

struct DynRec {                                 // layout of msg_dynamics_rec
    int64_t max_e, sum_e16, reduced_frames;
    int32_t state, hold_frames;
};
struct DynOpts {                                // layout of msg_dynamics_opts
    double threshold_db, ratio, knee_db, makeup_db;
    int64_t attack_step, release_step;
    int32_t hold_frames, flags;
};
// what the kernels take by value
struct DynPar {
    double thr, knee, slope, makeup;
    int64_t astep, rstep;
    float p0;
    int32_t hold;
};
// a run of frames as it acts on the value that enters it: c -> max(c - R, C)
struct DynSeg {
    int64_t R, C;
};

MSG_HD uint64_t dyn_bits(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(v);
#else
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
#endif
}
MSG_HD double dyn_from_bits(uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)b);
#else
    double v;
    std::memcpy(&v, &b, 8);
    return v;
#endif
}
MSG_HD uint32_t dyn_abs_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v) & 0x7fffffffu;
#else
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b & 0x7fffffffu;
#endif
}
MSG_HD float dyn_float(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(b);
#else
    float v;
    std::memcpy(&v, &b, 4);
    return v;
#endif
}

// log2 of a positive finite float32.  The float64 of a float32, denormals included, is normal:
// its exponent and mantissa are split by bits, m in [1, 2) is halved above sqrt 2 so that
// t = (m - 1) / (m + 1) has |t| <= 0.1716 (m - 1 is exact), and log2 m = (2 / ln 2) atanh t is
// the odd series to t^21: the first term left out is below 2e-17, the roundings below 1e-15.
MSG_HD double dyn_log2(float p) {
#if defined(__clang__)                          // g++ for x86-64 has no fused instruction to contract into
#pragma clang fp contract(off)
#endif
    const uint64_t b = dyn_bits((double)p);
    int e = (int)(b >> 52) - 1023;
    double m = dyn_from_bits((b & 0x000fffffffffffffULL) | 0x3ff0000000000000ULL);
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        e += 1;
    }
    const double t = (m - 1.0) / (m + 1.0), z = t * t;
    double q = 1.0 / 21.0;
    q = q * z + 1.0 / 19.0;
    q = q * z + 1.0 / 17.0;
    q = q * z + 1.0 / 15.0;
    q = q * z + 1.0 / 13.0;
    q = q * z + 1.0 / 11.0;
    q = q * z + 1.0 / 9.0;
    q = q * z + 1.0 / 7.0;
    q = q * z + 1.0 / 5.0;
    q = q * z + 1.0 / 3.0;
    q = q * z + 1.0;
    return (double)e + (t * q) * 2.8853900817779268;
}

// 2^x for |x| <= 60: k the nearest integer (x - k is exact), the Taylor polynomial of exp to
// u^13 at u = (x - k) ln 2, |u| <= 0.3466 (the first term left out is below 5e-18), times 2^k
// set by bits.  x = 0 gives exactly 1: every Horner step is q 0 + c.
MSG_HD double dyn_exp2(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int k = (int)(x < 0.0 ? x - 0.5 : x + 0.5);
    const double u = (x - (double)k) * 0.6931471805599453;
    double q = 1.0 / 6227020800.0;
    q = q * u + 1.0 / 479001600.0;
    q = q * u + 1.0 / 39916800.0;
    q = q * u + 1.0 / 3628800.0;
    q = q * u + 1.0 / 362880.0;
    q = q * u + 1.0 / 40320.0;
    q = q * u + 1.0 / 5040.0;
    q = q * u + 1.0 / 720.0;
    q = q * u + 1.0 / 120.0;
    q = q * u + 1.0 / 24.0;
    q = q * u + 1.0 / 6.0;
    q = q * u + 0.5;
    q = q * u + 1.0;
    q = q * u + 1.0;
    return q * dyn_from_bits((uint64_t)(k + 1023) << 52);
}

// step 2 from the level's bit pattern; a non-finite level demands nothing (its signal is skipped)
MSG_HD int64_t dyn_demand(uint32_t p_bits, const DynPar& par) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = dyn_float(p_bits);
    if (p_bits >= DYN_INF || !(p > par.p0)) return 0;
    const double lev = 6.020599913279624 * dyn_log2(p);
    const double over = lev - par.thr, o2 = 2.0 * over, W = par.knee;
    double curve;
    if (o2 > W) {
        curve = par.slope * over;
    } else if (o2 < -W || !(W > 0.0)) {
        curve = 0.0;
    } else {
        const double t = over + 0.5 * W;
        curve = par.slope * (t * t) / (2.0 * W);
    }
    const double v = curve * 4294967296.0 + 0.5;
    if (!(v >= 1.0)) return 0;
    return v >= 1099511627776.0 ? DYN_MAX : (int64_t)v;
}

// step 7
MSG_HD float dyn_gain(int64_t e, double makeup) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (float)dyn_exp2((makeup - (double)e * (1.0 / 4294967296.0)) * 0.16609640474436813);
}
MSG_HD bool dyn_is_one(float g) { return dyn_abs_bits(g) == 0x3f800000u; }   // g > 0 always

// ---- the max-plus algebra -------------------------------------------------------------
MSG_HD int64_t dyn_max(int64_t a, int64_t b) { return a > b ? a : b; }
MSG_HD int64_t dyn_dec(int64_t y, int64_t step) { return y > step ? y - step : 0; }
// min(count step, 2^40) for count >= 0: a product below 2^53 is exact in float64 and a larger
// one rounds to far more than 2^40
MSG_HD int64_t dyn_span(int64_t count, int64_t step) {
    return (double)count * (double)step >= 1099511627776.0 ? DYN_MAX : count * step;
}
// one frame of either recurrence
MSG_HD int64_t dyn_step(int64_t y, int64_t step, int64_t d) { return dyn_max(dyn_dec(y, step), d); }
// c through a run
MSG_HD int64_t dyn_carry(const DynSeg& s, int64_t c) { return dyn_max(dyn_dec(c, s.R), s.C); }
// the run `first` followed by the run `then`; {0, 0} is the empty run
MSG_HD DynSeg dyn_join(const DynSeg& first, const DynSeg& then) {
    const int64_t r = first.R + then.R;
    return DynSeg{r > DYN_MAX ? DYN_MAX : r, dyn_max(dyn_dec(first.C, then.R), then.C)};
}
// a run of cl frames with demands v[0 .. cl), walked from its first frame (the release) or from
// its last (the attack)
MSG_HD DynSeg dyn_run(const int64_t* v, int cl, int64_t step, bool backward) {
    DynSeg s{dyn_span(cl, step), 0};
    for (int k = 0; k < cl; ++k) s.C = dyn_step(s.C, step, v[backward ? cl - 1 - k : k]);
    return s;
}

inline int64_t dyn_tiles(int64_t n) { return (n + DYN_TILE - 1) / DYN_TILE; }
// LDS int64 words of a tile workgroup: chunk rows of DYN_C + 1 words over the halo and the tile
MSG_HD int dyn_pos(int j) { return j + (j >> 4); }
inline size_t dyn_lds_bytes(int hold) { return (size_t)(dyn_pos(hold + DYN_TILE) + 1) * 8; }

// p0 of step 2: the float32 at or just under 10^((threshold - knee / 2) / 20)
inline float dyn_p0(double threshold_db, double knee_db) {
    const double lin = std::pow(10.0, (threshold_db - 0.5 * knee_db) / 20.0);
    float p = (float)lin;
    if ((double)p > lin) p = std::nextafterf(p, 0.0f);
    return p;
}
// nullptr, or why the options are refused (hold_frames > DYN_HOLD_MAX is the caller's, another status)
inline const char* dyn_refused(const DynOpts& o) {
    if (o.flags != 0) return "flags must be 0";
    if (!std::isfinite(o.threshold_db) || o.threshold_db < -150.0 || o.threshold_db > 24.0)
        return "the threshold must be a finite number of dB from -150 to 24";
    if (!(o.ratio >= 1.0)) return "the ratio must be at least 1";
    if (!std::isfinite(o.knee_db) || o.knee_db < 0.0 || o.knee_db > 48.0)
        return "the knee must be a finite number of dB from 0 to 48";
    if (!std::isfinite(o.makeup_db) || std::fabs(o.makeup_db) > 48.0)
        return "the makeup gain must be a finite number of dB from -48 to 48";
    if (o.attack_step < 1 || o.attack_step > DYN_MAX || o.release_step < 1 || o.release_step > DYN_MAX)
        return "the attack and release steps must lie in 1 .. 2^40";
    if (o.hold_frames < 0) return "the hold must be a frame count from 0 up";
    return nullptr;
}
inline DynPar dyn_par(const DynOpts& o) {
    return DynPar{o.threshold_db, o.knee_db, 1.0 - 1.0 / o.ratio, o.makeup_db, o.attack_step, o.release_step,
                  dyn_p0(o.threshold_db, o.knee_db), o.hold_frames};
}

MSG_HD uint32_t dyn_level(const float* frame, int channels) {
    uint32_t p = dyn_abs_bits(frame[0]);
    if (channels == 2) {
        const uint32_t q = dyn_abs_bits(frame[1]);
        p = q > p ? q : p;
    }
    return p;
}
// the record of a finite signal from its folded integers
MSG_HD void dyn_finish(int64_t max_e, int64_t sum_e16, int64_t reduced, bool frames, const DynPar& par, DynRec* rec) {
    rec->max_e = max_e;
    rec->sum_e16 = sum_e16;
    rec->reduced_frames = reduced;
    rec->state = (reduced > 0 || (frames && par.makeup != 0.0)) ? 1 : 0;
    rec->hold_frames = par.hold;
}

// ---- the host reference: the definition as one sequential loop, x compressed in place ----
// env: null, or n words that get E (also for a non-finite signal, whose samples stay)
inline void dyn_host(float* x, int channels, int64_t n, const DynPar& par, DynRec* rec, int64_t* env = nullptr) {
    dyn_finish(0, 0, 0, false, par, rec);
    if (n <= 0) return;
    std::vector<int64_t> d((size_t)n), e((size_t)n);
    bool bad = false;
    for (int64_t f = 0; f < n; ++f) {
        const uint32_t p = dyn_level(x + f * channels, channels);
        bad = bad || p >= DYN_INF;
        d[(size_t)f] = dyn_demand(p, par);
    }
    // hold and release: the window's maximum from a queue of frames with falling demands
    std::vector<int64_t> q((size_t)par.hold + 2);
    size_t head = 0, count = 0;
    const size_t cap = q.size();
    int64_t y = 0;
    for (int64_t f = 0; f < n; ++f) {
        while (count && d[(size_t)q[(head + count - 1) % cap]] <= d[(size_t)f]) --count;
        q[(head + count) % cap] = f;
        ++count;
        if (q[head] < f - par.hold) {
            head = (head + 1) % cap;
            --count;
        }
        y = dyn_step(y, par.rstep, d[(size_t)q[head]]);
        e[(size_t)f] = y;
    }
    y = 0;
    for (int64_t f = n - 1; f >= 0; --f) {
        y = dyn_step(y, par.astep, d[(size_t)f]);
        e[(size_t)f] = dyn_max(e[(size_t)f], y);
    }
    if (env) std::memcpy(env, e.data(), (size_t)n * 8);
    if (bad) {
        rec->state = 2;
        return;
    }
    int64_t max_e = 0, sum = 0, reduced = 0;
    for (int64_t f = 0; f < n; ++f) {
        const int64_t v = e[(size_t)f];
        max_e = dyn_max(max_e, v);
        sum += v >> 16;
        reduced += v > 0 ? 1 : 0;
        const float g = dyn_gain(v, par.makeup);
        if (dyn_is_one(g)) continue;
        for (int c = 0; c < channels; ++c) x[f * channels + c] = x[f * channels + c] * g;
    }
    dyn_finish(max_e, sum, reduced, true, par, rec);
}
