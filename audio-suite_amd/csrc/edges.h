// edges.h — silence trim, fades and loop crossfade (msg_edges / msg_edges_host): the
// definition, shared by the device kernels (kernels_edges.h), the host planning in
// signal_abi.inc and the host reference below (built into libmsgpu and into the host
// sanitizer build).  Plain C++.  DESIGN.md "4i. Edges".
//
// Inputs: one signal x of n frames, CH in {1, 2} interleaved float32 channels, and the
// options in frames (the caller turns milliseconds into frames: llround(ms sr / 1000)).
//
// 1. Level.  m[f] = max over the channels of |x[f, c]|.  A frame is sound when m[f] >= thr,
//    thr = (float)10^(trim_db / 20), formed once on the host in float64 (edg_threshold).  A NaN
//    compares false and is silence, an infinity is sound; the comparison is made per channel,
//    so a frame with a NaN in one channel is sound when the other channel reaches thr.
// 2. Span.  first / last: the lowest and highest sound frames.  sides: EDG_HEAD | EDG_TAIL,
//    the ends that are trimmed; 0: no trim, nothing is searched and first = 0, last = n - 1.
//      start = head trimmed ? max(0, first - pre) : 0
//      end   = tail trimmed ? min(n, last + 1 + post) : n
//    Without a sound frame first = last = -1, the record carries EDG_SILENT and the span is
//    the whole signal.  n = 0: every field is 0.
// 3. Fades over len = end - start frames with Fi and Fo frames asked for.  Fi + Fo > len:
//    Fi' = floor(len Fi / (Fi + Fo)) in int64, Fo' = len - Fi'.  Frame k of the fade-in has
//    g = (float)c((2 k + 1) / (2 Fi')), frame k of the fade-out, counted from its first frame,
//    g = (float)c((2 (Fo' - k) - 1) / (2 Fo')); the argument is one float64 division of two
//    exact integers.  y = (float)((double)x (double)g): the product of two float32 values is
//    exact in float64, so there is one rounding and contraction cannot change it.  The other
//    frames of the span keep their bits, frames outside it are not touched, nothing moves.
// 4. Loop crossfade of X frames, instead of fades.  X' = min(X, len / 2).  For k < X',
//    t = (2 k + 1) / (2 X'):
//      y[start + k] = (float)((double)x[start + k] c(t) + (double)x[end - X' + k] c(1 - t))
//    with both gains rounded to float32 first: two exact products, one float64 add, one
//    rounding.  The source frames [end - X', end) and the written frames [start, start + X')
//    are disjoint because X' <= len / 2.  The delivered span ends at end - X': the record's
//    `end` holds that value.
// 5. Curves c: EDG_LINEAR t, EDG_HANN 1/2 - 1/2 cos(pi t) = sin^2(pi t / 2), EDG_QSIN
//    sin(pi t / 2).  edg_curve below is the one routine of both sides: float64 multiplies and
//    adds in one written order with contraction off, no libm and no ocml call, so the host
//    and the device agree to the bit.  sin(pi t / 2) is the Taylor polynomial of sin to x^15
//    on t <= 1/2 and of cos to x^16 at (1 - t) pi / 2 above (1 - t is exact there), |x| <=
//    pi / 4: the truncation is below 5e-17 and the 20 roundings of a Horner chain stay below
//    3e-15, squared for the Hann curve below 6e-15.  Against the float64 definition the
//    float32 gain therefore differs by at most one rounding to float32 of a value in [0, 1],
//    2^-25, plus 6e-15 (which can move that rounding to the neighbouring float only where the
//    definition lies within 6e-15 of a tie, still within 2^-25 + 6e-15): under 2^-24.
//
// Record (msg_edges_rec): first, last, start, end (after the loop), fade_in, fade_out and
// loop as applied (Fi', Fo', X'), flags.
//
// The device: k_edges_find over tiles of EDG_TILE frames, k_edges_span one lane per signal,
// k_edges_apply over tiles of EDG_APPLY_TILE frames of the fade or crossfade regions only.
#pragma once
#include <stdint.h>
#include <cmath>
#include "msg_common.h"

constexpr int EDG_T = 256;                      // threads of k_edges_find and k_edges_apply
constexpr int EDG_TILE = 4096;                  // frames per find tile
constexpr int EDG_APPLY_TILE = 1024;            // frames per apply tile
constexpr int EDG_HEAD = 1, EDG_TAIL = 2;       // sides
constexpr int EDG_LINEAR = 0, EDG_HANN = 1, EDG_QSIN = 2;
constexpr int64_t EDG_SILENT = 1;               // flags
constexpr int64_t EDG_NO_FIRST = INT64_MAX;     // `first` before any tile has reported
constexpr int64_t EDG_MAX_FRAMES = ((int64_t)1 << 31) - ((int64_t)1 << 20);   // the longest signal of any pass

struct EdgesRec {                               // layout of msg_edges_rec
    int64_t first, last, start, end, fade_in, fade_out, loop, flags;
};
struct EdgesOpts {                              // layout of msg_edges_opts
    double trim_db;
    int32_t sides, curve;
    int64_t pre, post, fade_in, fade_out, loop; // loop < 0: no crossfade
};
// what the kernels take by value
struct EdgesPar {
    float thr;
    int32_t sides, curve;
    int64_t pre, post, fade_in, fade_out, loop;
};

inline float edg_threshold(double trim_db) { return (float)std::pow(10.0, trim_db / 20.0); }
inline EdgesPar edg_par(const EdgesOpts& o) {
    return EdgesPar{o.sides ? edg_threshold(o.trim_db) : 0.0f, o.sides, o.curve, o.pre, o.post, o.fade_in, o.fade_out,
                    o.loop < 0 ? -1 : o.loop};
}

MSG_HD int64_t edg_min(int64_t a, int64_t b) { return a < b ? a : b; }
MSG_HD int64_t edg_max(int64_t a, int64_t b) { return a > b ? a : b; }
MSG_HD int64_t edg_tiles(int64_t n) { return (n + EDG_TILE - 1) / EDG_TILE; }
MSG_HD int64_t edg_apply_tiles_of(int64_t frames) { return (frames + EDG_APPLY_TILE - 1) / EDG_APPLY_TILE; }
// apply tiles of a signal of n frames: bounds of Fi', Fo' and X' that need no measurement
// (Fi' <= min(Fi, n), Fo' <= min(Fo, n), X' <= min(X, n / 2)); the fade-in's tiles come first
MSG_HD int64_t edg_in_tiles(const EdgesPar& p, int64_t n) {
    return edg_apply_tiles_of(p.loop >= 0 ? edg_min(p.loop, n / 2) : edg_min(p.fade_in, n));
}
MSG_HD int64_t edg_apply_tiles(const EdgesPar& p, int64_t n) {
    return edg_in_tiles(p, n) + (p.loop >= 0 ? 0 : edg_apply_tiles_of(edg_min(p.fade_out, n)));
}

// sin(pi t / 2) for 0 <= t <= 1 (step 5)
MSG_HD double edg_qsin(double t) {
#if defined(__clang__)                          // g++ for x86-64 has no fused instruction to contract into
#pragma clang fp contract(off)
#endif
    const double h = 1.5707963267948966;
    if (t <= 0.5) {
        const double x = t * h, z = x * x;
        double p = -1.0 / 1307674368000.0;
        p = p * z + 1.0 / 6227020800.0;
        p = p * z - 1.0 / 39916800.0;
        p = p * z + 1.0 / 362880.0;
        p = p * z - 1.0 / 5040.0;
        p = p * z + 1.0 / 120.0;
        p = p * z - 1.0 / 6.0;
        p = p * z + 1.0;
        return x * p;
    }
    const double x = (1.0 - t) * h, z = x * x;
    double p = 1.0 / 20922789888000.0;
    p = p * z - 1.0 / 87178291200.0;
    p = p * z + 1.0 / 479001600.0;
    p = p * z - 1.0 / 3628800.0;
    p = p * z + 1.0 / 40320.0;
    p = p * z - 1.0 / 720.0;
    p = p * z + 1.0 / 24.0;
    p = p * z - 0.5;
    p = p * z + 1.0;
    return p;
}

MSG_HD double edg_curve(int curve, double t) {
    if (curve == EDG_LINEAR) return t;
    const double s = edg_qsin(t);
    return curve == EDG_HANN ? s * s : s;
}

// the gain at t = num / (2 F): num = 2 k + 1 fading in, 2 (F - k) - 1 fading out
MSG_HD float edg_gain(int curve, int64_t num, int64_t F) {
    return (float)edg_curve(curve, (double)num / (double)(2 * F));
}
MSG_HD float edg_fade(float x, float g) { return (float)((double)x * (double)g); }
// step 4 for frame k of X: a is the span's frame start + k, b the frame end - X + k
MSG_HD void edg_loop_gains(int curve, int64_t k, int64_t X, float* ga, float* gb) {
    const double t = (double)(2 * k + 1) / (double)(2 * X);
    *ga = (float)edg_curve(curve, t);
    *gb = (float)edg_curve(curve, 1.0 - t);
}
MSG_HD float edg_mix(float a, float ga, float b, float gb) {
    return (float)((double)a * (double)ga + (double)b * (double)gb);
}

// steps 2 to 4 for a signal of n frames whose sound frames run from first to last (last < 0: none)
MSG_HD EdgesRec edg_span(int64_t n, int64_t first, int64_t last, const EdgesPar& p) {
    EdgesRec r{0, 0, 0, 0, 0, 0, 0, 0};
    if (n <= 0) return r;
    r.end = n;
    if (!p.sides) {
        r.last = n - 1;
    } else if (last < 0) {
        r.first = r.last = -1;
        r.flags |= EDG_SILENT;
    } else {
        r.first = first;
        r.last = last;
        if (p.sides & EDG_HEAD) r.start = edg_max(0, first - p.pre);
        if (p.sides & EDG_TAIL) r.end = edg_min(n, last + 1 + p.post);
    }
    const int64_t len = r.end - r.start;
    if (p.loop >= 0) {
        r.loop = edg_min(p.loop, len / 2);
        r.end -= r.loop;
        return r;
    }
    r.fade_in = p.fade_in;
    r.fade_out = p.fade_out;
    if (p.fade_in + p.fade_out > len) {
        r.fade_in = len * p.fade_in / (p.fade_in + p.fade_out);
        r.fade_out = len - r.fade_in;
    }
    return r;
}

// ---- the host reference: the definition as one loop, x shaped in place ------------------
inline void edg_host(float* x, int channels, int64_t n, const EdgesPar& p, EdgesRec* rec) {
    int64_t first = EDG_NO_FIRST, last = -1;
    if (p.sides)
        for (int64_t f = 0; f < n; ++f) {
            bool sound = false;
            for (int c = 0; c < channels; ++c) sound = sound || std::fabs(x[f * channels + c]) >= p.thr;
            if (sound) {
                if (last < 0) first = f;
                last = f;
            }
        }
    const EdgesRec r = edg_span(n, first, last, p);
    *rec = r;
    for (int64_t k = 0; k < r.loop; ++k) {
        float ga, gb;
        edg_loop_gains(p.curve, k, r.loop, &ga, &gb);
        for (int c = 0; c < channels; ++c)
            x[(r.start + k) * channels + c] = edg_mix(x[(r.start + k) * channels + c], ga, x[(r.end + k) * channels + c], gb);
    }
    for (int64_t k = 0; k < r.fade_in; ++k) {
        const float g = edg_gain(p.curve, 2 * k + 1, r.fade_in);
        for (int c = 0; c < channels; ++c) x[(r.start + k) * channels + c] = edg_fade(x[(r.start + k) * channels + c], g);
    }
    for (int64_t k = 0; k < r.fade_out; ++k) {
        const float g = edg_gain(p.curve, 2 * (r.fade_out - k) - 1, r.fade_out);
        const int64_t f = r.end - r.fade_out + k;
        for (int c = 0; c < channels; ++c) x[f * channels + c] = edg_fade(x[f * channels + c], g);
    }
}
