// filter.h — the delivery filter (msg_filter / msg_filter_host): the definition, shared by
// the device kernels (kernels_filter.h), the entry point in signal_abi.inc and the host
// reference below (built into libmsgpu and into the host sanitizer build).  Plain C++.
//
// A cascade is 1 .. FL_MAX_SECTIONS second-order sections in scipy's row layout
// b0 b1 b2 a0 a1 a2, float64, with a0 == 1.  Each section runs in transposed direct form II
// with two float64 state words per channel,
//   y  = b0 x + z0
//   z0 = (b1 x - a1 y) + z1
//   z1 = b2 x - a2 y
// every product and sum rounded by itself (no contraction), the order scipy.signal.sosfilt
// writes them in.  Sections run in series, channels are independent, and a signal starts
// from zero state at its own first frame.  The cascade's float64 output is rounded once to
// float32 and replaces the input in place.  FL_REVERSE runs the same recurrence from the
// signal's last frame to its first (sosfilt(x[::-1])[::-1]); a forward call followed by a
// reverse call with the same cascade has no phase shift and twice every band's gain in dB.
//
// Refused (fl_values): a section count outside 1 .. 8, a coefficient that is not finite,
// a0 != 1, and a section outside the stability triangle |a2| < 1, |a1| < 1 + a2.
//
// The filter is linear: the state after L frames is A^L s + (the state the same frames
// leave from zero state), A the zero-input step.  The device cuts a signal into tiles of
// FL_TILE frames counted from its first frame (its last for FL_REVERSE) and a tile into
// FL_T lane chunks of FL_C frames, and works through a tile section by section, so every
// scan inside a tile is 2 x 2 (A_k of one section); the joint 2S x 2S matrix of the whole
// cascade appears only in the scan over tiles.  DESIGN.md "4j. Filter" has the kernels.
#pragma once
#include <stdint.h>
#include <cmath>
#include <vector>
#include "msg_common.h"

constexpr int FL_MAX_SECTIONS = 8;
constexpr int FL_REVERSE = 1;             // MSG_FILTER_REVERSE
constexpr int FL_T = 256;                 // threads per tile workgroup (4 waves)
constexpr int FL_C = 16;                  // frames per lane chunk
constexpr int FL_TILE = FL_T * FL_C;      // 4096 frames
constexpr int FL_ROW = FL_C + 1;          // LDS frames per staged chunk: one frame of padding
constexpr int FL_NS = 2 * FL_MAX_SECTIONS;   // state words of the longest cascade, per channel

struct FilterOpts {                       // layout of msg_filter_opts
    int32_t n_sections, flags;
    double sos[FL_MAX_SECTIONS][6];
};

// the table uploaded with a call (doubles)
constexpr int FL_TAB_JOINT = 0;           // A^FL_TILE of the cascade, FL_NS x FL_NS row-major, zero outside 2S x 2S
constexpr int FL_TAB_SEC = FL_NS * FL_NS; // then FL_SEC_N doubles per section:
constexpr int FL_SEC_COEF = 0;            //   b0 b1 b2 a1 a2
constexpr int FL_SEC_LVL = 8;             //   A_k^(FL_C 2^j), j = 0..5, 2 x 2 row-major: the in-wave scan
constexpr int FL_SEC_WAVE = FL_SEC_LVL + 6 * 4;      //   A_k^(64 FL_C): from wave to wave
constexpr int FL_SEC_LANE = FL_SEC_WAVE + 4;         //   A_k^(FL_C l), l = 0..64
constexpr int FL_SEC_N = FL_SEC_LANE + 65 * 4;
constexpr int FL_TAB_N = FL_TAB_SEC + FL_MAX_SECTIONS * FL_SEC_N;

// one frame of one channel through one section; c: b0 b1 b2 a1 a2, z: the two state words
template <class R>
MSG_HD R fl_step(const double* c, R* z, R x) {
#if defined(__clang__)                    // g++ for x86-64 has no fused instruction to contract into
#pragma clang fp contract(off)
#endif
    const R y = (R)c[0] * x + z[0];
    z[0] = ((R)c[1] * x - (R)c[3] * y) + z[1];
    z[1] = (R)c[2] * x - (R)c[4] * y;
    return y;
}

// nullptr, or why the options are refused
inline const char* fl_refused(const FilterOpts& o) {
    if (o.n_sections < 1 || o.n_sections > FL_MAX_SECTIONS) return "the cascade has 1 to 8 sections";
    if (o.flags & ~FL_REVERSE) return "flags must be 0 or MSG_FILTER_REVERSE";
    for (int k = 0; k < o.n_sections; ++k) {
        const double* s = o.sos[k];
        for (int i = 0; i < 6; ++i)
            if (!std::isfinite(s[i])) return "the coefficients must be finite";
        if (s[3] != 1.0) return "a0 must be 1";
        if (!(std::fabs(s[5]) < 1.0) || !(std::fabs(s[4]) < 1.0 + s[5]))
            return "every section must lie inside the stability triangle |a2| < 1, |a1| < 1 + a2";
    }
    return nullptr;
}

inline int64_t fl_tiles(int64_t n) { return (n + FL_TILE - 1) / FL_TILE; }

// ---- the host reference: the definition as one sequential float64 loop ----------------
// x: n frames of `channels` interleaved float32 words, in place
inline void fl_host(float* x, int channels, int64_t n, const FilterOpts& o) {
    double c[FL_MAX_SECTIONS][5];
    for (int k = 0; k < o.n_sections; ++k) {
        c[k][0] = o.sos[k][0]; c[k][1] = o.sos[k][1]; c[k][2] = o.sos[k][2];
        c[k][3] = o.sos[k][4]; c[k][4] = o.sos[k][5];
    }
    const bool rev = (o.flags & FL_REVERSE) != 0;
    for (int ch = 0; ch < channels; ++ch) {
        double z[FL_MAX_SECTIONS][2] = {};
        for (int64_t r = 0; r < n; ++r) {
            float* q = x + (rev ? n - 1 - r : r) * channels + ch;
            double v = (double)*q;
            for (int k = 0; k < o.n_sections; ++k) v = fl_step<double>(c[k], z[k], v);
            *q = (float)v;
        }
    }
}

// ---- powers of the zero-input steps (host) --------------------------------------------
// Formed in extended precision and rounded once to float64 (loudness.h has the reason: a
// rumble high-pass at 384 kHz has its poles 3e-4 from the unit circle, a DC offset keeps
// the states far above the output, and a power's error is multiplied by them).
typedef long double fl_real;
inline void fl_mat_mul(int n, const fl_real* a, const fl_real* b, fl_real* out) {
    fl_real r[FL_NS * FL_NS];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            fl_real s = 0;
            for (int k = 0; k < n; ++k) s += a[n * i + k] * b[n * k + j];
            r[n * i + j] = s;
        }
    for (int i = 0; i < n * n; ++i) out[i] = r[i];
}
inline void fl_mat_pow(int n, const fl_real* a, int64_t L, fl_real* out) {
    fl_real base[FL_NS * FL_NS], acc[FL_NS * FL_NS];
    for (int i = 0; i < n * n; ++i) { base[i] = a[i]; acc[i] = (i % (n + 1) == 0) ? 1 : 0; }
    for (; L > 0; L >>= 1) {
        if (L & 1) fl_mat_mul(n, base, acc, acc);
        fl_mat_mul(n, base, base, base);
    }
    for (int i = 0; i < n * n; ++i) out[i] = acc[i];
}
// the table of a cascade; column j of a zero-input step is fl_step on the j-th unit state with x = 0
inline void fl_table(const FilterOpts& o, double* tab) {
    for (int i = 0; i < FL_TAB_N; ++i) tab[i] = 0.0;
    const int S = o.n_sections, n = 2 * S;
    for (int k = 0; k < S; ++k) {
        double* sec = tab + FL_TAB_SEC + k * FL_SEC_N;
        double* c = sec + FL_SEC_COEF;
        c[0] = o.sos[k][0]; c[1] = o.sos[k][1]; c[2] = o.sos[k][2]; c[3] = o.sos[k][4]; c[4] = o.sos[k][5];
        const fl_real A[4] = {-(fl_real)c[3], 1, -(fl_real)c[4], 0};
        fl_real M[4];
        auto put = [&](int at, int64_t L) {
            fl_mat_pow(2, A, L, M);
            for (int i = 0; i < 4; ++i) sec[at + i] = (double)M[i];
        };
        for (int l = 0; l <= 64; ++l) put(FL_SEC_LANE + 4 * l, (int64_t)FL_C * l);
        for (int j = 0; j < 6; ++j) put(FL_SEC_LVL + 4 * j, (int64_t)FL_C << j);
        put(FL_SEC_WAVE, 64 * FL_C);
    }
    // the joint step: the unit states through the whole cascade, in extended precision
    // (a later section's entries are products of coefficients)
    fl_real A[FL_NS * FL_NS], M[FL_NS * FL_NS];
    for (int j = 0; j < n; ++j) {
        fl_real z[FL_NS] = {};
        z[j] = 1;
        fl_real v = 0;
        for (int k = 0; k < S; ++k) v = fl_step<fl_real>(tab + FL_TAB_SEC + k * FL_SEC_N + FL_SEC_COEF, z + 2 * k, v);
        for (int i = 0; i < n; ++i) A[n * i + j] = z[i];
    }
    fl_mat_pow(n, A, FL_TILE, M);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) tab[FL_TAB_JOINT + FL_NS * i + j] = (double)M[n * i + j];
}
