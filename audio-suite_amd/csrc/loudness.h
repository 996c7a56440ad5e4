// loudness.h — ITU-R BS.1770-4 integrated loudness (msg_loudness / msg_loudness_host):
// the definition, shared by the device kernels (kernels_loudness.h), the host
// planning in msgpu.hip and the host reference below (built into libmsgpu and
// into the host sanitizer build).  Plain C++.
//
// K-weighting: two biquads in series, designed in float64 for any rate with
// sr % 10 == 0 from the analogue prototype by the bilinear transform, so that
// 48 kHz gives the standard's table.  K = tan(pi f0 / sr) for both stages.
//   shelf:     f0 = 1681.974450955533 Hz, G = 3.999843853973347 dB, Q = 0.7071752369554196,
//              Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2,
//              b = [Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2] / a0,
//              a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0]
//   high-pass: f0 = 38.13547087602444 Hz, Q = 0.5003270373238773, d = 1 + K/Q + K^2,
//              b = [1, -2, 1] (not normalised, as in the standard),
//              a = [1, 2 (K^2 - 1) / d, (1 - K/Q + K^2) / d]
// Blocks: hop = sr / 10; block j is frames [j hop, j hop + 4 hop); only complete
// blocks count (n_blocks = 0 for n < 4 hop, else (n - 4 hop) / hop + 1);
//   z_j = mean over the block of the sum over channels of the squared K-weighted
//         sample (channel weights 1, mono and stereo),  l_j = -0.691 + 10 log10 z_j.
// Gates: keep l_j > -70; G = -0.691 + 10 log10(mean z of those) - 10; keep also
// l_j > G; lufs = -0.691 + 10 log10(mean z of those) (mean_sq is that mean).  No
// block kept: lufs = -inf, mean_sq = 0.
// The filter recurrences, every block sum and the gating run in float64 on
// float32 inputs: at 384 kHz the high-pass poles sit 6e-4 from the unit circle
// and a float32 direct form misses the standard's 0.1 LU window.
//
// Each biquad runs in transposed direct form II, so one channel carries four
// state words s = (z1, z2 of the shelf, z1, z2 of the high-pass).  The filter is
// linear: the state after L frames is A^L s + (the state the same frames leave
// from zero state), A the 4 x 4 zero-input step.  The device cuts every hop into
// tiles of LD_TILE frames (a shorter last one: tiles never straddle a hop) and a
// tile into LD_T lane chunks of LD_C frames; DESIGN.md "Loudness" has the scan.
#pragma once
#include <stdint.h>
#include <cmath>
#include <limits>
#include <vector>
#include "msg_common.h"

constexpr int LD_T = 256;                 // threads per tile workgroup (4 waves)
constexpr int LD_C = 16;                  // frames per lane chunk
constexpr int LD_TILE = LD_T * LD_C;      // 4096 frames
constexpr int LD_ROW = LD_C + 1;          // LDS frames per staged chunk: one frame of padding
constexpr int LD_GT = 64;                 // threads of the gating workgroup (one wave)
constexpr int LD_GAIN_PER = 16;           // k_loud_gain: frames per thread
constexpr int LD_GAIN_TILE = LD_T * LD_GAIN_PER;
constexpr int64_t LD_SR_MIN = 4000;       // the shelf's 1682 Hz must lie below Nyquist

// the table uploaded with a call (doubles): coefficients, then 4 x 4 row-major powers of A
constexpr int LD_TAB_COEF = 0;            // b0 b1 b2 a1 a2 of the shelf, then of the high-pass
constexpr int LD_TAB_LVL = 16;            // A^(LD_C 2^k), k = 0..5: the in-wave scan
constexpr int LD_TAB_WAVE = LD_TAB_LVL + 6 * 16;     // A^(64 LD_C): from wave to wave
constexpr int LD_TAB_AT = LD_TAB_WAVE + 16;          // A^LD_TILE: a full tile
constexpr int LD_TAB_AR = LD_TAB_AT + 16;            // A^(hop mod LD_TILE): a hop's last tile
constexpr int LD_TAB_LANE = LD_TAB_AR + 16;          // A^(LD_C l), l = 0..64
constexpr int LD_TAB_N = LD_TAB_LANE + 65 * 16;

struct LoudRec {                          // layout of msg_loudness_rec
    double lufs, mean_sq, peak, gain;
    int32_t n_blocks, n_kept;
};

// one frame of one channel through the cascade; c: the ten coefficients, z: the state
MSG_HD double ld_step(const double* c, double* z, double x) {
    const double y1 = c[0] * x + z[0];
    z[0] = c[1] * x - c[3] * y1 + z[1];
    z[1] = c[2] * x - c[4] * y1;
    const double y2 = c[5] * y1 + z[2];
    z[2] = c[6] * y1 - c[8] * y2 + z[3];
    z[3] = c[7] * y1 - c[9] * y2;
    return y2;
}

MSG_HD double ld_level(double z) { return -0.691 + 10.0 * log10(z); }

inline bool ld_rate_ok(int64_t sr) { return sr >= LD_SR_MIN && sr % 10 == 0; }

inline void ld_kweight(int64_t sr, double c[10]) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)sr), Vh = std::pow(10.0, G / 20.0),
                     Vb = std::pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)sr), d = 1.0 + K / Q + K * K;
        c[5] = 1.0; c[6] = -2.0; c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / d;
        c[9] = (1.0 - K / Q + K * K) / d;
    }
}

// ---- tiles of a signal -------------------------------------------------------
inline int64_t ld_tiles_per_hop(int64_t hop) { return (hop + LD_TILE - 1) / LD_TILE; }
// every hop, the incomplete last one included (it only feeds the sample peak)
inline int64_t ld_tiles(int64_t n, int64_t hop) {
    const int64_t full = n / hop, tail = n - full * hop;
    return full * ld_tiles_per_hop(hop) + (tail + LD_TILE - 1) / LD_TILE;
}
inline int64_t ld_blocks(int64_t n, int64_t hop) { return n < 4 * hop ? 0 : (n - 4 * hop) / hop + 1; }

// ---- powers of the zero-input step (host) ----------------------------------------
// Formed in extended precision and rounded once to float64: with the high-pass
// poles 6e-4 from the unit circle a DC offset keeps the states 1e3 and more above
// the output, and a power's error is multiplied by them.
typedef long double ld_real;
inline void ld_mat_mul(const ld_real* a, const ld_real* b, ld_real* out) {
    ld_real r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            ld_real s = 0;
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            r[4 * i + j] = s;
        }
    for (int i = 0; i < 16; ++i) out[i] = r[i];
}
inline void ld_mat_pow(const ld_real* a, int64_t L, ld_real* out) {
    ld_real base[16], acc[16];
    for (int i = 0; i < 16; ++i) { base[i] = a[i]; acc[i] = (i % 5 == 0) ? 1 : 0; }
    for (; L > 0; L >>= 1) {
        if (L & 1) ld_mat_mul(base, acc, acc);
        ld_mat_mul(base, base, base);
    }
    for (int i = 0; i < 16; ++i) out[i] = acc[i];
}
// the table of a rate: column j of A is ld_step on the j-th unit state with x = 0
inline void ld_table(int64_t sr, double* tab) {
    for (int i = 0; i < LD_TAB_N; ++i) tab[i] = 0.0;
    double* c = tab + LD_TAB_COEF;
    ld_kweight(sr, c);
    ld_real A[16], M[16];
    for (int j = 0; j < 4; ++j) {
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        z[j] = 1.0;
        ld_step(c, z, 0.0);                      // exact: each entry is a coefficient, 0 or 1
        for (int i = 0; i < 4; ++i) A[4 * i + j] = z[i];
    }
    auto put = [&](int at, int64_t L) {
        ld_mat_pow(A, L, M);
        for (int i = 0; i < 16; ++i) tab[at + i] = (double)M[i];
    };
    for (int l = 0; l <= 64; ++l) put(LD_TAB_LANE + 16 * l, (int64_t)LD_C * l);
    for (int k = 0; k < 6; ++k) put(LD_TAB_LVL + 16 * k, (int64_t)LD_C << k);
    put(LD_TAB_WAVE, 64 * LD_C);
    put(LD_TAB_AT, LD_TILE);
    put(LD_TAB_AR, (sr / 10) % LD_TILE);
}

// ---- the host reference: the definition as one sequential float64 loop ----------
// x: n frames of `channels` interleaved float32 words; hops_out: the n / hop hop sums too (lrange.h)
inline void ld_host(const float* x, int channels, int64_t n, int64_t sr, LoudRec* rec,
                    std::vector<double>* hops_out = nullptr) {
    double c[10];
    ld_kweight(sr, c);
    const int64_t hop = sr / 10, hops = n / hop, nb = ld_blocks(n, hop);
    std::vector<double> hs((size_t)hops, 0.0);
    double z[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, peak = 0.0;
    for (int64_t f = 0; f < n; ++f) {
        double e = 0.0;
        for (int ch = 0; ch < channels; ++ch) {
            const double v = (double)x[f * channels + ch];
            peak = std::fabs(v) > peak ? std::fabs(v) : peak;
            if (f < hops * hop) {
                const double y = ld_step(c, z[ch], v);
                e += y * y;
            }
        }
        if (f < hops * hop) hs[(size_t)(f / hop)] += e;
    }
    std::vector<double> zb((size_t)nb);
    for (int64_t j = 0; j < nb; ++j)
        zb[(size_t)j] = (((hs[(size_t)j] + hs[(size_t)j + 1]) + hs[(size_t)j + 2]) + hs[(size_t)j + 3]) / (4.0 * (double)hop);
    const double ninf = -std::numeric_limits<double>::infinity();
    double s1 = 0.0, s2 = 0.0;
    int64_t c1 = 0, c2 = 0;
    for (int64_t j = 0; j < nb; ++j)
        if (ld_level(zb[(size_t)j]) > -70.0) { s1 += zb[(size_t)j]; ++c1; }
    const double gate = c1 ? ld_level(s1 / (double)c1) - 10.0 : 0.0;
    for (int64_t j = 0; j < nb && c1; ++j) {
        const double l = ld_level(zb[(size_t)j]);
        if (l > -70.0 && l > gate) { s2 += zb[(size_t)j]; ++c2; }
    }
    rec->mean_sq = c2 ? s2 / (double)c2 : 0.0;
    rec->lufs = c2 ? ld_level(rec->mean_sq) : ninf;
    rec->peak = peak;
    rec->gain = 0.0;
    rec->n_blocks = (int32_t)nb;
    rec->n_kept = (int32_t)c2;
    if (hops_out) hops_out->swap(hs);
}
