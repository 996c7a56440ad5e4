// resample.h — shapes of the polyphase resampler (msg_resample): which kernel a
// ratio runs on, its output tile, the tap-table layout and the LDS it stages.
// Plain C++ (host planning and the kernels' launch shapes share it).
//
//   y[k] = up * sum_m h[k down + half - m up] x[m],  half = (K - 1) / 2
//
// Decimation kernel (up == 1, down in {2, 4, 8}): a tile's input span is staged
// transposed, X[channel][j mod down][j / down] for local frame j, so output i
// is the sum over rows r of a stride-1 FIR
//   y[i] = sum_r sum_a trow[r][a] X[r][i + a],  trow[r][a] = h[K - 1 - (a down + r)]
// with wave-uniform taps; a lane owns RS_RB consecutive outputs and slides a
// window of 16-byte LDS reads along its row (conflict-free: lane stride 4 dwords).
//
// General kernel: taps phase-major, tab[p][q] = up h[p + q up] in rows of Q4
// floats (16-byte rows, zero-padded); output k has phase p = (k down + half) mod
// up and newest input m0 = (k down + half) / up.  Lane l of L = up G lanes owns
// outputs k0 + l + r L (r < RS_RB): they share the phase, so one 16-byte tap
// read serves RS_RB outputs of every channel; their inputs lie step = G down
// frames apart in the staged span.
#pragma once
#include <cstdint>
#include "msg_common.h"

constexpr int RS_RB = 4;              // outputs per lane
constexpr int RS_DTILE = 512;         // decimation kernel: output frames per workgroup
constexpr int RS_LANES = 256;         // general kernel: threads, and lanes when up <= 256
constexpr int RS_LDS_BYTES = 65536;   // staged span limit of either kernel
constexpr int64_t RS_TAB_MAX = (int64_t)1 << 20;   // tap-table floats (4 MiB: one XCD's L2)
constexpr int32_t RS_RATIO_MAX = 1 << 16;          // up, down

struct RsPlan {
    int kind;        // 0 decimation kernel, 1 general kernel, -1 unsupported
    int tile;        // output frames per workgroup
    int taps;        // decimation: taps per row A (multiple of 8); general: row stride Q4
    int row;         // decimation: LDS row stride in floats (an odd multiple of 4)
    int lanes;       // general: L
    int step;        // general: input frames between a lane's outputs
    int span;        // staged input frames
    int64_t tab;     // tap-table floats
    int lds_bytes;
};

inline RsPlan rs_plan(int32_t up, int32_t down, int64_t K, int channels) {
    RsPlan p{};
    p.kind = -1;
    if (up == 1 && (down == 2 || down == 4 || down == 8)) {
        const int64_t A = ((K - 1) / down + 1 + 7) & ~(int64_t)7;
        int64_t row = RS_DTILE + A;
        if (((row >> 2) & 1) == 0) row += 4;
        const int64_t bytes = (int64_t)channels * down * row * 4;
        if (bytes <= RS_LDS_BYTES) {
            p.kind = 0; p.tile = RS_DTILE; p.taps = (int)A; p.row = (int)row;
            p.span = (int)((RS_DTILE + A) * down); p.tab = A * down; p.lds_bytes = (int)bytes;
            return p;
        }
    }
    const int64_t Q4 = ((K + up - 1) / up + 3) & ~(int64_t)3;
    const int64_t tab = (int64_t)up * Q4;
    // G phase periods per tile: RS_LANES lanes when up allows, halved until the span fits
    int64_t G = up >= RS_LANES ? 1 : RS_LANES / up, L, step, span, bytes;
    for (;; G /= 2) {
        L = G * up; step = G * down;
        span = Q4 + ((L - 1) * down) / up + 2 + (RS_RB - 1) * step;
        bytes = (span * channels + 8) * 4;
        if (bytes <= RS_LDS_BYTES || G == 1) break;
    }
    if (bytes > RS_LDS_BYTES || tab > RS_TAB_MAX) return p;
    p.kind = 1; p.tile = (int)(RS_RB * L); p.taps = (int)Q4; p.lanes = (int)L; p.step = (int)step;
    p.span = (int)span; p.tab = tab; p.lds_bytes = (int)bytes;
    return p;
}

// the tap table of a plan, gain `up` folded in (float64 product, rounded once)
inline void rs_table(const RsPlan& p, int32_t up, int32_t down, const double* h, int64_t K, float* tab) {
    if (p.kind == 0) {
        for (int r = 0; r < down; ++r)
            for (int a = 0; a < p.taps; ++a) {
                const int64_t u = (int64_t)a * down + r;
                tab[(int64_t)r * p.taps + a] = u <= K - 1 ? (float)(up * h[K - 1 - u]) : 0.0f;
            }
    } else {
        for (int ph = 0; ph < up; ++ph)
            for (int q = 0; q < p.taps; ++q) {
                const int64_t t = ph + (int64_t)q * up;
                tab[(int64_t)ph * p.taps + q] = t < K ? (float)(up * h[t]) : 0.0f;
            }
    }
}

MSG_HD int64_t rs_out_len(int64_t n, int32_t up, int32_t down) { return (n * up + down - 1) / down; }
