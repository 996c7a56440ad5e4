// lrange.h — EBU R 128 delivery meters on top of loudness.h (msg_loudness_range /
// msg_loudness_range_host / msg_lrange_hops_host): the loudness range (EBU Tech 3342)
// and the maximum momentary and short-term loudness (EBU Tech 3341).  The definition,
// shared by the device kernels (kernels_lrange.h) and the host reference below (built
// into libmsgpu and into the host sanitizer build).  Plain C++.
//
// Everything is formed from the K-weighted hop sums of loudness.h: hop = sr / 10,
// hops = n / hop, H_k the sum over hop k of the squared K-weighted samples of every
// channel (on the device: the hop's tiles added in order), level(z) = ld_level(z).
// Rates as for msg_loudness (ld_rate_ok).
//
// Momentary (400 ms): nb = hops < 4 ? 0 : hops - 3 blocks, msg_loudness's own,
//   z_j = (((H_j + H_j+1) + H_j+2) + H_j+3) / (4 hop);
//   z_max_m = max_j z_j (ungated), max_momentary = level(z_max_m); nb = 0: 0 and -inf.
// Short-term (3 s): ns = hops < 30 ? 0 : hops - 29 windows, one per 100 ms,
//   W_i = H_i + H_i+1 + ... + H_i+29, a left fold in ascending order from H_i,
//   zs_i = W_i / (30 hop), S_i = level(zs_i);
//   z_max_s = max_i zs_i, max_short = level(z_max_s); ns = 0: 0 and -inf.
// Loudness range: keep S_i > -70 (count n_abs); gate = level(mean zs of those) - 20,
//   -inf when none; keep also S_i > gate (count n_kept = c2).  Of the kept windows in
//   ascending order of zs, z_lo is element ((c2 - 1) 10 + 50) / 100 and z_hi element
//   ((c2 - 1) 95 + 50) / 100 (integer division: the nearest rank of the 10th and 95th
//   percentile); lo = level(z_lo), hi = level(z_hi), lra = hi - lo.  c2 = 0: lra = 0,
//   lo = hi = -inf, z_lo = z_hi = 0.
// The mean of the relative gate is folded as k_loud_gate folds its sums: lane i of LR_T
// takes windows i, i + LR_T, ... in order, an xor-butterfly joins the 64 lanes of each
// wave, and the waves are added in order.  The maxima and the order statistics do not
// depend on any order, so a record depends on its own hop sums only.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <limits>
#include <vector>
#include "loudness.h"

constexpr int LR_T = 256;                 // threads of k_lrange (4 waves): the lanes of the gate's fold
constexpr int LR_M = 4;                   // hops of a momentary block
constexpr int LR_S = 30;                  // hops of a short-term window
constexpr double LR_ABS = -70.0;          // absolute gate, LUFS
constexpr double LR_REL = 20.0;           // relative gate, LU under the mean
constexpr uint64_t LR_DROPPED = ~0ull;    // the pattern a window outside the gates sorts as: above every kept one

struct LRangeRec {                        // layout of msg_lrange_rec
    double lra, lo, hi, max_momentary, max_short, gate, z_lo, z_hi, z_max_m, z_max_s;
    int32_t n_momentary, n_short, n_abs, n_kept;
};

MSG_HD int64_t lr_blocks(int64_t hops) { return hops < LR_M ? 0 : hops - (LR_M - 1); }
MSG_HD int64_t lr_windows(int64_t hops) { return hops < LR_S ? 0 : hops - (LR_S - 1); }
MSG_HD double lr_block_z(const double* H, int64_t j, int64_t hop) {
    return (((H[j] + H[j + 1]) + H[j + 2]) + H[j + 3]) / (4.0 * (double)hop);
}
MSG_HD double lr_window_z(const double* H, int64_t i, int64_t hop) {
    double w = H[i];
    for (int k = 1; k < LR_S; ++k) w += H[i + k];
    return w / ((double)LR_S * (double)hop);
}
// the ranks of the two percentiles among c2 kept windows
MSG_HD int64_t lr_rank_lo(int64_t c2) { return ((c2 - 1) * 10 + 50) / 100; }
MSG_HD int64_t lr_rank_hi(int64_t c2) { return ((c2 - 1) * 95 + 50) / 100; }

// the record from the maxima, the gate's count and the two selected values
MSG_HD void lr_finish(LRangeRec* r, double zm, double zs, double gate, double z_lo, double z_hi, int64_t nb, int64_t ns,
                      int64_t c1, int64_t c2) {
    const double ninf = -__builtin_inf();
    r->z_max_m = zm;
    r->z_max_s = zs;
    r->max_momentary = nb ? ld_level(zm) : ninf;
    r->max_short = ns ? ld_level(zs) : ninf;
    r->gate = gate;
    r->z_lo = c2 ? z_lo : 0.0;
    r->z_hi = c2 ? z_hi : 0.0;
    r->lo = c2 ? ld_level(z_lo) : ninf;
    r->hi = c2 ? ld_level(z_hi) : ninf;
    r->lra = c2 ? r->hi - r->lo : 0.0;
    r->n_momentary = (int32_t)nb;
    r->n_short = (int32_t)ns;
    r->n_abs = (int32_t)c1;
    r->n_kept = (int32_t)c2;
}

// ---- the host reference: the definition from given hop sums ---------------------------
inline void lr_hops_host(const double* H, int64_t hops, int64_t hop, LRangeRec* rec) {
    const int64_t nb = lr_blocks(hops), ns = lr_windows(hops);
    double zm = 0.0, zsm = 0.0;
    for (int64_t j = 0; j < nb; ++j) {
        const double z = lr_block_z(H, j, hop);
        zm = z > zm ? z : zm;
    }
    std::vector<double> zs((size_t)ns);
    double lane[LR_T];
    int64_t c1 = 0, c2 = 0;
    for (int l = 0; l < LR_T; ++l) lane[l] = 0.0;
    for (int64_t i = 0; i < ns; ++i) {
        const double z = zs[(size_t)i] = lr_window_z(H, i, hop);
        zsm = z > zsm ? z : zsm;
        if (ld_level(z) > LR_ABS) { lane[i % LR_T] += z; ++c1; }     // lane l: its windows in ascending order
    }
    for (int w = 0; w < LR_T; w += 64)
        for (int o = 32; o >= 1; o >>= 1)
            for (int l = 0; l < o; ++l) lane[w + l] += lane[w + l + o];
    double s1 = lane[0];
    for (int w = 64; w < LR_T; w += 64) s1 += lane[w];
    const double gate = c1 ? ld_level(s1 / (double)c1) - LR_REL : -std::numeric_limits<double>::infinity();
    std::vector<double> kept;
    kept.reserve((size_t)c1);
    for (int64_t i = 0; i < ns && c1; ++i) {
        const double l = ld_level(zs[(size_t)i]);
        if (l > LR_ABS && l > gate) kept.push_back(zs[(size_t)i]);
    }
    c2 = (int64_t)kept.size();
    double z_lo = 0.0, z_hi = 0.0;
    if (c2) {
        std::sort(kept.begin(), kept.end());
        z_lo = kept[(size_t)lr_rank_lo(c2)];
        z_hi = kept[(size_t)lr_rank_hi(c2)];
    }
    lr_finish(rec, zm, zsm, gate, z_lo, z_hi, nb, ns, c1, c2);
}

// one signal in host memory: ld_host's loop (its record into loud when given), then the hop sums' record
inline void lr_host(const float* x, int channels, int64_t n, int64_t sr, LoudRec* loud, LRangeRec* rec) {
    std::vector<double> hs;
    LoudRec l;
    ld_host(x, channels, n, sr, &l, &hs);
    if (loud) *loud = l;
    lr_hops_host(hs.data(), (int64_t)hs.size(), sr / 10, rec);
}
