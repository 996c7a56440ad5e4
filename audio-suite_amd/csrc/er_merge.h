// er_merge.h — host: the early-reflection tap merge of one preset
// (msg_render_batch's tap-merge stage).  Taps whose rounded delays coincide are
// merged in tap order and in float64 (the order MS:416-420 adds them), and the
// taps that act on the output (0 < offset < out_n, MS:418-420) are compacted to
// the front of the preset's tap range sorted by offset: k_h_build walks only
// the taps whose shifted IR overlaps its tile.  Header-only, the standard
// library and tap_sort.h alone, so tests/er_merge_check.cpp compiles the same code.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "tap_sort.h"

// off[0, nt): each tap's rounded offset; on return off[0, live) holds the live
// slots' offsets in increasing order.  Host-gain form (g != nullptr): g[0, nt)
// holds the taps' gains, on return g[0, live) the slots' sums.  Device-gain
// form (g == nullptr): kx[0, m) receives the in-range taps' indices in sorted
// order, first / cnt[0, live) each slot's range of kx (k_er_gains draws and
// sums the gains).  *tap_max: the largest live offset, 0 without live taps.
// Returns live.
inline int er_merge_taps(int nt, int64_t out_n, int32_t* off, double* g, int32_t* kx, int32_t* first, int32_t* cnt,
                         int32_t* tap_max) {
    // (offset, tap index) packed in one key, sorted stably by offset (tap_sort.h)
    thread_local std::vector<uint64_t> keybuf, tmpbuf;
    thread_local std::vector<double> g0;
    keybuf.resize(nt);
    tmpbuf.resize(nt);
    if (g) g0.assign(g, g + nt);
    int m = 0;
    uint32_t omax = 0;
    for (int k = 0; k < nt; ++k)
        if (off[k] > 0 && off[k] < out_n) {
            keybuf[m++] = ((uint64_t)(uint32_t)off[k] << 32) | (uint32_t)k;
            omax = std::max(omax, (uint32_t)off[k]);
        }
    const uint64_t* key = sort_taps_by_offset(keybuf.data(), tmpbuf.data(), m, omax);
    int live = 0;
    if (!g) {                                    // slots -> key ranges, summed by k_er_gains
        for (int i = 0; i < m; ++i) kx[i] = (int32_t)(uint32_t)key[i];
        for (int i = 0; i < m;) {
            const uint32_t o = (uint32_t)(key[i] >> 32);
            int j = i + 1;
            while (j < m && (uint32_t)(key[j] >> 32) == o) ++j;
            off[live] = (int32_t)o;
            first[live] = i;
            cnt[live] = j - i;
            ++live;
            i = j;
        }
    } else {
        for (int i = 0; i < m;) {
            const uint32_t o = (uint32_t)(key[i] >> 32);
            double acc = g0[(uint32_t)key[i]];
            int j = i + 1;
            for (; j < m && (uint32_t)(key[j] >> 32) == o; ++j) acc += g0[(uint32_t)key[j]];
            off[live] = (int32_t)o;
            g[live] = acc;
            ++live;
            i = j;
        }
    }
    *tap_max = live ? off[live - 1] : 0;
    return live;
}
