// loudness_check.cpp — host check of csrc/loudness.h, built with ASan + UBSan by
// tests/test_loudness_host.py: the table of a rate against the recurrence it stands
// for (the state L frames on is A^L s + the zero-state end state, for every L the
// kernels use), the tile counts, and the host loop at the edge lengths.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>
#include "loudness.h"

static int bad = 0;
static void expect(bool ok, const char* what, long a, long b) {
    if (!ok) { ++bad; std::printf("FAIL %s (%ld, %ld)\n", what, a, b); }
}

static void check_power(const double* tab, int at, int64_t L, int64_t sr, std::mt19937& g) {
    std::normal_distribution<double> nd;
    const double* c = tab + LD_TAB_COEF;
    std::vector<float> x((size_t)L);
    for (auto& v : x) v = (float)(0.5 + 0.1 * nd(g));
    double s0[4], s[4], e[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) s[i] = s0[i] = 100.0 * nd(g);
    for (int64_t k = 0; k < L; ++k) { ld_step(c, s, x[(size_t)k]); ld_step(c, e, x[(size_t)k]); }
    double scale = 0.0;
    for (int i = 0; i < 4; ++i) scale = std::fmax(scale, std::fabs(s[i]));
    for (int i = 0; i < 4; ++i) {
        double r = e[i];
        for (int j = 0; j < 4; ++j) r += tab[at + 4 * i + j] * s0[j];
        expect(std::fabs(r - s[i]) <= 1e-9 * (scale + 1.0), "A^L s + e", (long)sr, (long)L);
    }
}

int main() {
    std::mt19937 g(3);
    for (int64_t sr : {44100, 48000, 96000, 384000}) {
        std::vector<double> tab(LD_TAB_N);
        ld_table(sr, tab.data());
        const int64_t hop = sr / 10;
        for (int l = 0; l <= 64; ++l) check_power(tab.data(), LD_TAB_LANE + 16 * l, (int64_t)LD_C * l, sr, g);
        for (int k = 0; k < 6; ++k) check_power(tab.data(), LD_TAB_LVL + 16 * k, (int64_t)LD_C << k, sr, g);
        check_power(tab.data(), LD_TAB_WAVE, 64 * LD_C, sr, g);
        check_power(tab.data(), LD_TAB_AT, LD_TILE, sr, g);
        check_power(tab.data(), LD_TAB_AR, hop % LD_TILE, sr, g);
        // tiles: every frame in exactly one tile, none across a hop
        for (int64_t n : {(int64_t)0, (int64_t)1, hop - 1, hop, hop + 1, 4 * hop - 1, 4 * hop, 5 * hop + LD_TILE + 1}) {
            const int64_t tph = ld_tiles_per_hop(hop);
            int64_t covered = 0;
            for (int64_t t = 0; t < ld_tiles(n, hop); ++t) {
                const int64_t h = t / tph, ti = t % tph, hl = n - h * hop < hop ? n - h * hop : hop;
                const int64_t lt = hl - ti * LD_TILE < LD_TILE ? hl - ti * LD_TILE : LD_TILE;
                expect(lt > 0 && lt <= LD_TILE, "tile length", (long)n, (long)t);
                covered += lt;
            }
            expect(covered == n, "tiles cover the signal", (long)n, (long)covered);
            std::vector<float> x((size_t)(2 * n));
            std::normal_distribution<float> nf;
            for (auto& v : x) v = 0.1f * nf(g);
            LoudRec r1, r2;
            ld_host(x.data(), 1, n, sr, &r1);
            ld_host(x.data(), 2, n, sr, &r2);
            expect(r1.n_blocks == ld_blocks(n, hop) && r2.n_blocks == r1.n_blocks, "blocks", (long)n, (long)r1.n_blocks);
            expect((r1.n_blocks == 0) == std::isinf(r1.lufs), "no block, no level", (long)n, (long)r1.n_blocks);
        }
    }
    std::printf("bad %d\n", bad);
    return bad != 0;
}
