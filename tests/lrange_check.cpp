// lrange_check.cpp — host check of csrc/lrange.h, built with ASan + UBSan by
// tests/test_lrange_host.py: the record from hop sums at every edge count against a
// sort-free restatement (counting ranks), the stated empty cases, ties across a rank, and
// the host loop over short signals.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>
#include "lrange.h"

static int bad = 0;
static void expect(bool ok, const char* what, long a, long b) {
    if (!ok) { ++bad; std::printf("FAIL %s (%ld, %ld)\n", what, a, b); }
}

// v is element `rank` of the kept values in ascending order: fewer than rank + 1 lie below it, at least rank + 1 at or below
static bool is_rank(const std::vector<double>& kept, double v, int64_t rank) {
    int64_t below = 0, upto = 0;
    for (double k : kept) { below += k < v; upto += k <= v; }
    return below <= rank && rank < upto;
}

static void check_hops(const std::vector<double>& H, int64_t hop) {
    const int64_t hops = (int64_t)H.size();
    LRangeRec r;
    lr_hops_host(H.data(), hops, hop, &r);
    const int64_t nb = hops < 4 ? 0 : hops - 3, ns = hops < 30 ? 0 : hops - 29;
    expect(r.n_momentary == nb && r.n_short == ns, "counts", (long)hops, (long)r.n_short);
    double zm = 0.0, zs = 0.0;
    std::vector<double> w((size_t)ns), kept;
    for (int64_t j = 0; j < nb; ++j) zm = std::fmax(zm, (((H[j] + H[j + 1]) + H[j + 2]) + H[j + 3]) / (4.0 * (double)hop));
    int64_t c1 = 0;
    for (int64_t i = 0; i < ns; ++i) {
        double a = H[(size_t)i];
        for (int k = 1; k < 30; ++k) a += H[(size_t)(i + k)];
        w[(size_t)i] = a / (30.0 * (double)hop);
        zs = std::fmax(zs, w[(size_t)i]);
        c1 += ld_level(w[(size_t)i]) > -70.0;
    }
    expect(r.z_max_m == zm && r.z_max_s == zs, "maxima", (long)hops, 0);
    expect(r.n_abs == c1, "absolute gate", (long)r.n_abs, (long)c1);
    expect((nb == 0) == (std::isinf(r.max_momentary) && r.max_momentary < 0) || zm == 0.0, "no block, no level", (long)hops, 0);
    for (int64_t i = 0; i < ns; ++i) {
        const double l = ld_level(w[(size_t)i]);
        if (l > -70.0 && l > r.gate) kept.push_back(w[(size_t)i]);
    }
    expect(r.n_kept == (int64_t)kept.size(), "relative gate", (long)r.n_kept, (long)kept.size());
    if (c1 == 0) expect(std::isinf(r.gate) && r.gate < 0, "no window, gate -inf", (long)hops, 0);
    if (kept.empty()) {
        expect(r.lra == 0.0 && r.z_lo == 0.0 && r.z_hi == 0.0 && std::isinf(r.lo) && std::isinf(r.hi), "empty record", (long)hops, 0);
    } else {
        const int64_t c2 = (int64_t)kept.size();
        expect(is_rank(kept, r.z_lo, ((c2 - 1) * 10 + 50) / 100), "10th percentile", (long)hops, (long)c2);
        expect(is_rank(kept, r.z_hi, ((c2 - 1) * 95 + 50) / 100), "95th percentile", (long)hops, (long)c2);
        expect(r.lra == r.hi - r.lo && r.lra >= 0.0, "lra", (long)hops, (long)c2);
    }
}

int main() {
    std::mt19937 g(7);
    std::uniform_real_distribution<double> u(-6.0, 1.0);
    const int64_t hop = 4800;
    for (int64_t hops : {0, 1, 3, 4, 29, 30, 31, 39, 40, 41, 255, 285, 286, 1200}) {
        std::vector<double> H((size_t)hops);
        for (auto& v : H) v = (double)hop * std::pow(10.0, u(g));          // seven decades: both gates at work
        check_hops(H, hop);
        for (auto& v : H) v = 0.125 * (double)hop;                          // all equal: every rank the same value
        check_hops(H, hop);
        if (hops) {
            LRangeRec r;
            lr_hops_host(H.data(), hops, hop, &r);
            expect(r.lra == 0.0, "all equal, lra 0", (long)hops, 0);
        }
        for (auto& v : H) v = 0.0;                                          // silent
        check_hops(H, hop);
        for (size_t i = 0; i < H.size(); ++i) H[i] = (i / 40) % 2 ? 4.0 * (double)hop : 1e-3 * (double)hop;   // runs of ties
        check_hops(H, hop);
    }
    // the host loop at the edge lengths (hop 400 at 4 kHz), mono and stereo
    for (int64_t n : {0, 1, 399, 400, 1599, 1600, 11999, 12000, 12399, 12400}) {
        std::vector<float> x((size_t)(2 * n));
        std::normal_distribution<float> nf;
        for (auto& v : x) v = 0.1f * nf(g);
        for (int ch = 1; ch <= 2; ++ch) {
            LoudRec l, l0;
            LRangeRec r, r2;
            lr_host(x.data(), ch, n, 4000, &l, &r);
            lr_host(x.data(), ch, n, 4000, nullptr, &r2);
            ld_host(x.data(), ch, n, 4000, &l0);
            expect(l.lufs == l0.lufs || (std::isinf(l.lufs) && std::isinf(l0.lufs)), "loudness record", (long)n, ch);
            expect(l.n_blocks == l0.n_blocks && l.n_kept == l0.n_kept && l.peak == l0.peak, "loudness counts", (long)n, ch);
            expect(r.n_momentary == l.n_blocks, "momentary blocks are msg_loudness's", (long)n, (long)r.n_momentary);
            expect(r.n_short == (n / 400 < 30 ? 0 : n / 400 - 29), "windows", (long)n, (long)r.n_short);
            expect(r.z_max_s == r2.z_max_s && r.z_lo == r2.z_lo && r.n_kept == r2.n_kept, "no loudness record taken", (long)n, ch);
        }
    }
    std::printf("bad %d\n", bad);
    return bad != 0;
}
