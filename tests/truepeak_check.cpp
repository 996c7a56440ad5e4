// truepeak_check.cpp — csrc/truepeak.h as a stand-alone host program for the sanitizers
// (tests/test_truepeak_host.py): the tap table's unit sums and mirror images, the host
// loop over exactly-sized heap blocks at the edge lengths (a read one frame outside
// is an ASan report), dbtp against the C library within 1e-12 dB.  Prints "bad N".
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "truepeak.h"

int main() {
    int bad = 0;
    float tab[TP_TAB_N];
    tp_table(tab);
    for (int os = 2; os <= 4; os += 2)
        for (int p = 1; p < os; ++p) {
            const float* t = tab + tp_tab_at(os) + (p - 1) * TP_TAPS;
            const float* u = tab + tp_tab_at(os) + (os - p - 1) * TP_TAPS;
            double sum = 0.0;
            for (int q = 0; q < TP_TAPS; ++q) {
                sum += (double)t[q];
                if (t[q] != u[TP_TAPS - 1 - q]) ++bad;
            }
            if (std::fabs(sum - 1.0) > 24 * 0x1p-24) { std::printf("phase %d of %d sums to %.9f\n", p, os, sum); ++bad; }
        }
    const int64_t lens[] = {0, 1, 2, 11, 12, 13, 23, 24, 25, TP_TILE - 1, TP_TILE, TP_TILE + 1, 2 * TP_TILE + 1};
    for (int64_t n : lens)
        for (int ch = 1; ch <= 2; ++ch)
            for (int64_t sr : {48000, 96000, 384000}) {
                std::unique_ptr<float[]> x(new float[(size_t)(n * ch)]);       // exactly n frames
                uint32_t s = (uint32_t)(n * 2654435761u + ch);
                for (int64_t i = 0; i < n * ch; ++i) {
                    s = s * 1664525u + 1013904223u;
                    x[(size_t)i] = ((float)(s >> 8) * 0x1p-24f - 0.5f) * 0.2f;
                }
                TruePeakRec r;
                tp_host(x.get(), ch, n, sr, &r);
                double pk = 0.0;
                for (int64_t i = 0; i < n * ch; ++i) pk = std::fabs((double)x[(size_t)i]) > pk ? std::fabs((double)x[(size_t)i]) : pk;
                if (r.peak != pk || r.true_peak < r.peak || r.true_peak > 2.25 * pk || r.os != tp_os(sr) || r.gain != 0.0) {
                    std::printf("n %lld ch %d sr %lld: peak %.9g true peak %.9g\n", (long long)n, ch, (long long)sr, r.peak,
                                r.true_peak);
                    ++bad;
                }
                if (n == 0 ? !(r.dbtp < -1e300) : std::fabs(r.dbtp - 20.0 * std::log10(r.true_peak)) > 1e-12) ++bad;
            }
    const float edge[] = {1.0f, 0.99999994f, 1.0000001f, 1.4142135f, 1.4142137f, 0.70710677f, 0.70710683f, 2.0f, 0.5f,
                          1e-38f, 1.4e-45f, 3.4028235e38f, 10.0f, 1e10f};
    for (float v : edge) {
        const double d = tp_db((double)v), want = 20.0 * std::log10((double)v);
        if (std::fabs(d - want) > 1e-12 * (1.0 + std::fabs(want))) { std::printf("tp_db(%.9g) = %.17g, libm %.17g\n", v, d, want); ++bad; }
    }
    if (tp_db(10.0) != 20.0 || tp_db(100.0) != 40.0 || tp_db(1.0) != 0.0 || !(tp_db(0.0) < -1e300)) ++bad;
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
