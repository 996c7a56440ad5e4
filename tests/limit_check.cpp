// limit_check.cpp — csrc/limit.h as a stand-alone host program for the sanitizers
// (tests/test_limit_host.py): the weight table's padding and sum, the host loop in place over
// exactly-sized heap blocks at the edge lengths and look-aheads (a read or write one frame
// outside is an ASan report), the sample-peak guarantee, the record's consistency, the NaN
// rule.  Prints "bad N".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "limit.h"

int main() {
    int bad = 0;
    for (int L : {1, 2, 12, 72, 240, 4096}) {
        std::vector<float> w((size_t)lim_taps4(L));
        lim_weights(L, w.data());
        double sum = 0.0;
        for (int k = 0; k < lim_taps4(L); ++k) {
            sum += (double)w[(size_t)k];
            if (k <= 2 * L ? !(w[(size_t)k] > 0.0f) || w[(size_t)k] != w[(size_t)(2 * L - k)] : w[(size_t)k] != 0.0f) ++bad;
        }
        if (std::fabs(sum - 1.0) > (2 * L + 1) * 0x1p-25) { std::printf("L %d: the weights sum to %.9f\n", L, sum); ++bad; }
        if (lim_staged(L) % 4 || lim_words64(L) > lim_threads(L) || lim_lds_bytes(L) > 163840) ++bad;
    }
    const float c32 = 0.8912509f;
    for (int L : {1, 12, 240}) {
        const int64_t T = lim_tile(L);
        const int64_t lens[] = {0, 1, 2, 12, 25, L, 2 * L + 13, T - 1, T, T + 1, 2 * T + 1};
        for (int64_t n : lens)
            for (int ch = 1; ch <= 2; ++ch)
                for (int64_t sr : {48000, 96000, 384000}) {
                    std::unique_ptr<float[]> x(new float[(size_t)(n * ch)]);   // exactly n frames
                    uint32_t s = (uint32_t)(n * 2654435761u + ch + L);
                    for (int64_t i = 0; i < n * ch; ++i) {
                        s = s * 1664525u + 1013904223u;
                        x[(size_t)i] = ((float)(s >> 8) * 0x1p-24f - 0.5f) * ((s & 0xff) < 3 ? 3.0f : 0.2f);
                    }
                    std::vector<float> before(x.get(), x.get() + n * ch);
                    LimitRec r;
                    lim_host(x.get(), ch, n, sr, c32, L, &r);
                    int64_t changed = 0;
                    double pk = 0.0;
                    for (int64_t f = 0; f < n; ++f) {
                        bool diff = false;
                        for (int c = 0; c < ch; ++c) {
                            const float a = before[(size_t)(f * ch + c)], b = x[(size_t)(f * ch + c)];
                            diff = diff || std::memcmp(&a, &b, 4) != 0;
                            pk = std::fabs((double)b) > pk ? std::fabs((double)b) : pk;
                            if (std::fabs(b) > std::fabs(a)) ++bad;
                        }
                        changed += diff;
                    }
                    const bool ok = pk <= (double)c32 * (1.0 + 0x1p-22) && r.lookahead == L && changed <= r.limited_frames &&
                                    r.state == (r.limited_frames ? 1 : 0) && r.min_gain > 0.0 &&
                                    (r.limited_frames ? r.min_gain < 1.0 : r.min_gain == 1.0) &&
                                    r.reduction_db == 0.0 - tp_db(r.min_gain);
                    if (!ok) {
                        std::printf("L %d n %lld ch %d sr %lld: peak %.9g min_gain %.9g frames %lld changed %lld state %d\n", L,
                                    (long long)n, ch, (long long)sr, pk, r.min_gain, (long long)r.limited_frames,
                                    (long long)changed, r.state);
                        ++bad;
                    }
                    if (n > 0) {                                                // one NaN: untouched, state 2
                        std::vector<float> y(before);
                        y[(size_t)((n / 2) * ch)] = NAN;
                        std::vector<float> keep(y);
                        lim_host(y.data(), ch, n, sr, c32, L, &r);
                        if (std::memcmp(y.data(), keep.data(), y.size() * 4) != 0 || r.state != 2 || r.limited_frames != 0 ||
                            r.min_gain != 1.0)
                            ++bad;
                    }
                }
    }
    {                                                                           // the largest look-ahead once
        const int L = LIM_L_MAX;
        const int64_t n = 2 * L + 100;
        std::unique_ptr<float[]> x(new float[(size_t)n]);
        for (int64_t i = 0; i < n; ++i) x[(size_t)i] = i == L ? 2.0f : 0.01f;
        LimitRec r;
        lim_host(x.get(), 1, n, 384000, c32, L, &r);
        if (r.state != 1 || r.limited_frames != n || std::fabs(x[(size_t)L]) > c32 * (1.0f + 0x1p-22f)) ++bad;
    }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
