// er_merge_check.cpp — audio-suite_amd/csrc/er_merge.h against a brute-force
// merge (a std::map<offset, double> accumulated in tap order), over random tap
// sets with heavy offset duplication and offsets at and beyond both ends of
// the output (0, negatives, out_n - 1, out_n, later).  The host-gain form must
// equal the brute force (live count, sorted offsets, bit-equal gains); the
// device-gain form's key ranges, summed in order, must give the same bits.
// Prints "cases N bad N".
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>
#include "er_merge.h"

int main() {
    std::mt19937_64 rng(24680);
    std::uniform_real_distribution<double> gain(-1.0, 1.0);
    int bad = 0, cases = 0;
    const int64_t outs[] = {1, 2, 3, 17, 4800, 65537, (int64_t)1 << 24};
    for (int64_t out_n : outs)
        for (int nt : {1, 2, 7, 320, 2000})
            for (int rep = 0; rep < 12; ++rep) {
                // a few distinct offsets for many taps (rep picks how few), the edges always among them
                const int64_t span = std::min<int64_t>(out_n + 8, rep % 3 == 0 ? 5 : rep % 3 == 1 ? 97 : out_n + 8);
                const int32_t edges[] = {0, -1, -12345, (int32_t)(out_n - 1), (int32_t)out_n, (int32_t)(out_n + 1),
                                         (int32_t)std::min<int64_t>(2 * out_n + 7, INT32_MAX)};
                std::vector<int32_t> off0(nt);
                std::vector<double> g0(nt);
                for (int k = 0; k < nt; ++k) {
                    const uint64_t r = rng();
                    off0[k] = (r & 7) == 0 ? edges[(r >> 3) % 7] : (int32_t)((int64_t)((r >> 3) % (uint64_t)(span + 4)) - 3);
                    g0[k] = gain(rng);
                }
                std::map<int32_t, double> ref;                       // tap order: the first gain, then +=
                for (int k = 0; k < nt; ++k) {
                    if (!(off0[k] > 0 && off0[k] < out_n)) continue;
                    auto it = ref.find(off0[k]);
                    if (it == ref.end()) ref.emplace(off0[k], g0[k]);
                    else it->second += g0[k];
                }
                bool ok = true;
                // host-gain form
                std::vector<int32_t> off(off0);
                std::vector<double> g(g0);
                int32_t tmax = -1;
                const int live = er_merge_taps(nt, out_n, off.data(), g.data(), nullptr, nullptr, nullptr, &tmax);
                ok = ok && live == (int)ref.size();
                int i = 0;
                for (auto it = ref.begin(); ok && it != ref.end(); ++it, ++i)
                    ok = off[i] == it->first && std::memcmp(&g[i], &it->second, sizeof(double)) == 0;
                ok = ok && tmax == (live ? off[live - 1] : 0) && tmax == (ref.empty() ? 0 : ref.rbegin()->first);
                // device-gain form
                std::vector<int32_t> offd(off0), kx(nt), first(nt), cnt(nt);
                int32_t tmaxd = -1;
                const int lived = er_merge_taps(nt, out_n, offd.data(), nullptr, kx.data(), first.data(), cnt.data(), &tmaxd);
                ok = ok && lived == live && tmaxd == tmax;
                for (int j = 0; ok && j < live; ++j) {
                    ok = offd[j] == off[j] && cnt[j] >= 1 && first[j] >= 0 && first[j] + cnt[j] <= nt;
                    if (!ok) break;
                    double acc = g0[kx[first[j]]];
                    for (int q = 1; q < cnt[j]; ++q) acc += g0[kx[first[j] + q]];
                    ok = std::memcmp(&acc, &g[j], sizeof(double)) == 0;
                }
                ++cases;
                if (!ok) ++bad;
            }
    printf("cases %d bad %d\n", cases, bad);
    return bad != 0;
}
