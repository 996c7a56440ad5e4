// flac_check.cpp — csrc/flac.h in a stand-alone program (built by tests/test_flac_host.py with
// -fsanitize=address,undefined): the sequential host loop (flac_host) against the block-wise helpers
// the kernels use, run as the kernels run them but on the host and in shuffled order: the plan of
// every channel from the lanes' chunk sums, the scan of the frame lengths, the pack into a zeroed
// buffer by OR, and CRC-16 from chunk CRCs.  Equal bytes, equal lengths; prints "bad 0".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "flac.h"

static int bad = 0;
static std::mt19937_64 rng(12345);

static std::vector<int> shuffled(int n) {
    std::vector<int> v((size_t)n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = i;
    std::shuffle(v.begin(), v.end(), rng);
    return v;
}

static void pack_pcm(const std::vector<int32_t>& q, int bits, std::vector<uint8_t>& out) {
    out.clear();
    for (int32_t v : q)
        for (int b = 0; b < bits / 8; ++b) out.push_back((uint8_t)((uint32_t)v >> (8 * b)));
}

// one block as the plan and pack sweeps see it; returns the frame's bytes
static std::vector<uint8_t> block_frame(const uint8_t* pcm, int channels, int bits, int64_t n, int B, int64_t sr, int64_t j,
                                        int lanes, FlacPlan* plan_out) {
    const int bn = (int)(n - j * B < B ? n - j * B : B);
    std::vector<int32_t> xl((size_t)FLAC_XS, 0), xr((size_t)FLAC_XS, 0);
    for (int i = 0; i < bn; ++i) {
        const int64_t f = j * B + i;
        xl[(size_t)flac_pos(i)] = flac_load(pcm, bits, f * channels);
        if (channels == 2) xr[(size_t)flac_pos(i)] = flac_load(pcm, bits, f * channels + 1);
    }
    const int cw = (bn + lanes - 1) / lanes;
    auto lo = [&](int t) { return std::min(bn, t * cw); };
    auto hi = [&](int t) { return std::min(bn, lo(t) + cw); };
    const FlacAddPlain add{};
    FlacBest best[4];
    std::vector<uint32_t> us((size_t)lanes * FLAC_C);
    for (int c = 0; c < (channels == 2 ? 4 : 1); ++c) {
        const FlacX x{xl.data(), channels == 2 ? xr.data() : xl.data(), c};
        FlacWork W;
        for (int t : shuffled(128)) flac_work_zero(&W, t);
        flac_work_init(&W);
        for (int t : shuffled(lanes)) flac_chunk_abs(x, lo(t), hi(t), &W, add);
        const int o = flac_order(W.abs), pm = flac_pmax(bn, o);
        if (bn > 4 && W.mn != W.mx) {
            for (int t : shuffled(lanes))
                flac_chunk_S(x, lo(t), hi(t), o, pm, bn, *reinterpret_cast<uint32_t(*)[FLAC_C]>(&us[(size_t)t * FLAC_C]), &W, add);
            for (int t : shuffled(127)) flac_entry_k0(&W, bn, o, pm, bits, t);
            for (int t : shuffled(lanes))
                flac_chunk_E(*reinterpret_cast<uint32_t(*)[FLAC_C]>(&us[(size_t)t * FLAC_C]), lo(t), hi(t), pm, bn, &W, add);
            for (int t : shuffled(127)) flac_entry_pick(&W, bn, o, pm, bits, t);
        }
        flac_finish(&W, bn, bits + (c == 3), bits, o, pm, &best[c]);
    }
    uint8_t hdr[FLAC_HDR_MAX];
    FlacPlan P;
    int hb = flac_header(hdr, B, bn, sr, channels == 2 ? 0 : -1, bits, j);
    flac_assign(best, channels, hb, &P);
    *plan_out = P;

    const int total = P.bytes;
    if (total < 4 || total > (int)flac_frame_bound(bn, channels, bits)) { ++bad; return {}; }
    std::vector<uint32_t> fw((size_t)(total + 3) / 4 + 1, 0);
    const FlacOrPlain orr{};
    hb = flac_header(hdr, B, bn, sr, P.assign, bits, j);
    for (int t : shuffled(hb)) flac_put(orr, fw.data(), 8 * t, hdr[t], 8);
    int64_t pos = 8 * hb;
    for (int s = 0; s < channels; ++s) {
        const int c = flac_assign_chan(P.assign, s), d = bits + (c == 3);
        const FlacX x{xl.data(), channels == 2 ? xr.data() : xl.data(), c};
        const FlacBest& sub = P.sub[s];
        const int64_t first = flac_sub_head(x, sub, d, bits, pos, fw.data(), orr, true);
        if (sub.type == FLAC_TYPE_CONSTANT) {
            pos = first + d;
        } else if (sub.type == FLAC_TYPE_VERBATIM) {
            for (int i : shuffled(bn)) flac_put(orr, fw.data(), first + (int64_t)i * d, (uint32_t)x(i) & flac_mask(d), d);
            pos = first + (int64_t)bn * d;
        } else {
            const int o = sub.order;
            for (int t : shuffled(o)) flac_put(orr, fw.data(), first + (int64_t)t * d, (uint32_t)x(t) & flac_mask(d), d);
            std::vector<int64_t> len((size_t)lanes), ex((size_t)lanes);
            for (int t : shuffled(lanes))
                len[(size_t)t] = flac_chunk_len(x, lo(t), hi(t), sub, bn, bits, *reinterpret_cast<uint32_t(*)[FLAC_C]>(&us[(size_t)t * FLAC_C]));
            int64_t all = 0;
            for (int t = 0; t < lanes; ++t) { ex[(size_t)t] = all; all += len[(size_t)t]; }
            const int64_t base = first + (int64_t)o * d + 6;
            for (int t : shuffled(lanes))
                flac_chunk_pack(*reinterpret_cast<uint32_t(*)[FLAC_C]>(&us[(size_t)t * FLAC_C]), lo(t), hi(t), sub, bn, bits,
                                base + ex[(size_t)t], fw.data(), orr);
            pos = base + all;
        }
    }
    const int nb = total - 2;
    if ((pos + 7) >> 3 != nb) { ++bad; std::printf("length: plan %d, packed %lld\n", nb, (long long)((pos + 7) >> 3)); return {}; }
    const int m = (nb + lanes - 1) / lanes;
    uint32_t crc = 0;
    for (int t : shuffled(lanes)) {
        const int a0 = std::min(nb, t * m), a1 = std::min(nb, a0 + m);
        uint32_t cc = 0;
        for (int a = a0; a < a1; ++a) cc = flac_crc16(cc, flac_byte(fw.data(), a));
        crc ^= flac_mulmod16(cc, flac_xpow16((uint32_t)(nb - a1)));
    }
    flac_put(orr, fw.data(), (int64_t)nb * 8, crc, 16);
    std::vector<uint8_t> out((size_t)total);
    for (int a = 0; a < total; ++a) out[(size_t)a] = (uint8_t)flac_byte(fw.data(), a);
    return out;
}

static void check(const char* name, const std::vector<int32_t>& q, int channels, int bits, int B, int64_t sr) {
    const int64_t n = (int64_t)q.size() / channels;
    std::vector<uint8_t> pcm;
    pack_pcm(q, bits, pcm);
    pcm.resize(pcm.size() + 1);                   // never an empty buffer
    std::vector<uint8_t> ref((size_t)flac_bound(n, channels, bits, B) + 1);
    FlacRec rec;
    flac_host(pcm.data(), channels, bits, n, B, sr, true, ref.data(), &rec);
    if (rec.bytes > flac_bound(n, channels, bits, B)) { ++bad; std::printf("%s: beyond the bound\n", name); }
    std::vector<uint8_t> got;
    int32_t mn = 0, mx = 0;
    int64_t frames = 0;
    for (int lanes : {FLAC_T, 64}) {
        if (lanes * FLAC_C < B) continue;          // a lane's chunk is at most FLAC_C samples
        got.clear();
        frames = 0;
        for (int64_t j = 0; j * B < n; ++j) {
            FlacPlan P;
            const std::vector<uint8_t> f = block_frame(pcm.data(), channels, bits, n, B, sr, j, lanes, &P);
            if ((int)f.size() != P.bytes) ++bad;
            mn = frames == 0 || P.bytes < mn ? P.bytes : mn;
            mx = frames == 0 || P.bytes > mx ? P.bytes : mx;
            ++frames;
            got.insert(got.end(), f.begin(), f.end());
        }
        const bool same = (int64_t)got.size() == rec.bytes && std::equal(got.begin(), got.end(), ref.begin());
        if (!same || frames != rec.frames || (frames && (mn != rec.min_frame || mx != rec.max_frame))) {
            ++bad;
            std::printf("%s ch %d bits %d B %d n %lld lanes %d: %zu bytes against %lld\n", name, channels, bits, B, (long long)n,
                        lanes, got.size(), (long long)rec.bytes);
        }
    }
}

int main() {
    // the CRC of "123456789", the concatenation identity and an MD5
    const char* d = "123456789";
    uint32_t c8 = 0, c16 = 0;
    for (int i = 0; i < 9; ++i) { c8 = flac_crc8(c8, (uint8_t)d[i]); c16 = flac_crc16(c16, (uint8_t)d[i]); }
    if (c8 != 0xF4 || c16 != 0xFEE8) { ++bad; std::printf("crc %x %x\n", c8, c16); }
    uint32_t ca = 0, cb = 0;
    for (int i = 0; i < 4; ++i) ca = flac_crc16(ca, (uint8_t)d[i]);
    for (int i = 4; i < 9; ++i) cb = flac_crc16(cb, (uint8_t)d[i]);
    if ((flac_mulmod16(ca, flac_xpow16(5)) ^ cb) != 0xFEE8) { ++bad; std::printf("crc identity\n"); }
    uint8_t md[16];
    flac_md5_host(reinterpret_cast<const uint8_t*>("abc"), 3, md);
    if (md[0] != 0x90 || md[1] != 0x01 || md[15] != 0x72) { ++bad; std::printf("md5\n"); }

    int cases = 0;
    for (int bits : {16, 24}) {
        const int32_t S = 1 << (bits - 1);
        for (int channels : {1, 2}) {
            for (int B : {256, 1024, 4096}) {
                for (int64_t n : {0, 1, 4, 5, 255, 256, 257, 1000, 1024, 4095, 4096, 4097, 4096 + 1536}) {
                    if (n > 3 * (int64_t)B + 100 && B < 4096) continue;
                    std::vector<int32_t> q((size_t)(n * channels));
                    std::uniform_int_distribution<int32_t> full(-S, S - 1);
                    std::normal_distribution<double> g(0.0, 0.1 * S);
                    for (int kind = 0; kind < 8; ++kind) {
                        for (int64_t i = 0; i < n; ++i)
                            for (int c = 0; c < channels; ++c) {
                                int32_t v = 0;
                                switch (kind) {
                                    case 0: v = full(rng); break;                                         // full-scale noise
                                    case 1: v = (int32_t)std::lrint(0.1 * S * std::sin(0.0576 * (double)i + c)) + (int32_t)(full(rng) % 3); break;
                                    case 2: v = c ? -1234 : 77; break;                                    // constant
                                    case 3: v = ((i & 1) ? S - 1 : -S); if (c) v = -v - 1; break;           // alternation, L = -R - 1
                                    case 4: v = (i == n / 2) ? S - 1 : 0; break;                          // a lone sample
                                    case 5: v = (int32_t)std::max<double>(-S, std::min<double>(S - 1, g(rng))); if (c) v = q[(size_t)(i * channels)]; break;
                                    case 6: v = c ? 0 : (int32_t)(full(rng) >> 6); break;                 // one silent channel
                                    default: v = (int32_t)(full(rng) >> (i * 13 / (n + 1) + 3)); break;   // a decay
                                }
                                q[(size_t)(i * channels + c)] = v;
                            }
                        check("case", q, channels, bits, B, kind & 1 ? 44101 : 48000);
                        ++cases;
                    }
                }
            }
        }
    }
    std::printf("cases %d bad %d\n", cases, bad);
    return bad ? 1 : 0;
}
