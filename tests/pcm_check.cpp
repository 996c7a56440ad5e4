// pcm_check.cpp — csrc/pcm.h as a stand-alone host program for the sanitizers
// (tests/test_pcm_host.py): the host loop over exactly-sized heap blocks, input and
// output, at the edge lengths (a byte read or written outside is an ASan report), the
// packing against a byte-by-byte restatement, the rounding and clipping edges, the
// record.  Prints "bad N".
#include <cmath>
#include <cstdio>
#include <limits>
#include <memory>

#include "pcm.h"

static int32_t unpack(const unsigned char* o, int bits) {
    uint32_t u = (uint32_t)o[0] | ((uint32_t)o[1] << 8);
    if (bits == 16) return (int32_t)(int16_t)u;
    u |= (uint32_t)o[2] << 16;
    return (int32_t)(u << 8) >> 8;
}

int main() {
    int bad = 0;
    const int64_t words[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 4095, 4096, 4097, 8195, 20011};
    for (int64_t W : words)
        for (int ch = 1; ch <= 2; ++ch)
            for (int bits = 16; bits <= 24; bits += 8)
                for (int dither = 0; dither <= 1; ++dither) {
                    if (W % ch) continue;
                    const double S = (double)(1 << (bits - 1));
                    std::unique_ptr<float[]> x(new float[(size_t)W]);                         // exactly W words
                    std::unique_ptr<unsigned char[]> out(new unsigned char[(size_t)pcm_bytes(W, bits)]);
                    uint32_t s = (uint32_t)(W * 2654435761u + ch);
                    for (int64_t i = 0; i < W; ++i) {
                        s = s * 1664525u + 1013904223u;
                        x[(size_t)i] = ((float)(s >> 8) * 0x1p-24f - 0.5f) * 2.4f;            // clips now and then
                    }
                    PcmRec r;
                    pcm_host(x.get(), ch, W / ch, bits, dither, 7, 3, out.get(), &r);
                    const uint64_t k = pcm_stream_key(7, 3);
                    int64_t clipped = 0;
                    int32_t lo = 0, hi = 0;
                    for (int64_t w = 0; w < W; ++w) {
                        const double d = dither ? pcm_dither_at(pcm_arg(k, (uint64_t)w)) : 0.0;
                        if (!(d > -1.0 && d < 1.0) || d * 0x1p24 != std::nearbyint(d * 0x1p24)) ++bad;
                        double want = std::nearbyint((double)x[(size_t)w] * S + d);
                        if (want < -S) { want = -S; ++clipped; }
                        if (want > S - 1) { want = S - 1; ++clipped; }
                        const int32_t q = unpack(out.get() + w * (bits / 8), bits);
                        if (q != (int32_t)want) ++bad;
                        lo = w == 0 || q < lo ? q : lo;
                        hi = w == 0 || q > hi ? q : hi;
                    }
                    if (r.clipped != clipped || r.nan != 0 || r.q_min != lo || r.q_max != hi || r.bits != bits ||
                        r.dither != dither) {
                        std::printf("W %lld ch %d bits %d dither %d: clipped %lld (%lld) range [%d, %d] ([%d, %d])\n",
                                    (long long)W, ch, bits, dither, (long long)r.clipped, (long long)clipped, r.q_min,
                                    r.q_max, lo, hi);
                        ++bad;
                    }
                }
    // the edges without dither, and pcm_pack4 against the host loop's bytes
    for (int bits = 16; bits <= 24; bits += 8) {
        const float S = (float)(1 << (bits - 1));
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        const float x[12] = {0.5f / S, -0.5f / S, 1.5f / S, -1.5f / S, 2.5f / S, -2.5f / S, 1.0f, -1.0f, inf, -inf, nan, 0.0f};
        const int32_t want[12] = {0, 0, 2, -2, 2, -2, (int32_t)S - 1, -(int32_t)S, (int32_t)S - 1, -(int32_t)S, 0, 0};
        std::unique_ptr<unsigned char[]> out(new unsigned char[(size_t)pcm_bytes(12, bits)]);
        PcmRec r;
        pcm_host(x, 1, 12, bits, PCM_DITHER_NONE, 0, 0, out.get(), &r);
        for (int w = 0; w < 12; ++w)
            if (unpack(out.get() + w * (bits / 8), bits) != want[w]) { std::printf("edge %d at %d bits\n", w, bits); ++bad; }
        if (r.clipped != 3 || r.nan != 1 || r.q_min != -(int32_t)S || r.q_max != (int32_t)S - 1) ++bad;
        for (int g = 0; g < 3; ++g) {
            uint32_t p[3];
            if (bits == 16) pcm_pack4<16>(want + 4 * g, p); else pcm_pack4<24>(want + 4 * g, p);
            unsigned char b[12];
            for (int j = 0; j < 12; ++j) b[j] = (unsigned char)(p[j / 4] >> (8 * (j % 4)));
            if (std::memcmp(b, out.get() + 4 * g * (bits / 8), (size_t)(4 * (bits / 8))) != 0) { std::printf("pack4 %d at %d bits\n", g, bits); ++bad; }
        }
    }
    PcmRec r;
    pcm_host(nullptr, 2, 0, 24, PCM_DITHER_TPDF, 1, 2, nullptr, &r);
    if (r.clipped || r.nan || r.q_min || r.q_max || r.bits != 24 || r.dither != 1) ++bad;
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
