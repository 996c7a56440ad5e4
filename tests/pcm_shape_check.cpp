// pcm_shape_check.cpp — csrc/pcm_shape.h as a stand-alone host program for the sanitizers
// (tests/test_pcm_shape_host.py): the error-feedback host loop over exactly-sized heap
// blocks, input and output, at the edge lengths (a byte read or written outside is an ASan
// report), against a word-by-word restatement of the definition with its own history in
// 64-bit integers; NaN and infinities in mid-signal (a NaN or an infinity converted to an
// integer would be a UBSan report); the bounds on |E|, |A| and |F + D|.  Prints "bad N".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

#include "pcm_shape.h"

static int32_t unpack(const unsigned char* o, int bits) {
    uint32_t u = (uint32_t)o[0] | ((uint32_t)o[1] << 8);
    if (bits == 16) return (int32_t)(int16_t)u;
    u |= (uint32_t)o[2] << 16;
    return (int32_t)(u << 8) >> 8;
}

int main() {
    int bad = 0;
    const int64_t C = PCM_SHAPE_CHUNK;
    const int64_t words[] = {0, 1, 2, 3, 4, 5, 8, 9, 10, 11, C - 1, C, C + 1, 2 * C + 3, 20011};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t W : words)
        for (int ch = 1; ch <= 2; ++ch)
            for (int bits = 16; bits <= 24; bits += 8)
                for (int dither = 0; dither <= 1; ++dither)
                    for (int shape = PCM_SHAPE_E3; shape <= PCM_SHAPE_F9; ++shape) {
                        if (W % ch) continue;
                        const double S = (double)(1 << (bits - 1));
                        const int K = pcm_shape_taps(shape);
                        std::unique_ptr<float[]> x(new float[(size_t)W]);                     // exactly W words
                        std::unique_ptr<unsigned char[]> out(new unsigned char[(size_t)pcm_bytes(W, bits)]);
                        uint32_t s = (uint32_t)(W * 2654435761u + ch + 16 * shape);
                        for (int64_t i = 0; i < W; ++i) {
                            s = s * 1664525u + 1013904223u;
                            x[(size_t)i] = ((float)(s >> 8) * 0x1p-24f - 0.5f) * 2.4f;        // clips now and then
                        }
                        if (W > 1000) { x[301] = inf; x[700] = nan; x[1100] = -inf; x[1401] = nan; }
                        PcmRec r;
                        int64_t max_e = -1;
                        pcm_shape_host(x.get(), ch, W / ch, bits, dither, shape, 7, 3, out.get(), &r, &max_e);
                        const uint64_t k = pcm_stream_key(7, 3);
                        int64_t clipped = 0, nans = 0, big = 0;
                        int64_t E[2][PCM_SHAPE_KMAX] = {{0}};
                        int32_t lo = 0, hi = 0;
                        for (int64_t w = 0; w < W; ++w) {
                            int64_t* e = E[ch == 2 ? (w & 1) : 0];
                            const int64_t D = dither ? pcm_dither_int(pcm_arg(k, (uint64_t)w)) : 0;
                            int64_t A = 0;
                            for (int j = 0; j < K; ++j) A += (int64_t)pcm_shape_h(shape, j + 1) * e[j];
                            const int64_t F = (A + 32768) >> 16;
                            if (A >= (1ll << 46) || A <= -(1ll << 46) || F + D >= (1ll << 30) || F + D <= -(1ll << 30)) ++bad;
                            const double y = (double)x[(size_t)w] * S + (double)(F + D) * 0x1p-24;
                            const double rr = std::nearbyint(y);
                            const bool isnan = y != y, clip = rr < -S || rr > S - 1;
                            double want = rr;
                            if (isnan) { want = 0.0; ++nans; }
                            if (rr < -S) { want = -S; ++clipped; }
                            if (rr > S - 1) { want = S - 1; ++clipped; }
                            const int64_t fed = (isnan || clip) ? 0 : (int64_t)std::nearbyint((rr - y) * 0x1p24) + D;
                            for (int j = K - 1; j >= 1; --j) e[j] = e[j - 1];
                            e[0] = fed;
                            big = std::llabs(fed) > big ? std::llabs(fed) : big;
                            const int32_t q = unpack(out.get() + w * (bits / 8), bits);
                            if (q != (int32_t)want) ++bad;
                            lo = w == 0 || q < lo ? q : lo;
                            hi = w == 0 || q > hi ? q : hi;
                        }
                        if (r.clipped != clipped || r.nan != nans || r.q_min != lo || r.q_max != hi || r.bits != bits ||
                            r.dither != dither || max_e != big || big >= 3 * (1ll << 23)) {
                            std::printf("W %lld ch %d bits %d dither %d shape %d: clipped %lld (%lld) nan %lld (%lld) "
                                        "range [%d, %d] ([%d, %d]) max |E| %lld (%lld)\n",
                                        (long long)W, ch, bits, dither, shape, (long long)r.clipped, (long long)clipped,
                                        (long long)r.nan, (long long)nans, r.q_min, r.q_max, lo, hi, (long long)max_e,
                                        (long long)big);
                            ++bad;
                        }
                    }
    // an empty signal with null buffers, and the shape checks
    PcmRec r;
    pcm_shape_host(nullptr, 2, 0, 24, PCM_DITHER_TPDF, PCM_SHAPE_F9, 1, 2, nullptr, &r);
    if (r.clipped || r.nan || r.q_min || r.q_max || r.bits != 24 || r.dither != 1) ++bad;
    if (pcm_shape_ok(0) || pcm_shape_ok(4) || !pcm_shape_ok(PCM_SHAPE_E3) || !pcm_shape_ok(PCM_SHAPE_F9)) ++bad;
    if (pcm_shape_taps(PCM_SHAPE_E3) != 3 || pcm_shape_taps(PCM_SHAPE_LIPSHITZ5) != 5 || pcm_shape_taps(PCM_SHAPE_F9) != 9) ++bad;
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
