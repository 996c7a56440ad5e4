// pcm_shape.h — noise-shaped dither for the PCM export (msg_quantize_shaped /
// msg_quantize_shaped_host): an error-feedback quantiser beside pcm.h's, the definition
// shared by the device kernel (kernels_pcm_shape.h) and the host loop below.  Plain C++.
//
// Words, S, the dither stream (seed, key, w), the packing and the record (clipped, nan,
// q_min, q_max) are pcm.h's.  dither is NONE (D = 0) or TPDF (D = a - b of pcm_dither_at,
// taken as the integer, |D| < 2^24).
//
// Shapes: K taps c_k, noise transfer function NTF(z) = 1 - sum c_k z^-k (Lipshitz,
// Vanderkooy and Wannamaker's published curves, designed for 44.1 kHz):
//   1 "e3"         1.623, -0.982, 0.109
//   2 "lipshitz5"  2.033, -2.165, 1.959, -1.590, 0.6149
//   3 "f9"         2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847
// The definition is the integer table H_k = -llround(c_k 65536) below.
//
// State: each channel of each signal keeps its own history E_1 .. E_K, integers in units
// of 2^-24 LSB, all 0 at the signal's first frame.  Channel c's word of frame f is still
// w = f channels + c of the dither stream.
//
// Step for word w:
//   A = sum_k H_k E_k                      int64, exact
//   F = (A + 32768) >> 16                  arithmetic shift (floor)
//   v = (double)x S                        exact
//   y = v + (double)(F + D) 2^-24          one rounded float64 add (the product is exact, so a
//                                          contracted fused step gives the same bits)
//   r = rint(y)                            ties to even
//   isnan = (y != y);  clip = r < -S || r > S - 1
//   q as in pcm_word: clamped, 0 for a NaN; clipped / nan / q_min / q_max counted as there
//   t = (isnan || clip) ? 0.0 : (r - y) 2^24       selected on the double, before any conversion
//   E_new = (int64)rint(t) + ((isnan || clip) ? 0 : D)
//   E_K .. E_2 = E_{K-1} .. E_1;  E_1 = E_new
// The error fed back is the total error, dither included, so the delivered error is
// NTF * e.  A clipped or NaN word feeds back 0: no wind-up, no NaN in the history, and no
// NaN or infinity is ever converted to an integer.  Every operation is exact integer
// arithmetic or one correctly rounded IEEE operation on exact operands: host, device and
// NumPy cannot differ by contraction.
//
// Bounds: |rint(t)| <= 2^23 and |D| < 2^24, so |E| < 1.5 2^24 (E fits int32); with
// sum |H_k| <= 21.39 2^16 (f9), |A| < 1.5 2^24 21.39 2^16 < 2^46 and |F + D| < 2^30 (F + D
// fits int32).  The output lies within 1.5 (1 + sum |c_k|) LSB of v: 33.6 LSB for f9.
//
// A channel is one chain from its first word to its last: it is never cut into blocks
// that start from an empty history (DESIGN.md §4h has the measurement), so a signal's bytes
// depend on the signal, bits, dither, shape, seed and key alone.
#pragma once
#include "pcm.h"

// the tap loops are unrolled on the device, where the history must stay in registers
#if defined(__HIPCC__)
#define PCM_SHAPE_UNROLL _Pragma("unroll")
#else
#define PCM_SHAPE_UNROLL
#endif

constexpr int PCM_SHAPE_E3 = 1, PCM_SHAPE_LIPSHITZ5 = 2, PCM_SHAPE_F9 = 3;   // MSG_SHAPE_* of msgpu.h
constexpr int PCM_SHAPE_KMAX = 9;
constexpr int PCM_SHAPE_CHUNK = 32;        // words a lane loads ahead of their use: eight 16-byte pieces
constexpr int PCM_SHAPE_T = 64;            // threads per workgroup: one wave, one signal per lane

MSG_HD bool pcm_shape_ok(int shape) { return shape >= PCM_SHAPE_E3 && shape <= PCM_SHAPE_F9; }
MSG_HD constexpr int pcm_shape_taps(int shape) { return shape == PCM_SHAPE_E3 ? 3 : (shape == PCM_SHAPE_LIPSHITZ5 ? 5 : 9); }

// H_k of `shape`, k = 1 .. K
MSG_HD constexpr int32_t pcm_shape_h(int shape, int k) {
    constexpr int32_t PCM_SHAPE_H[3][PCM_SHAPE_KMAX] = {
        {-106365, 64356, -7143, 0, 0, 0, 0, 0, 0},
        {-133235, 141885, -128385, 104202, -40298, 0, 0, 0, 0},
        {-158073, 220856, -258015, 273547, -219742, 144507, -83952, 37290, -5551},
    };
    return PCM_SHAPE_H[shape - 1][k - 1];
}

// D of the word whose stream argument is k + (w + 1) G: a - b as the integer
MSG_HD int32_t pcm_dither_int(uint64_t arg) {
    const uint64_t h = dg_fmix64(arg);
    return (int32_t)(h & 0xFFFFFFu) - (int32_t)((h >> 32) & 0xFFFFFFu);
}

// One channel's history.  tail = sum_{k >= 2} H_k E_k of the next word: it does not hold
// the newest error, so it is formed beside the step and only H_1 E_1 waits for it.
template <int SHAPE>
struct PcmShapeState {
    int32_t E[pcm_shape_taps(SHAPE)];
    int64_t tail;
};
template <int SHAPE>
MSG_HD void pcm_shape_reset(PcmShapeState<SHAPE>& st) {
    PCM_SHAPE_UNROLL
    for (int k = 0; k < pcm_shape_taps(SHAPE); ++k) st.E[k] = 0;
    st.tail = 0;
}

// one word of one channel: the step above.  D: the word's dither integer (0 without dither)
template <int SHAPE>
MSG_HD int32_t pcm_shape_word(float x, double S, int32_t D, PcmShapeState<SHAPE>& st, PcmAcc& acc) {
    constexpr int K = pcm_shape_taps(SHAPE);
    const int64_t A = st.tail + (int64_t)pcm_shape_h(SHAPE, 1) * st.E[0];
    const int32_t FD = (int32_t)((A + 32768) >> 16) + D;     // |F + D| < 2^30
    const double v = (double)x * S;
    const double y = v + (double)FD * 0x1p-24;
    // selects, not branches, as in pcm_word
    const bool isnan = !(y == y);
    double r = __builtin_rint(y);
    const bool under = r < -S, over = r > S - 1.0;           // both false for a NaN
    const bool none = isnan || under || over;                 // nothing is fed back
    const double t = none ? 0.0 : (r - y) * 0x1p24;           // exact: |r - y| <= 1/2
    const int32_t e = (int32_t)__builtin_rint(t) + (none ? 0 : D);
    r = under ? -S : (over ? S - 1.0 : r);
    r = isnan ? 0.0 : r;
    const int32_t q = (int32_t)r;
    acc.clipped += (under || over) ? 1 : 0;
    acc.nan += isnan ? 1 : 0;
    acc.q_min = acc.q_min < q ? acc.q_min : q;
    acc.q_max = acc.q_max > q ? acc.q_max : q;
    // the next word's tail from the history as it is: E_1 .. E_{K-1} become E_2 .. E_K
    int64_t tail = 0;
    PCM_SHAPE_UNROLL
    for (int k = K - 1; k >= 1; --k) {
        tail += (int64_t)pcm_shape_h(SHAPE, k + 1) * st.E[k - 1];
        st.E[k] = st.E[k - 1];
    }
    st.E[0] = e;
    st.tail = tail;
    return q;
}

// ---- the host loop: the definition word by word ----------------------------------------------
// x: n frames of `channels` interleaved words; out: exactly n channels bits / 8 bytes.
// max_e (may be null): the largest |E| fed back.
template <int BITS, bool DITHER, int SHAPE>
inline void pcm_shape_host_loop(const float* x, int channels, int64_t words, uint64_t k, unsigned char* out, PcmRec* rec,
                                int64_t* max_e) {
    const double S = (double)(1 << (BITS - 1));
    int64_t clipped = 0, nan = 0, big = 0;
    PcmAcc acc = pcm_acc_zero();
    PcmShapeState<SHAPE> st[2];
    pcm_shape_reset(st[0]);
    pcm_shape_reset(st[1]);
    for (int64_t w = 0; w < words; ++w) {
        PcmShapeState<SHAPE>& s = st[channels == 2 ? (w & 1) : 0];
        const int32_t D = DITHER ? pcm_dither_int(pcm_arg(k, (uint64_t)w)) : 0;
        const int32_t q = pcm_shape_word<SHAPE>(x[w], S, D, s, acc);
        clipped += acc.clipped; nan += acc.nan;
        acc.clipped = acc.nan = 0;
        const int64_t mag = s.E[0] < 0 ? -(int64_t)s.E[0] : (int64_t)s.E[0];
        big = big > mag ? big : mag;
        unsigned char* o = out + w * (BITS / 8);
        o[0] = (unsigned char)((uint32_t)q & 0xFF);
        o[1] = (unsigned char)(((uint32_t)q >> 8) & 0xFF);
        if (BITS == 24) o[2] = (unsigned char)(((uint32_t)q >> 16) & 0xFF);
    }
    pcm_finish(clipped, nan, acc.q_min, acc.q_max, words > 0, BITS, DITHER ? PCM_DITHER_TPDF : PCM_DITHER_NONE, rec);
    if (max_e) *max_e = big;
}

template <int SHAPE>
inline void pcm_shape_host_bits(const float* x, int channels, int64_t words, int bits, int dither, uint64_t k,
                                unsigned char* o, PcmRec* rec, int64_t* max_e) {
    if (bits == 16) {
        if (dither == PCM_DITHER_TPDF) pcm_shape_host_loop<16, true, SHAPE>(x, channels, words, k, o, rec, max_e);
        else pcm_shape_host_loop<16, false, SHAPE>(x, channels, words, k, o, rec, max_e);
    } else {
        if (dither == PCM_DITHER_TPDF) pcm_shape_host_loop<24, true, SHAPE>(x, channels, words, k, o, rec, max_e);
        else pcm_shape_host_loop<24, false, SHAPE>(x, channels, words, k, o, rec, max_e);
    }
}

inline void pcm_shape_host(const float* x, int channels, int64_t n, int bits, int dither, int shape, uint64_t seed,
                           uint64_t key, void* out, PcmRec* rec, int64_t* max_e = nullptr) {
    const uint64_t k = pcm_stream_key(seed, key);
    const int64_t words = n * channels;
    unsigned char* o = static_cast<unsigned char*>(out);
    if (shape == PCM_SHAPE_E3) pcm_shape_host_bits<PCM_SHAPE_E3>(x, channels, words, bits, dither, k, o, rec, max_e);
    else if (shape == PCM_SHAPE_LIPSHITZ5) pcm_shape_host_bits<PCM_SHAPE_LIPSHITZ5>(x, channels, words, bits, dither, k, o, rec, max_e);
    else pcm_shape_host_bits<PCM_SHAPE_F9>(x, channels, words, bits, dither, k, o, rec, max_e);
}
