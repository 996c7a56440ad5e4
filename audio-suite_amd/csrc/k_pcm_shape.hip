// k_pcm_shape.hip — translation unit of the noise-shaped quantiser's kernel
// (kernels_pcm_shape.h); the definition and the host loop are in pcm_shape.h.
#include "kernels_pcm_shape.h"
#include "launch.h"

static_assert(PCM_SHAPE_CHUNK % 4 == 0 && PCM_SHAPE_T == 64, "whole pieces per chunk, one wave per workgroup");
static_assert(pcm_shape_taps(PCM_SHAPE_F9) == PCM_SHAPE_KMAX, "the longest shape");

// |A| < 2^46 and |F + D| < 2^30 from |E| < 1.5 2^24 (pcm_shape.h)
template <int SHAPE>
constexpr int64_t pcm_shape_abs_sum() {
    int64_t s = 0;
    for (int k = 1; k <= pcm_shape_taps(SHAPE); ++k) s += pcm_shape_h(SHAPE, k) < 0 ? -pcm_shape_h(SHAPE, k) : pcm_shape_h(SHAPE, k);
    return s;
}
constexpr int64_t PCM_SHAPE_E_MAX = 3 * (1ll << 23);
static_assert(pcm_shape_abs_sum<PCM_SHAPE_E3>() * PCM_SHAPE_E_MAX < (1ll << 46), "A fits");
static_assert(pcm_shape_abs_sum<PCM_SHAPE_LIPSHITZ5>() * PCM_SHAPE_E_MAX < (1ll << 46), "A fits");
static_assert(pcm_shape_abs_sum<PCM_SHAPE_F9>() * PCM_SHAPE_E_MAX < (1ll << 46), "A fits");
static_assert(((pcm_shape_abs_sum<PCM_SHAPE_F9>() * PCM_SHAPE_E_MAX + 32768) >> 16) + (1ll << 24) < (1ll << 30), "F + D fits");

template <int BITS, int DITHER, int SHAPE>
static hipError_t pcm_shape_launch(int n_sig, int channels, hipStream_t s, const float* x, const int64_t* meta, void* out,
                                   void* rec) {
    const dim3 grid((unsigned)((n_sig + PCM_SHAPE_T - 1) / PCM_SHAPE_T)), block(PCM_SHAPE_T);
    if (channels == 2)
        hipLaunchKernelGGL((k_pcm_shape<BITS, DITHER, SHAPE, 2>), grid, block, 0, s, x, meta, n_sig,
                           static_cast<unsigned char*>(out), static_cast<PcmRec*>(rec));
    else
        hipLaunchKernelGGL((k_pcm_shape<BITS, DITHER, SHAPE, 1>), grid, block, 0, s, x, meta, n_sig,
                           static_cast<unsigned char*>(out), static_cast<PcmRec*>(rec));
    return hipGetLastError();
}

template <int BITS, int DITHER>
static hipError_t pcm_shape_pick(int shape, int n_sig, int channels, hipStream_t s, const float* x, const int64_t* meta,
                                 void* out, void* rec) {
    if (shape == PCM_SHAPE_E3) return pcm_shape_launch<BITS, DITHER, PCM_SHAPE_E3>(n_sig, channels, s, x, meta, out, rec);
    if (shape == PCM_SHAPE_LIPSHITZ5)
        return pcm_shape_launch<BITS, DITHER, PCM_SHAPE_LIPSHITZ5>(n_sig, channels, s, x, meta, out, rec);
    return pcm_shape_launch<BITS, DITHER, PCM_SHAPE_F9>(n_sig, channels, s, x, meta, out, rec);
}

hipError_t launch_pcm_shape(int n_sig, int channels, int bits, int dither, int shape, hipStream_t s, const float* x,
                            const int64_t* meta, void* out, void* rec) {
    if (bits == 16)
        return dither == PCM_DITHER_TPDF ? pcm_shape_pick<16, 1>(shape, n_sig, channels, s, x, meta, out, rec)
                                         : pcm_shape_pick<16, 0>(shape, n_sig, channels, s, x, meta, out, rec);
    return dither == PCM_DITHER_TPDF ? pcm_shape_pick<24, 1>(shape, n_sig, channels, s, x, meta, out, rec)
                                     : pcm_shape_pick<24, 0>(shape, n_sig, channels, s, x, meta, out, rec);
}
