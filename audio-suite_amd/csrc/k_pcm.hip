// k_pcm.hip — translation unit of the PCM quantiser's kernels (kernels_pcm.h); the
// definition and the host loop are in pcm.h.
#include "kernels_pcm.h"
#include "launch.h"

static_assert(sizeof(PcmRec) == 32, "PcmRec is msg_pcm_rec");
static_assert(PCM_TILE == (PCM_T / 64) * PCM_TURNS * 256, "a wave's turns of four words per lane fill the tile");
static_assert(PCM_TILE * 2 % 16 == 0 && PCM_TILE * 3 % 16 == 0, "every tile's output starts 16-byte aligned");

template <int BITS, int DITHER>
static hipError_t pcm_launch(int n_sig, int channels, unsigned tiles, hipStream_t s, const float* x, const int64_t* meta,
                             void* out, void* part, void* rec) {
    if (tiles > 0) {
        hipLaunchKernelGGL((k_pcm<BITS, DITHER>), dim3(tiles), dim3(PCM_T), 0, s, x, channels, meta, n_sig,
                           static_cast<unsigned char*>(out), static_cast<int4*>(part));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_pcm_fin, dim3((unsigned)n_sig), dim3(PCM_FT), 0, s, meta, n_sig, static_cast<const int4*>(part),
                       BITS, DITHER, static_cast<PcmRec*>(rec));
    return hipGetLastError();
}

hipError_t launch_pcm(int n_sig, int channels, int bits, int dither, unsigned tiles, hipStream_t s, const float* x,
                      const int64_t* meta, void* out, void* part, void* rec) {
    if (bits == 16)
        return dither == PCM_DITHER_TPDF ? pcm_launch<16, 1>(n_sig, channels, tiles, s, x, meta, out, part, rec)
                                         : pcm_launch<16, 0>(n_sig, channels, tiles, s, x, meta, out, part, rec);
    return dither == PCM_DITHER_TPDF ? pcm_launch<24, 1>(n_sig, channels, tiles, s, x, meta, out, part, rec)
                                     : pcm_launch<24, 0>(n_sig, channels, tiles, s, x, meta, out, part, rec);
}
