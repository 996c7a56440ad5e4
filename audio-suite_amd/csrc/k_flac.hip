// k_flac.hip — translation unit of the FLAC encoder's kernels (kernels_flac.h); the definition and
// the host loop are in flac.h.
#include "kernels_flac.h"
#include "launch.h"

static_assert(sizeof(FlacRec) == 88 && sizeof(FlacPlan) == 168 && sizeof(FlacBest) == 80, "FlacRec is msg_flac_rec; the plan's layout");
static_assert(FLAC_T % 64 == 0 && FLAC_T * FLAC_C == FLAC_MAXB && FLAC_T >= 128, "whole waves, chunks of 16, a lane per partition entry");

template <int CH>
static hipError_t flac_launch(int n_sig, int bits, int B, int sr, bool md5, unsigned tiles, hipStream_t s, const uint8_t* pcm,
                              const int64_t* meta, FlacPlan* plan, int64_t* pre, FlacRec* rec, uint8_t* out, int64_t out_bytes) {
    hipError_t e;
    // the launches order the phases: the plan sweep, the two scans, the pack sweep, the MD5
    if (tiles > 0) {
        hipLaunchKernelGGL(k_flac_plan<CH>, dim3(tiles), dim3(FLAC_T), 0, s, pcm, meta, n_sig, bits, B, sr, plan);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_flac_scan, dim3((unsigned)n_sig), dim3(FLAC_T), 0, s, meta, n_sig, CH, plan, pre, rec);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_flac_offsets, dim3(1), dim3(FLAC_T), 0, s, n_sig, rec);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (tiles > 0) {
        hipLaunchKernelGGL(k_flac_pack<CH>, dim3(tiles), dim3(FLAC_T), 0, s, pcm, meta, n_sig, bits, B, sr, plan, pre, rec, out,
                           out_bytes);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (md5) hipLaunchKernelGGL(k_flac_md5, dim3((unsigned)n_sig), dim3(64), 0, s, pcm, meta, n_sig, CH * (bits / 8), rec);
    return hipGetLastError();
}

hipError_t launch_flac(int n_sig, int channels, int bits, int block, int sr, bool md5, unsigned tiles, hipStream_t s,
                       const void* pcm, const int64_t* meta, void* plan, int64_t* pre, void* rec, void* out, int64_t out_bytes) {
    const uint8_t* x = static_cast<const uint8_t*>(pcm);
    FlacPlan* pl = static_cast<FlacPlan*>(plan);
    FlacRec* r = static_cast<FlacRec*>(rec);
    uint8_t* o = static_cast<uint8_t*>(out);
    return channels == 1 ? flac_launch<1>(n_sig, bits, block, sr, md5, tiles, s, x, meta, pl, pre, r, o, out_bytes)
                         : flac_launch<2>(n_sig, bits, block, sr, md5, tiles, s, x, meta, pl, pre, r, o, out_bytes);
}
