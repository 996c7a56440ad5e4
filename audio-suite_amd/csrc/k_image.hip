// k_image.hip — translation unit of the stereo meter's and the stereo image's kernels
// (kernels_image.h); the definition and the host references are in image.h.
#include "kernels_image.h"
#include "launch.h"

static_assert(sizeof(ImageRec) == 64, "ImageRec is msg_stereo_rec");
static_assert(IMG_T % 64 == 0 && IMG_TILE == IMG_T * IMG_PER * 2, "whole waves, two frames per piece");

hipError_t launch_image_meter(int n_sig, unsigned tiles, hipStream_t s, const float* x, const int64_t* meta, int64_t hop,
                              double* part, void* rec) {
    const int tph = (int)img_tiles_per_hop(hop);
    if (tiles > 0) {
        hipLaunchKernelGGL(k_image_sums, dim3(tiles), dim3(IMG_T), 0, s, x, meta, n_sig, hop, tph, part);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_image_record, dim3((unsigned)n_sig), dim3(IMG_GT), 0, s, meta, n_sig, hop, tph, part,
                       static_cast<ImageRec*>(rec));
    return hipGetLastError();
}

hipError_t launch_image_apply(int n_sig, unsigned tiles, hipStream_t s, float* x, const int64_t* meta, const float* m,
                              const float* fold, float* y, const void* rec) {
    if (tiles == 0) return hipSuccess;
    const ImageRec* r = static_cast<const ImageRec*>(rec);
    if (fold)
        hipLaunchKernelGGL(k_image_apply<true>, dim3(tiles), dim3(IMG_T), 0, s, x, meta, n_sig, fold[0], fold[1], 0.f, 0.f,
                           y, r);
    else
        hipLaunchKernelGGL(k_image_apply<false>, dim3(tiles), dim3(IMG_T), 0, s, x, meta, n_sig, m[0], m[1], m[2], m[3],
                           y, r);
    return hipGetLastError();
}
