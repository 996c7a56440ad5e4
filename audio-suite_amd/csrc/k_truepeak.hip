// k_truepeak.hip — translation unit of the BS.1770 true-peak kernels (kernels_truepeak.h);
// the definition and the host reference are in truepeak.h.
#include "kernels_truepeak.h"
#include "launch.h"

static_assert(sizeof(TruePeakRec) == 40, "TruePeakRec is msg_truepeak_rec");
static_assert(TP_TILE % (4 * TP_T) == 0 && TP_ROW % 4 == 0, "a lane owns whole groups of four positions");

template <int CH, int OS>
static hipError_t tp_launch(int n_sig, unsigned tiles, hipStream_t s, const float* x, const int64_t* meta,
                            const float* tab, void* part, void* rec) {
    if (tiles > 0) {
        hipLaunchKernelGGL((k_truepeak<CH, OS>), dim3(tiles), dim3(TP_T), 0, s, x, meta, n_sig, tab,
                           static_cast<uint2*>(part));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_truepeak_fin, dim3((unsigned)n_sig), dim3(TP_FT), 0, s, meta, n_sig,
                       static_cast<const uint2*>(part), OS, static_cast<TruePeakRec*>(rec));
    return hipGetLastError();
}

template <int CH>
static hipError_t tp_launch_os(int os, int n_sig, unsigned tiles, hipStream_t s, const float* x, const int64_t* meta,
                               const float* tab, void* part, void* rec) {
    return os == 4   ? tp_launch<CH, 4>(n_sig, tiles, s, x, meta, tab, part, rec)
           : os == 2 ? tp_launch<CH, 2>(n_sig, tiles, s, x, meta, tab, part, rec)
                     : tp_launch<CH, 1>(n_sig, tiles, s, x, meta, tab, part, rec);
}

hipError_t launch_truepeak(int n_sig, int channels, int os, unsigned tiles, hipStream_t s, const float* x,
                           const int64_t* meta, const float* tab, void* part, void* rec) {
    return channels == 1 ? tp_launch_os<1>(os, n_sig, tiles, s, x, meta, tab, part, rec)
                         : tp_launch_os<2>(os, n_sig, tiles, s, x, meta, tab, part, rec);
}

hipError_t launch_truepeak_gain(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                                void* loud_rec, void* tp_rec, double target, double ceil_tp, double ceil_pk) {
    const dim3 grid(tiles > 0 ? tiles : 1u);
    if (channels == 1)
        hipLaunchKernelGGL(k_truepeak_gain<1>, grid, dim3(TP_T), 0, s, x, meta, n_sig, static_cast<LoudRec*>(loud_rec),
                           static_cast<TruePeakRec*>(tp_rec), target, ceil_tp, ceil_pk);
    else
        hipLaunchKernelGGL(k_truepeak_gain<2>, grid, dim3(TP_T), 0, s, x, meta, n_sig, static_cast<LoudRec*>(loud_rec),
                           static_cast<TruePeakRec*>(tp_rec), target, ceil_tp, ceil_pk);
    return hipGetLastError();
}
