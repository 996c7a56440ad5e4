// k_loudness.hip — translation unit of the BS.1770 loudness kernels (kernels_loudness.h)
// and of the loudness-range kernels on top of them (kernels_lrange.h); the definitions
// and the host references are in loudness.h and lrange.h.
#include "kernels_loudness.h"
#include "kernels_lrange.h"
#include "launch.h"

static_assert(sizeof(LoudRec) == 40, "LoudRec is msg_loudness_rec");
static_assert(sizeof(LRangeRec) == 96, "LRangeRec is msg_lrange_rec");

// the two sweeps and the scan between them: one energy and one peak per tile in part
template <int CH>
static hipError_t loud_sweeps(int n_sig, unsigned tiles, hipStream_t s, const float* x, const int64_t* meta,
                              int64_t hop, int tph, const double* tab, double* state, double* part) {
    if (tiles > 0) {
        hipLaunchKernelGGL((k_loud_tiles<CH, false>), dim3(tiles), dim3(LD_T), 0, s, x, meta, n_sig, hop, tph, tab,
                           state, part);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_loud_scan, dim3((unsigned)((n_sig * CH + 63) / 64)), dim3(64), 0, s, meta, n_sig, CH, hop,
                           tph, tab, state);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_loud_tiles<CH, true>), dim3(tiles), dim3(LD_T), 0, s, x, meta, n_sig, hop, tph, tab,
                           state, part);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

static hipError_t loud_measure(int n_sig, int channels, unsigned tiles, hipStream_t s, const float* x,
                               const int64_t* meta, int64_t hop, int tph, const double* tab, double* state,
                               double* part, void* rec) {
    const hipError_t e = channels == 1 ? loud_sweeps<1>(n_sig, tiles, s, x, meta, hop, tph, tab, state, part)
                                       : loud_sweeps<2>(n_sig, tiles, s, x, meta, hop, tph, tab, state, part);
    if (e != hipSuccess || !rec) return e;
    hipLaunchKernelGGL(k_loud_gate, dim3((unsigned)n_sig), dim3(LD_GT), 0, s, meta, n_sig, hop, tph, part,
                       static_cast<LoudRec*>(rec));
    return hipGetLastError();
}

hipError_t launch_loudness(int n_sig, int channels, unsigned tiles, hipStream_t s, const float* x, const int64_t* meta,
                           int64_t hop, const double* tab, double* state, double* part, void* rec) {
    return loud_measure(n_sig, channels, tiles, s, x, meta, hop, (int)ld_tiles_per_hop(hop), tab, state, part, rec);
}

hipError_t launch_loudness_range(int n_sig, int channels, unsigned tiles, hipStream_t s, const float* x,
                                 const int64_t* meta, int64_t hop, const double* tab, double* state, double* part,
                                 void* loud_rec, double* hops, double* win, void* range_rec) {
    const int tph = (int)ld_tiles_per_hop(hop);
    hipError_t e = loud_measure(n_sig, channels, tiles, s, x, meta, hop, tph, tab, state, part, loud_rec);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lrange_hops, dim3((unsigned)n_sig), dim3(LR_T), 0, s, meta, n_sig, hop, tph, part, hops);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lrange, dim3((unsigned)n_sig), dim3(LR_T), 0, s, meta, n_sig, hop, hops, win,
                       static_cast<LRangeRec*>(range_rec));
    return hipGetLastError();
}

hipError_t launch_loudness_gain(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                                void* rec, double target, double ceiling) {
    const dim3 grid(tiles > 0 ? tiles : 1u);
    if (channels == 1)
        hipLaunchKernelGGL(k_loud_gain<1>, grid, dim3(LD_T), 0, s, x, meta, n_sig, static_cast<LoudRec*>(rec), target,
                           ceiling);
    else
        hipLaunchKernelGGL(k_loud_gain<2>, grid, dim3(LD_T), 0, s, x, meta, n_sig, static_cast<LoudRec*>(rec), target,
                           ceiling);
    return hipGetLastError();
}
