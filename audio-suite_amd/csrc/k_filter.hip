// k_filter.hip — translation unit of the delivery filter's kernels (kernels_filter.h); the
// definition and the host reference are in filter.h.
#include "kernels_filter.h"
#include "launch.h"

static_assert(sizeof(FilterOpts) == 8 + 8 * 6 * 8, "FilterOpts is msg_filter_opts");
static_assert(FL_T % 64 == 0 && FL_T / 64 * 64 * FL_C == FL_TILE && FL_NS <= 64, "whole waves, the lane table's reach");

template <int CH>
static hipError_t fl_launch(int n_sig, unsigned tiles, hipStream_t s, float* x, const int64_t* meta, int S, int reverse,
                            const double* tab, double* state) {
    hipError_t e;
    // the launches order the three phases: sweep 1, the scan over tiles, sweep 2
    hipLaunchKernelGGL((k_filter_tiles<CH, false>), dim3(tiles), dim3(FL_T), 0, s, x, meta, n_sig, S, reverse, tab, state);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_filter_scan, dim3((unsigned)(n_sig * CH)), dim3(FL_NS), 0, s, meta, n_sig, CH, S, tab, state);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL((k_filter_tiles<CH, true>), dim3(tiles), dim3(FL_T), 0, s, x, meta, n_sig, S, reverse, tab, state);
    return hipGetLastError();
}

hipError_t launch_filter(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                         int n_sections, int reverse, const double* tab, double* state) {
    if (tiles == 0) return hipSuccess;
    return channels == 1 ? fl_launch<1>(n_sig, tiles, s, x, meta, n_sections, reverse, tab, state)
                         : fl_launch<2>(n_sig, tiles, s, x, meta, n_sections, reverse, tab, state);
}
