// k_resample.hip — translation unit of the polyphase resampler (kernels_resample.h).
#include "kernels_resample.h"
#include "launch.h"

template <int DOWN>
static void dec_launch(int channels, unsigned tiles, const RsPlan& p, hipStream_t s, const float* x, float* y,
                       const int64_t* meta, int n_sig, const float* tab, int half, int K) {
    if (channels == 1)
        hipLaunchKernelGGL((k_resample_dec<DOWN, 1>), dim3(tiles), dim3(RS_DTILE / RS_RB), p.lds_bytes, s, x, y, meta,
                           n_sig, tab, p.taps, p.row, half, K);
    else
        hipLaunchKernelGGL((k_resample_dec<DOWN, 2>), dim3(tiles), dim3(RS_DTILE / RS_RB * 2), p.lds_bytes, s, x, y,
                           meta, n_sig, tab, p.taps, p.row, half, K);
}

hipError_t launch_resample(const RsPlan& p, int channels, unsigned tiles, hipStream_t s, const float* x, float* y,
                           const int64_t* meta, int n_sig, const float* tab, int up, int down, int64_t K) {
    const int half = (int)((K - 1) / 2);
    if (p.kind == 0) {
        if (down == 2) dec_launch<2>(channels, tiles, p, s, x, y, meta, n_sig, tab, half, (int)K);
        else if (down == 4) dec_launch<4>(channels, tiles, p, s, x, y, meta, n_sig, tab, half, (int)K);
        else dec_launch<8>(channels, tiles, p, s, x, y, meta, n_sig, tab, half, (int)K);
    } else if (channels == 1) {
        hipLaunchKernelGGL(k_resample_gen<1>, dim3(tiles), dim3(RS_LANES), p.lds_bytes, s, x, y, meta, n_sig, tab, up,
                           down, half, p.taps, p.lanes, p.step, p.span);
    } else {
        hipLaunchKernelGGL(k_resample_gen<2>, dim3(tiles), dim3(RS_LANES), p.lds_bytes, s, x, y, meta, n_sig, tab, up,
                           down, half, p.taps, p.lanes, p.step, p.span);
    }
    return hipGetLastError();
}
