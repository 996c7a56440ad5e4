// k_limit.hip — translation unit of the look-ahead limiter's kernels (kernels_limit.h);
// the definition and the host reference are in limit.h.
#include "kernels_limit.h"
#include "launch.h"

static_assert(sizeof(LimitRec) == 32, "LimitRec is msg_limit_rec");
static_assert(LIM_ENV_TILE % 4 == 0 && LIM_ENV_ROW % 4 == 0, "a lane owns whole groups of four positions");

// the kernel also has 256 bytes of static LDS (the block-wide vote), so it asks for what the
// largest look-ahead needs and not for the whole 160 KiB
void limit_init_attrs() {
    const int lds = (int)lim_lds_bytes(LIM_L_MAX);
    (void)hipFuncSetAttribute((const void*)k_limit_apply<1, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute((const void*)k_limit_apply<2, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

template <int CH, int OS>
static void lim_env(unsigned tiles, hipStream_t s, const float* x, const int64_t* meta, int n_sig, const float* tab,
                    float c32, const void* tp_rec, float* rbuf, uint32_t* nanpart) {
    hipLaunchKernelGGL((k_limit_env<CH, OS>), dim3(tiles), dim3(LIM_ENV_T), 0, s, x, meta, n_sig, tab, c32,
                       static_cast<const TruePeakRec*>(tp_rec), rbuf, nanpart);
}

template <int CH>
static hipError_t lim_launch(int n_sig, int os, unsigned env_tiles, unsigned tiles, hipStream_t s, float* x,
                             const int64_t* meta, const float* tab, float c32, int L, const float* w, const void* tp_rec,
                             float* rbuf, uint32_t* nanpart, int32_t* state, void* part, void* rec) {
    if (env_tiles > 0) {
        if (os == 4) lim_env<CH, 4>(env_tiles, s, x, meta, n_sig, tab, c32, tp_rec, rbuf, nanpart);
        else if (os == 2) lim_env<CH, 2>(env_tiles, s, x, meta, n_sig, tab, c32, tp_rec, rbuf, nanpart);
        else lim_env<CH, 1>(env_tiles, s, x, meta, n_sig, tab, c32, tp_rec, rbuf, nanpart);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_limit_state, dim3((unsigned)n_sig), dim3(LIM_FT), 0, s, meta, n_sig, c32,
                       static_cast<const TruePeakRec*>(tp_rec), nanpart, state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (tiles > 0) {
        const size_t lds = lim_lds_bytes(L);
        if (lim_threads(L) == 256)
            hipLaunchKernelGGL((k_limit_apply<CH, 256>), dim3(tiles), dim3(256), lds, s, x, meta, n_sig,
                               reinterpret_cast<const float4*>(w), L, state, rbuf, static_cast<uint2*>(part));
        else
            hipLaunchKernelGGL((k_limit_apply<CH, 1024>), dim3(tiles), dim3(1024), lds, s, x, meta, n_sig,
                               reinterpret_cast<const float4*>(w), L, state, rbuf, static_cast<uint2*>(part));
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_limit_fin, dim3((unsigned)n_sig), dim3(LIM_FT), 0, s, meta, n_sig, L, state,
                       static_cast<const uint2*>(part), static_cast<LimitRec*>(rec));
    return hipGetLastError();
}

hipError_t launch_limit(int n_sig, int channels, int os, unsigned env_tiles, unsigned tiles, hipStream_t s, float* x,
                        const int64_t* meta, const float* tab, float c32, int L, const float* w, const void* tp_rec,
                        float* rbuf, uint32_t* nanpart, int32_t* state, void* part, void* rec) {
    return channels == 1 ? lim_launch<1>(n_sig, os, env_tiles, tiles, s, x, meta, tab, c32, L, w, tp_rec, rbuf, nanpart,
                                         state, part, rec)
                         : lim_launch<2>(n_sig, os, env_tiles, tiles, s, x, meta, tab, c32, L, w, tp_rec, rbuf, nanpart,
                                         state, part, rec);
}
