// k_dynamics.hip — translation unit of the compressor's kernels (kernels_dynamics.h); the
// definition and the host reference are in dynamics.h.
#include "kernels_dynamics.h"
#include "launch.h"

static_assert(sizeof(DynRec) == 32 && sizeof(DynOpts) == 56, "DynRec is msg_dynamics_rec, DynOpts msg_dynamics_opts");
static_assert(DYN_T % 64 == 0 && DYN_T * DYN_C == DYN_TILE && DYN_C == 16, "whole waves, rows of 16 + 1 words");
static_assert(DYN_HOLD_MAX <= DYN_TILE && DYN_HOLD_MAX + DYN_TILE <= 2 * DYN_C * DYN_T,
              "the halo lies in the tile before, and a doubling pass holds halo + tile in 32 words per lane");

// a full hold halo takes more dynamic LDS than a kernel gets unasked
void dynamics_init_attrs() {
    const int lds = (int)dyn_lds_bytes(DYN_HOLD_MAX);
    (void)hipFuncSetAttribute((const void*)k_dynamics_tiles<1, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute((const void*)k_dynamics_tiles<1, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute((const void*)k_dynamics_tiles<2, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute((const void*)k_dynamics_tiles<2, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

template <int CH, bool HOLD>
static hipError_t dyn_launch(int n_sig, unsigned tiles, hipStream_t s, float* x, const int64_t* meta, const DynPar& par,
                             int64_t* carry, uint32_t* flag, int32_t* state, DynRec* rec, int64_t* halo) {
    hipError_t e;
    const size_t lds = dyn_lds_bytes(HOLD ? par.hold : 0);
    const int64_t n_tiles = tiles;
    // the launches order the three phases: sweep 1, the scan over tiles, sweep 2
    if (tiles > 0) {
        hipLaunchKernelGGL((k_dynamics_tiles<CH, HOLD, false>), dim3(tiles), dim3(DYN_T), lds, s, x, meta, n_sig, par, carry,
                           flag, state, rec, n_tiles, halo);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_dynamics_scan, dim3((unsigned)n_sig, 2), dim3(DYN_T), 0, s, meta, n_sig, par, carry, flag, state,
                       rec, n_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (tiles > 0)
        hipLaunchKernelGGL((k_dynamics_tiles<CH, HOLD, true>), dim3(tiles), dim3(DYN_T), lds, s, x, meta, n_sig, par, carry,
                           flag, state, rec, n_tiles, halo);
    return hipGetLastError();
}

hipError_t launch_dynamics(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                           const DynPar& par, int64_t* carry, uint32_t* flag, int32_t* state, void* rec, int64_t* halo) {
    DynRec* r = static_cast<DynRec*>(rec);
    if (par.hold > 0)
        return channels == 1 ? dyn_launch<1, true>(n_sig, tiles, s, x, meta, par, carry, flag, state, r, halo)
                             : dyn_launch<2, true>(n_sig, tiles, s, x, meta, par, carry, flag, state, r, halo);
    return channels == 1 ? dyn_launch<1, false>(n_sig, tiles, s, x, meta, par, carry, flag, state, r, halo)
                         : dyn_launch<2, false>(n_sig, tiles, s, x, meta, par, carry, flag, state, r, halo);
}
