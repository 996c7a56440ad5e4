// k_gate.hip — translation unit of the gate's kernels (kernels_gate.h); the definition and the
// host reference are in gate.h.
#include "kernels_gate.h"
#include "launch.h"

static_assert(sizeof(GateRec) == 48 && sizeof(GateOpts) == 56, "GateRec is msg_gate_rec, GateOpts msg_gate_opts");
static_assert(DYN_T % 64 == 0 && DYN_T * DYN_C == DYN_TILE && DYN_C == 16, "whole waves, rows of 16 + 1 words, 16-bit masks");

template <int CH>
static hipError_t gate_launch(int n_sig, unsigned tiles, hipStream_t s, float* x, const int64_t* meta, const GatePar& par,
                              int64_t* carry, int64_t* trans, uint32_t* flag, int32_t* state, GateRec* rec) {
    hipError_t e;
    const int64_t n_tiles = tiles;
    // the launches order the phases: the state sweep and its scan, sweep 1, the envelope scan, sweep 2
    if (tiles > 0 && !par.local) {
        hipLaunchKernelGGL((k_gate_tiles<CH, GATE_SWEEP_STATE>), dim3(tiles), dim3(DYN_T), 0, s, x, meta, n_sig, par, carry,
                           trans, flag, state, rec, n_tiles);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_gate_scan_state, dim3((unsigned)n_sig), dim3(DYN_T), 0, s, meta, n_sig, par, trans, n_tiles);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (tiles > 0) {
        hipLaunchKernelGGL((k_gate_tiles<CH, GATE_SWEEP_SUM>), dim3(tiles), dim3(DYN_T), 0, s, x, meta, n_sig, par, carry,
                           trans, flag, state, rec, n_tiles);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_gate_scan_env, dim3((unsigned)n_sig, 2), dim3(DYN_T), 0, s, meta, n_sig, par, carry, flag, state, rec,
                       n_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (tiles > 0)
        hipLaunchKernelGGL((k_gate_tiles<CH, GATE_SWEEP_APPLY>), dim3(tiles), dim3(DYN_T), 0, s, x, meta, n_sig, par, carry,
                           trans, flag, state, rec, n_tiles);
    return hipGetLastError();
}

hipError_t launch_gate(int n_sig, int channels, unsigned tiles, hipStream_t s, float* x, const int64_t* meta,
                       const GatePar& par, int64_t* carry, int64_t* trans, uint32_t* flag, int32_t* state, void* rec) {
    GateRec* r = static_cast<GateRec*>(rec);
    return channels == 1 ? gate_launch<1>(n_sig, tiles, s, x, meta, par, carry, trans, flag, state, r)
                         : gate_launch<2>(n_sig, tiles, s, x, meta, par, carry, trans, flag, state, r);
}
