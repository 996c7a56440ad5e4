// k_edges.hip — translation unit of the edges pass's kernels (kernels_edges.h); the
// definition and the host reference are in edges.h.
#include "kernels_edges.h"
#include "launch.h"

static_assert(sizeof(EdgesRec) == 64, "EdgesRec is msg_edges_rec");
static_assert(EDG_T % 64 == 0 && EDG_APPLY_TILE % EDG_T == 0 && EDG_TILE % 4 == 0, "whole waves, whole rounds, whole pieces");

template <int CH>
static hipError_t edg_launch(int n_sig, unsigned find_tiles, unsigned apply_tiles, hipStream_t s, float* x,
                             const int64_t* meta, const EdgesPar& par, EdgesRec* rec) {
    const unsigned sig_blocks = (unsigned)((n_sig + EDG_T - 1) / EDG_T);
    hipError_t e;
    if (par.sides) {
        hipLaunchKernelGGL(k_edges_init, dim3(sig_blocks), dim3(EDG_T), 0, s, n_sig, rec);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (find_tiles > 0) {
            hipLaunchKernelGGL((k_edges_find<CH>), dim3(find_tiles), dim3(EDG_T), 0, s, x, meta, n_sig, par.thr, rec);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(k_edges_span, dim3(sig_blocks), dim3(EDG_T), 0, s, meta, n_sig, par, rec);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (apply_tiles > 0) hipLaunchKernelGGL((k_edges_apply<CH>), dim3(apply_tiles), dim3(EDG_T), 0, s, x, meta, n_sig, par, rec);
    return hipGetLastError();
}

hipError_t launch_edges(int n_sig, int channels, unsigned find_tiles, unsigned apply_tiles, hipStream_t s, float* x,
                        const int64_t* meta, const EdgesPar& par, void* rec) {
    return channels == 1 ? edg_launch<1>(n_sig, find_tiles, apply_tiles, s, x, meta, par, static_cast<EdgesRec*>(rec))
                         : edg_launch<2>(n_sig, find_tiles, apply_tiles, s, x, meta, par, static_cast<EdgesRec*>(rec));
}
