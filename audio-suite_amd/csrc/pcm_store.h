// pcm_store.h — the packed-word store the PCM quantisers' kernels share (kernels_pcm.h,
// kernels_pcm_shape.h).
#pragma once
#include <hip/hip_runtime.h>
#include "msg_common.h"

// The first m of a lane's four packed words stored at dst (4-byte aligned; 8-byte at 16
// bits).  m = 4: one dwordx2 or dwordx3.  m < 4, the signal's end: whole dwords, then
// its last partial dword in sub-dword stores, and not a byte more.
template <int BITS>
MSG_DEV void pcm_store4(const uint32_t pk[3], int m, unsigned char* __restrict__ dst) {
    typedef uint32_t v2u __attribute__((ext_vector_type(2)));
    struct alignas(4) v3u { uint32_t a, b, c; };              // 12 bytes at a 4-byte address: one dwordx3
    if (m == 4) {
        if (BITS == 16) *reinterpret_cast<v2u*>(dst) = v2u{pk[0], pk[1]};
        else *reinterpret_cast<v3u*>(dst) = v3u{pk[0], pk[1], pk[2]};
        return;
    }
    const int nb = m * (BITS / 8), full = nb >> 2;
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (j < full) reinterpret_cast<uint32_t*>(dst)[j] = pk[j];
    uint32_t last = full == 0 ? pk[0] : (full == 1 ? pk[1] : pk[2]);
    unsigned char* tail = dst + 4 * full;
    if (nb & 2) { *reinterpret_cast<uint16_t*>(tail) = (uint16_t)last; tail += 2; last >>= 16; }
    if (nb & 1) *tail = (unsigned char)last;
}
