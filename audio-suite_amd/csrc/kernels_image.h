// kernels_image.h — the device side of msg_stereo_meter / msg_stereo (TU k_image.hip).  The
// definition, the tile shapes and the record are in image.h; DESIGN.md "4k. Stereo".
//
//   k_image_sums      one workgroup per tile of IMG_TILE frames of one hop (or of the tail):
//                     16-byte pieces (img_piece, sig_piece for whole frames), one read of the samples; lane t takes
//                     the tile's frame pairs t, t + IMG_T, ... and adds L L, R R and L R in
//                     float64 in that order, the wave folds by the xor butterfly, the waves
//                     fold in order, and the tile's three sums are written
//   k_image_record    one wave per signal: lanes 0 .. 2 add one sum each over the hops in
//                     order and the tail; lane i takes blocks i, i + 64, ... for the smallest
//                     kept correlation and its first index; lane 0 writes the record
//   k_image_apply     one workgroup per tile of IMG_TILE frames: the 2 x 2 matrix in place, or
//                     the fold row into a mono buffer; the matrix's second column is negated
//                     for a signal whose record says corr < 0
//
// meta (int64): offsets, frames, n_sig + 1 first tiles, then (apply) the fold's output offsets.
// A stereo buffer is 8-byte aligned (sig_aligned), so a tile's first float lies 0 or 2 floats
// past a 16-byte address and a piece always holds two whole frames.
#pragma once
#include <hip/hip_runtime.h>
#include "image.h"
#include "sig_tiles.h"

struct ImgTile {
    int p;          // signal
    int lt;         // frames of the tile (1 .. IMG_TILE)
    int64_t f0;     // first frame, from the signal's base
};
// the hop cut of loudness.h: tile tt of a signal is tile tt % tph of hop tt / tph, the tail being the last hop
MSG_DEV ImgTile img_locate(const int64_t* __restrict__ meta, int n_sig, int64_t hop, int tph, int64_t tile) {
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    ImgTile t;
    t.p = sig_owner(tile_base, n_sig, tile);
    const int64_t n = meta[n_sig + t.p], tt = tile - tile_base[t.p];
    const int64_t h = tt / tph, ti = tt - h * tph;
    const int64_t hl = n - h * hop < hop ? n - h * hop : hop;
    t.f0 = h * hop + ti * IMG_TILE;
    const int64_t left = hl - ti * IMG_TILE;
    t.lt = (int)(left < IMG_TILE ? left : IMG_TILE);
    return t;
}

// floats past a 16-byte address of float gbase of x: 0 or 2 for a stereo frame
MSG_DEV int img_shift(const float* x, int64_t gbase) {
    return (int)(((int64_t)(reinterpret_cast<uintptr_t>(x) >> 2) + gbase) & 3);
}

typedef float img_v2f __attribute__((ext_vector_type(2)));

// sig_piece for whole frames: the floats e0 .. e0 + 3 (e0 even, e0 >= -2) of a span of E floats (E even).
// A piece inside the span is one 16-byte load; an edge piece loads the one frame that lies inside
// as 8 bytes; floats outside read as zero and are never loaded.  Not pinned: the caller pins
// (sig_pin) once its loads are issued.
MSG_DEV float4 img_piece(const float* __restrict__ x, int64_t gbase, int e0, int E) {
    const float* q = x + gbase + e0;
    if (e0 >= 0 && e0 + 4 <= E) return *reinterpret_cast<const float4*>(q);
    img_v2f lo = {0.f, 0.f}, hi = {0.f, 0.f};
    if (e0 >= 0 && e0 < E) lo = *reinterpret_cast<const img_v2f*>(q);
    if (e0 + 2 < E) hi = *reinterpret_cast<const img_v2f*>(q + 2);
    return float4{lo.x, lo.y, hi.x, hi.y};
}

// the frame pair at local float e0 (a multiple of 4, 0 <= e0 < E) of a span whose first float lies a
// floats past a 16-byte address: one 16-byte piece, or, a = 2, the 8-byte halves of the two pieces
// the pair straddles (the same bytes from HBM, each once)
MSG_DEV float4 img_pair(const float* __restrict__ x, int64_t gbase, int e0, int a, int E) {
    if (a == 0) return img_piece(x, gbase, e0, E);
    const float* q = x + gbase + e0;
    const img_v2f lo = *reinterpret_cast<const img_v2f*>(q);
    img_v2f hi = {0.f, 0.f};
    if (e0 + 2 < E) hi = *reinterpret_cast<const img_v2f*>(q + 2);
    return float4{lo.x, lo.y, hi.x, hi.y};
}

__global__ void __launch_bounds__(IMG_T)
k_image_sums(const float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, int64_t hop, int tph,
             double* __restrict__ part) {
    __shared__ double red[IMG_T / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const ImgTile t = img_locate(meta, n_sig, hop, tph, tile);
    const int64_t gbase = (meta[t.p] + t.f0) * 2;        // 64-bit from the buffer's base
    const int E = t.lt * 2;
    const int a = img_shift(x, gbase);

    float4 v[IMG_PER];                                   // all loads in flight first
#pragma unroll
    for (int k = 0; k < IMG_PER; ++k) {
        const int e0 = 4 * (tid + k * IMG_T);
        v[k] = e0 < E ? img_pair(x, gbase, e0, a, E) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < IMG_PER; ++k) sig_pin(v[k]);
    double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < IMG_PER; ++k) {                  // floats past the tile are zeros and add +0
        const double l0 = (double)v[k].x, r0 = (double)v[k].y, l1 = (double)v[k].z, r1 = (double)v[k].w;
        s[0] += l0 * l0; s[1] += r0 * r0; s[2] += l0 * r0;
        s[0] += l1 * l1; s[1] += r1 * r1; s[2] += l1 * r1;
    }
    // fixed order: xor-butterfly in each wave, then the waves in order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += __shfl_xor(s[q], o, 64);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 3; ++q) red[wave][q] = s[q];
    __syncthreads();
    if (tid < 3) {
        double r = red[0][tid];
        for (int w = 1; w < IMG_T / 64; ++w) r += red[w][tid];
        part[3 * tile + tid] = r;
    }
}

// sum q of hop h of a signal whose tiles start at t0: its tiles in order
MSG_DEV double img_hop_sum(const double* __restrict__ part, int64_t t0, int tph, int64_t h, int q) {
    const int64_t tb = t0 + h * tph;
    double a = part[3 * tb + q];
    for (int i = 1; i < tph; ++i) a += part[3 * (tb + i) + q];
    return a;
}

__global__ void __launch_bounds__(IMG_GT)
k_image_record(const int64_t* __restrict__ meta, int n_sig, int64_t hop, int tph, const double* __restrict__ part,
               ImageRec* __restrict__ rec) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t n = meta[n_sig + p], t0 = tile_base[p], t1 = tile_base[p + 1];
    const int64_t hops = n / hop, nb = img_blocks(n, hop);

    // the whole-signal sums: lane q adds sum q over the hops in order, then the tail's tiles in order
    double w = 0.0;
    if (lane < 3) {
        for (int64_t h = 0; h < hops; ++h) w += img_hop_sum(part, t0, tph, h, lane);
        const int64_t tt = t0 + hops * tph;
        if (tt < t1) {
            double a = part[3 * tt + lane];
            for (int64_t i = tt + 1; i < t1; ++i) a += part[3 * i + lane];
            w += a;
        }
    }
    const double sll = __shfl(w, 0, 64), srr = __shfl(w, 1, 64), slr = __shfl(w, 2, 64);

    // the smallest kept block correlation and its first index
    constexpr int64_t NONE = INT64_MAX;
    double best = __builtin_inf();
    int64_t at = NONE, kept = 0;
    for (int64_t j = lane; j < nb; j += IMG_GT) {
        double b[3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
            b[q] = ((img_hop_sum(part, t0, tph, j, q) + img_hop_sum(part, t0, tph, j + 1, q)) +
                    img_hop_sum(part, t0, tph, j + 2, q)) + img_hop_sum(part, t0, tph, j + 3, q);
        if (!img_kept(b[0], b[1], hop)) continue;
        ++kept;
        const double rho = b[2] / sqrt(b[0] * b[1]);
        if (at == NONE || rho < best) { best = rho; at = j; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int64_t oa = (int64_t)sig_shfl64((uint64_t)at, o);
        kept += (int64_t)sig_shfl64((uint64_t)kept, o);
        if (oa != NONE && (at == NONE || ob < best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    if (lane == 0) {
        ImageRec r;
        r.sll = sll;
        r.srr = srr;
        r.slr = slr;
        r.corr = img_corr(sll, srr, slr);
        r.corr_min = at == NONE ? r.corr : best;
        r.corr_min_block = at == NONE ? -1.0 : (double)at;
        r.blocks_kept = (double)kept;
        r.blocks = (double)nb;
        rec[p] = r;
    }
}

// one 16-byte piece of a tile: the floats e0 .. e0 + 3 of its E, two frames, either of which may lie outside
template <bool FOLD>
MSG_DEV void img_put(float* __restrict__ x, int64_t gbase, float* __restrict__ y, int64_t ybase, int e0, int E,
                     const float4 v, const float (&m)[4]) {
    typedef img_v2f v2f;
    const bool first = e0 >= 0, second = e0 + 2 < E;       // e0 >= -2 and e0 < E
    if (FOLD) {
        const float o0 = img_mix(m[0], v.x, m[1], v.y), o1 = img_mix(m[0], v.z, m[1], v.w);
        float* q = y + ybase + (e0 >> 1);                  // e0 = -2: frame -1, never stored
        if (first && second && !(reinterpret_cast<uintptr_t>(q) & 7)) {
            *reinterpret_cast<v2f*>(q) = v2f{o0, o1};
        } else {
            if (first) q[0] = o0;
            if (second) q[1] = o1;
        }
    } else {
        float4 o;
        o.x = img_mix(m[0], v.x, m[1], v.y);
        o.y = img_mix(m[2], v.x, m[3], v.y);
        o.z = img_mix(m[0], v.z, m[1], v.w);
        o.w = img_mix(m[2], v.z, m[3], v.w);
        float* q = x + gbase + e0;
        if (first && second) {
            *reinterpret_cast<float4*>(q) = o;
        } else {
            if (first) *reinterpret_cast<v2f*>(q) = v2f{o.x, o.y};
            if (second) *reinterpret_cast<v2f*>(q + 2) = v2f{o.z, o.w};
        }
    }
}

// m: m00 m01 m10 m11, or (FOLD) f0 f1 and two words not read
template <bool FOLD>
__global__ void __launch_bounds__(IMG_T)
k_image_apply(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, float m0, float m1, float m2, float m3,
              float* __restrict__ y, const ImageRec* __restrict__ rec) {
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int p = sig_owner(tile_base, n_sig, tile);
    const int64_t off = meta[p], n = meta[n_sig + p];
    const int64_t f0 = (tile - tile_base[p]) * IMG_TILE;           // f0 < n
    const int64_t left = n - f0;
    const int E = (int)(left < IMG_TILE ? left : IMG_TILE) * 2;    // the tile's floats
    const int64_t gbase = (off + f0) * 2;
    const int64_t ybase = FOLD ? meta[3 * (int64_t)n_sig + 1 + p] + f0 : 0;
    const int a = img_shift(x, gbase);
    const bool flip = rec && rec[p].corr < 0.0;
    const float m[4] = {m0, flip ? -m1 : m1, m2, flip ? -m3 : m3};

    // pieces at 16-byte addresses: piece c holds the floats 4 c - a .. 4 c - a + 3
    float4 v[IMG_PER];                                             // all loads in flight first
#pragma unroll
    for (int k = 0; k < IMG_PER; ++k) {
        const int e0 = 4 * (tid + k * IMG_T) - a;
        v[k] = e0 < E ? img_piece(x, gbase, e0, E) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < IMG_PER; ++k) sig_pin(v[k]);
#pragma unroll
    for (int k = 0; k < IMG_PER; ++k) {
        const int e0 = 4 * (tid + k * IMG_T) - a;
        if (e0 < E) img_put<FOLD>(x, gbase, y, ybase, e0, E, v[k], m);
    }
    // a shifted full tile ends half a piece further on
    for (int c = tid + IMG_PER * IMG_T; 4 * c - a < E; c += IMG_T) {
        const int e0 = 4 * c - a;
        img_put<FOLD>(x, gbase, y, ybase, e0, E, img_piece(x, gbase, e0, E), m);
    }
}
