// kernels_loudness.h — the device side of msg_loudness / msg_loudness_gain (TU
// k_loudness.hip).  The definition, the tile shapes and the table layout are in
// loudness.h; DESIGN.md "Loudness" explains the decomposition.
//
//   k_loud_tiles<CH, false>  sweep 1, one workgroup per tile: each lane runs the
//                            cascade from zero state over its chunk, the lanes'
//                            end states are scanned in order, and the tile's
//                            zero-state end state and sample peak are written
//   k_loud_scan              one thread per (signal, channel): the ordered scan
//                            over its tiles, s_in[t+1] = A^len(t) s_in[t] + s_zs_end[t],
//                            in place (the slot of tile t then holds s_in[t])
//   k_loud_tiles<CH, true>   sweep 2: the same lane scan seeded with s_in[t], then
//                            every lane reruns its chunk from its true state and
//                            the squares fold into one sum per tile
//   k_loud_gate              one wave per signal: z_j from four hop sums (a hop
//                            sum: its tiles in order), both gates, the peak, the record
//   k_loud_gain              g from the record in float64, x *= (float)g in place
//
// Staged tile: chunk l of a tile lies at LDS frame l LD_ROW (LD_ROW = LD_C + 1):
// a lane's frame k is at dword CH (17 l + k), so the 32 lanes of a read group hit
// 32 different banks (mono, ds_read_b32: stride 17 dwords, odd) or 32 different
// bank pairs (stereo, ds_read_b64: stride 34 dwords = 2 x 17).
#pragma once
#include <hip/hip_runtime.h>
#include "loudness.h"
#include "sig_tiles.h"

// out = M v + add, M 4 x 4 row-major (out may be v or add)
MSG_DEV void ld_mv(const double* __restrict__ M, const double (&v)[4], const double (&add)[4], double (&out)[4]) {
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        r[i] = (((M[4 * i] * v[0] + M[4 * i + 1] * v[1]) + M[4 * i + 2] * v[2]) + M[4 * i + 3] * v[3]) + add[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = r[i];
}

// the signal holding a tile (last p with tile_base[p] <= tile) and the tile's place in it
struct LdTile {
    int p;          // signal
    int lt;         // frames of the tile (1 .. LD_TILE)
    int64_t f0;     // first frame, from the signal's base
};
MSG_DEV LdTile ld_locate(const int64_t* __restrict__ meta, int n_sig, int64_t hop, int tph, int64_t tile) {
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    LdTile t;
    t.p = sig_owner(tile_base, n_sig, tile);
    const int64_t n = meta[n_sig + t.p], tt = tile - tile_base[t.p];
    const int64_t h = tt / tph, ti = tt - h * tph;
    const int64_t hl = n - h * hop < hop ? n - h * hop : hop;
    t.f0 = h * hop + ti * LD_TILE;
    const int64_t left = hl - ti * LD_TILE;
    t.lt = (int)(left < LD_TILE ? left : LD_TILE);
    return t;
}

// cl frames of a staged chunk through the cascade; returns the sum of squares when ENERGY
template <int CH, bool ENERGY, bool FULL>
MSG_DEV double ld_run(const double (&c)[10], const float* chunk, int cl, double (&z)[CH][4]) {
    double acc = 0.0;
    if (FULL) {
#pragma unroll
        for (int k = 0; k < LD_C; ++k)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const double y = ld_step(c, z[ch], (double)chunk[k * CH + ch]);
                if (ENERGY) acc += y * y;
            }
    } else {                                            // unrolled too: the states stay in registers
#pragma unroll
        for (int k = 0; k < LD_C; ++k)
            if (k < cl) {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    const double y = ld_step(c, z[ch], (double)chunk[k * CH + ch]);
                    if (ENERGY) acc += y * y;
                }
            }
    }
    return acc;
}

template <int CH, bool ENERGY>
__global__ void __launch_bounds__(LD_T)
k_loud_tiles(const float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, int64_t hop, int tph,
             const double* __restrict__ tab, double* __restrict__ state, double* __restrict__ part) {
    __shared__ float lds[LD_T * LD_ROW * CH];
    __shared__ double wv[LD_T / 64][CH][4];
    __shared__ double red[LD_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const LdTile t = ld_locate(meta, n_sig, hop, tph, tile);
    const float* xs = x + (meta[t.p] + t.f0) * CH;      // 64-bit from the buffer's base

    // stage the tile: all loads in flight first
    float v[LD_C][CH];
#pragma unroll
    for (int k = 0; k < LD_C; ++k) {
        const int f = k * LD_T + tid;
        if (CH == 2) {
            typedef float v2f __attribute__((ext_vector_type(2)));
            const v2f w = f < t.lt ? reinterpret_cast<const v2f*>(xs)[f] : v2f{0.f, 0.f};
            v[k][0] = w.x; v[k][CH - 1] = w.y;
        } else {
            v[k][0] = f < t.lt ? xs[f] : 0.f;
        }
    }
    float pk = 0.f;
#pragma unroll
    for (int k = 0; k < LD_C; ++k) {
        const int f = k * LD_T + tid;
        if (f < t.lt) {
            const int pos = ((f / LD_C) * LD_ROW + (f % LD_C)) * CH;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                lds[pos + ch] = v[k][ch];
                pk = fmaxf(pk, fabsf(v[k][ch]));
            }
        }
    }
    __syncthreads();

    double c[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) c[i] = tab[LD_TAB_COEF + i];
    const int left = t.lt - tid * LD_C;
    const int cl = left < 0 ? 0 : (left > LD_C ? LD_C : left);     // frames of this lane's chunk
    const float* chunk = lds + tid * LD_ROW * CH;

    // zero-state end state of every full chunk, then the ordered scan over the wave's lanes:
    // after level k, P = the state the last 2^(k+1) chunks up to this one leave from zero state
    double P[CH][4];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) P[ch][i] = 0.0;
    if (cl == LD_C) ld_run<CH, false, true>(c, chunk, LD_C, P);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double* M = tab + LD_TAB_LVL + 16 * k;
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            double u[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = __shfl_up(P[ch][i], 1u << k, 64);
            if (lane >= (1 << k)) ld_mv(M, u, P[ch], P[ch]);
        }
    }
    double Pex[CH][4];                                  // the chunks before this one, from the wave's start
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double u = __shfl_up(P[ch][i], 1u, 64);
            Pex[ch][i] = lane ? u : 0.0;
        }
    if (lane == 63) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < 4; ++i) wv[wave][ch][i] = P[ch][i];
    }
    __syncthreads();
    // the state at this wave's first frame: the tile's incoming state through the waves before it
    double V[CH][4];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch)
#pragma unroll
        for (int i = 0; i < 4; ++i) V[ch][i] = ENERGY ? state[(tile * CH + ch) * 4 + i] : 0.0;
    for (int w = 0; w < wave; ++w)
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) ld_mv(tab + LD_TAB_WAVE, V[ch], wv[w][ch], V[ch]);
    const double* Ml = tab + LD_TAB_LANE + 16 * lane;   // A^(LD_C lane)

    if (!ENERGY) {
        // the tile's zero-state end state: after the last full chunk, or after the
        // frames of the one partial chunk run from the state in front of it
        const int m = t.lt / LD_C;
        if (m == LD_T) {
            if (tid == LD_T - 1) {
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    double e[4];
                    ld_mv(Ml + 16, V[ch], P[ch], e);
#pragma unroll
                    for (int i = 0; i < 4; ++i) state[(tile * CH + ch) * 4 + i] = e[i];
                }
            }
        } else if (tid == m) {
            double s[CH][4];
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) ld_mv(Ml, V[ch], Pex[ch], s[ch]);
            ld_run<CH, false, false>(c, chunk, cl, s);
#pragma unroll
            for (int ch = 0; ch < CH; ++ch)
#pragma unroll
                for (int i = 0; i < 4; ++i) state[(tile * CH + ch) * 4 + i] = s[ch][i];
        }
        // the tile's sample peak
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
        if (lane == 0) red[wave] = (double)pk;
        __syncthreads();
        if (tid == 0) {
            double r = red[0];
            for (int w = 1; w < LD_T / 64; ++w) r = r > red[w] ? r : red[w];
            part[2 * tile + 1] = r;
        }
    } else {
        double acc = 0.0;
        if (cl > 0) {
            double s[CH][4];
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) ld_mv(Ml, V[ch], Pex[ch], s[ch]);
            acc = cl == LD_C ? ld_run<CH, true, true>(c, chunk, LD_C, s) : ld_run<CH, true, false>(c, chunk, cl, s);
        }
        // fixed order: xor-butterfly in each wave, then the waves in order (dg_block_fold)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            double r = red[0];
            for (int w = 1; w < LD_T / 64; ++w) r += red[w];
            part[2 * tile] = r;
        }
    }
}

// the ordered scan over a signal's tiles, one thread per (signal, channel), in place
__global__ void __launch_bounds__(64)
k_loud_scan(const int64_t* __restrict__ meta, int n_sig, int channels, int64_t hop, int tph,
            const double* __restrict__ tab, double* state) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    const int p = idx / channels, ch = idx - p * channels;
    if (p >= n_sig) return;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t n = meta[n_sig + p], t0 = tile_base[p], t1 = tile_base[p + 1];
    double AT[16], AR[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { AT[i] = tab[LD_TAB_AT + i]; AR[i] = tab[LD_TAB_AR + i]; }
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t h = 0;
    int ti = 0;
    constexpr int B = 4;                                // tiles fetched ahead of the chain
    for (int64_t tb = t0; tb < t1; tb += B) {
        double e[B][4];
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) e[b][i] = tb + b < t1 ? state[((tb + b) * channels + ch) * 4 + i] : 0.0;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (tb + b >= t1) break;
            double* st = state + ((tb + b) * channels + ch) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) st[i] = s[i];
            const int64_t hl = n - h * hop < hop ? n - h * hop : hop;
            const bool full = hl - (int64_t)ti * LD_TILE >= LD_TILE;
            double M[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) M[i] = full ? AT[i] : AR[i];
            ld_mv(M, s, e[b], s);
            if (++ti == tph) { ti = 0; ++h; }
        }
    }
}

// z of block j of a signal whose tiles start at t0: four hop sums, each its tiles in order
MSG_DEV double ld_block_z(const double* __restrict__ part, int64_t t0, int tph, int64_t hop, int64_t j) {
    double hs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t tb = t0 + (j + k) * tph;
        double a = part[2 * tb];
        for (int i = 1; i < tph; ++i) a += part[2 * (tb + i)];
        hs[k] = a;
    }
    return (((hs[0] + hs[1]) + hs[2]) + hs[3]) / (4.0 * (double)hop);
}

// one wave per signal: lane i takes blocks i, i + 64, ... in order, then the xor-butterfly
__global__ void __launch_bounds__(LD_GT)
k_loud_gate(const int64_t* __restrict__ meta, int n_sig, int64_t hop, int tph, const double* __restrict__ part,
            LoudRec* __restrict__ rec) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t n = meta[n_sig + p], t0 = tile_base[p], t1 = tile_base[p + 1];
    const int64_t nb = n < 4 * hop ? 0 : (n - 4 * hop) / hop + 1;
    double s1 = 0.0, s2 = 0.0, pk = 0.0;
    int64_t c1 = 0, c2 = 0;
    for (int64_t j = lane; j < nb; j += LD_GT) {
        const double z = ld_block_z(part, t0, tph, hop, j);
        if (ld_level(z) > -70.0) { s1 += z; ++c1; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { s1 += __shfl_xor(s1, o, 64); c1 += sig_shfl64(c1, o); }
    const double gate = c1 ? ld_level(s1 / (double)c1) - 10.0 : 0.0;
    if (c1)
        for (int64_t j = lane; j < nb; j += LD_GT) {
            const double z = ld_block_z(part, t0, tph, hop, j), l = ld_level(z);
            if (l > -70.0 && l > gate) { s2 += z; ++c2; }
        }
    for (int64_t t = t0 + lane; t < t1; t += LD_GT) pk = pk > part[2 * t + 1] ? pk : part[2 * t + 1];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s2 += __shfl_xor(s2, o, 64);
        c2 += sig_shfl64(c2, o);
        const double q = __shfl_xor(pk, o, 64);
        pk = pk > q ? pk : q;
    }
    if (lane == 0) {
        LoudRec r;
        r.mean_sq = c2 ? s2 / (double)c2 : 0.0;
        r.lufs = c2 ? ld_level(r.mean_sq) : -__builtin_inf();
        r.peak = pk;
        r.gain = 0.0;
        r.n_blocks = (int32_t)nb;
        r.n_kept = (int32_t)c2;
        rec[p] = r;
    }
}

// g = 10^((target - lufs) / 20), held to ceiling / peak when ceiling > 0; lufs = -inf: g = 1
MSG_DEV double ld_gain_of(const LoudRec* r, double target, double ceiling) {
    const double lufs = r->lufs, peak = r->peak;
    if (!(lufs > -__builtin_inf())) return 1.0;
    double g = exp10((target - lufs) / 20.0);
    if (ceiling > 0.0 && g * peak > ceiling) g = ceiling / peak;
    return g;
}

// meta: offsets, frames, then n_sig + 1 first tiles of LD_GAIN_TILE frames; grid max(1, tiles)
template <int CH>
__global__ void __launch_bounds__(LD_T)
k_loud_gain(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, LoudRec* rec, double target,
            double ceiling) {
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t tile = blockIdx.x;
    if (tile == 0)                                       // signals without a tile get their gain here
        for (int q = threadIdx.x; q < n_sig; q += LD_T)
            if (tile_base[q + 1] == tile_base[q]) rec[q].gain = ld_gain_of(rec + q, target, ceiling);
    if (tile >= tile_base[n_sig]) return;
    int lo = 0, hi = n_sig;                              // sig_owner's search, written out (see sig_tiles.h)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_base[mid] <= tile) lo = mid; else hi = mid;
    }
    const int p = __builtin_amdgcn_readfirstlane(lo);
    const double g = ld_gain_of(rec + p, target, ceiling);
    if (tile == tile_base[p] && threadIdx.x == 0) rec[p].gain = g;
    sig_scale<CH, LD_T, LD_GAIN_PER>(x, meta, n_sig, p, tile, (float)g);
}
