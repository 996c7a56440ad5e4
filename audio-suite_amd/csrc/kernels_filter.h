// kernels_filter.h — the device side of msg_filter (TU k_filter.hip).  The definition, the
// tile shapes and the table layout are in filter.h; DESIGN.md "4j. Filter" explains the
// decomposition, which is that of the loudness pass (kernels_loudness.h) with a caller's
// cascade and with the filtered samples written back.
//
//   k_filter_tiles<CH, false>  sweep 1, one workgroup per tile of FL_TILE frames counted from
//                              the signal's first frame (its last with FL_REVERSE): the tile
//                              runs through the cascade from zero state and its end state,
//                              2S words per channel, is written.  A signal's last tile has
//                              no successor, so a shorter tile returns at once.
//   k_filter_scan              16 lanes per (signal, channel): the ordered scan over its tiles,
//                              s_in[t+1] = A^FL_TILE s_in[t] + s_end[t], A the joint 2S x 2S
//                              zero-input step, in place (the slot of tile t then holds s_in[t])
//   k_filter_tiles<CH, true>   sweep 2: the same work from the tile's true incoming state, the
//                              cascade's output rounded to float32 and stored over the input.
//                              A tile reads only its own span, so in place is safe.
//
// Inside a tile a lane holds its chunk of FL_C frames in registers as float64 and the tile
// goes through the cascade section by section.  Per section: the chunk's end state from zero
// state, the ordered scan of those over the wave's lanes with A_k^(FL_C 2^j) (2 x 2), the
// waves in order through LDS, and the chunk again from its true state, its output replacing
// the chunk in the registers as the next section's input.
//
// No workgroup waits on another and nothing is added atomically: the launches order the
// phases and every fold has one written order, so a signal's samples do not depend on the
// batch it lies in.  A NaN only travels to later lanes, waves and tiles of its own signal
// and channel.
//
// Staged tile: chunk l lies at LDS frame l FL_ROW (FL_ROW = FL_C + 1), as in the loudness
// pass: a lane's frame k is at dword CH (17 l + k), conflict-free for the 32 lanes of a
// read group, mono and stereo.
#pragma once
#include <hip/hip_runtime.h>
#include "filter.h"
#include "sig_tiles.h"

// out = M v + add, M 2 x 2 row-major (out may be v or add)
MSG_DEV void fl_mv(const double* __restrict__ M, const double (&v)[2], const double (&add)[2], double (&out)[2]) {
    const double r0 = (M[0] * v[0] + M[1] * v[1]) + add[0];
    const double r1 = (M[2] * v[0] + M[3] * v[1]) + add[1];
    out[0] = r0;
    out[1] = r1;
}

// cl frames of a chunk through one section from state z; OUT: the outputs replace the chunk
template <int CH, bool OUT, bool FULL>
MSG_DEV void fl_run(const double (&c)[5], double (&v)[FL_C][CH], int cl, double (&z)[CH][2]) {
#pragma unroll
    for (int k = 0; k < FL_C; ++k)
        if (FULL || k < cl) {                           // unrolled: the chunk and the states stay in registers
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const double y = fl_step<double>(c, z[ch], v[k][ch]);
                if (OUT) v[k][ch] = y;
            }
        }
}

template <int CH, bool WRITE>
__global__ void __launch_bounds__(FL_T)
k_filter_tiles(float* __restrict__ x, const int64_t* __restrict__ meta, int n_sig, int S, int reverse,
               const double* __restrict__ tab, double* __restrict__ state) {
    __shared__ float lds[FL_T * FL_ROW * CH];
    __shared__ double wv[FL_MAX_SECTIONS][FL_T / 64][CH][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t tile = blockIdx.x;
    const int p = sig_owner(tile_base, n_sig, tile);
    const int64_t n = meta[n_sig + p], f0 = (tile - tile_base[p]) * FL_TILE;
    const int lt = (int)(n - f0 < FL_TILE ? n - f0 : FL_TILE);       // frames of the tile (1 .. FL_TILE)
    if (!WRITE && lt < FL_TILE) return;                 // the signal's last tile: nobody reads its end state
    // frame r of the tile: forward f0 + r of the signal, reverse n - 1 - f0 - r
    float* xs = x + (meta[p] + (reverse ? n - 1 - f0 : f0)) * CH;    // 64-bit from the buffer's base
    const int step = reverse ? -1 : 1;
    typedef float v2f __attribute__((ext_vector_type(2)));

    // stage the tile: all loads in flight first
    float ld[FL_C][CH];
#pragma unroll
    for (int k = 0; k < FL_C; ++k) {
        const int f = k * FL_T + tid;
        if (CH == 2) {
            const v2f w = f < lt ? reinterpret_cast<const v2f*>(xs)[step * f] : v2f{0.f, 0.f};
            ld[k][0] = w.x; ld[k][CH - 1] = w.y;
        } else {
            ld[k][0] = f < lt ? xs[step * f] : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < FL_C; ++k) {
        const int f = k * FL_T + tid;
        if (f < lt) {
            const int pos = ((f / FL_C) * FL_ROW + (f % FL_C)) * CH;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) lds[pos + ch] = ld[k][ch];
        }
    }
    __syncthreads();

    const int left = lt - tid * FL_C;
    const int cl = left < 0 ? 0 : (left > FL_C ? FL_C : left);       // frames of this lane's chunk
    float* chunk = lds + tid * FL_ROW * CH;
    double v[FL_C][CH];
#pragma unroll
    for (int k = 0; k < FL_C; ++k)
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) v[k][ch] = k < cl ? (double)chunk[k * CH + ch] : 0.0;

    const int n2 = 2 * S;
    for (int s = 0; s < S; ++s) {
        const double* sec = tab + FL_TAB_SEC + s * FL_SEC_N;
        double c[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) c[i] = sec[FL_SEC_COEF + i];

        // zero-state end state of every full chunk, then the ordered scan over the wave's lanes:
        // after level j, P = the state the last 2^(j+1) chunks up to this one leave from zero state
        double P[CH][2];
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) P[ch][0] = P[ch][1] = 0.0;
        if (cl == FL_C) fl_run<CH, false, true>(c, v, FL_C, P);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double* M = sec + FL_SEC_LVL + 4 * j;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                double u[2];
                u[0] = __shfl_up(P[ch][0], 1u << j, 64);
                u[1] = __shfl_up(P[ch][1], 1u << j, 64);
                if (lane >= (1 << j)) fl_mv(M, u, P[ch], P[ch]);
            }
        }
        double Pex[CH][2];                              // the chunks before this one, from the wave's start
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const double u = __shfl_up(P[ch][i], 1u, 64);
                Pex[ch][i] = lane ? u : 0.0;
            }
        if (lane == 63) {
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) { wv[s][wave][ch][0] = P[ch][0]; wv[s][wave][ch][1] = P[ch][1]; }
        }
        __syncthreads();                                // one slot of wv per section: no second barrier
        // the state at this wave's first frame: the tile's incoming state through the waves before it
        double V[CH][2];
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int i = 0; i < 2; ++i) V[ch][i] = WRITE ? state[(tile * CH + ch) * n2 + 2 * s + i] : 0.0;
        for (int w = 0; w < wave; ++w)
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) fl_mv(sec + FL_SEC_WAVE, V[ch], wv[s][w][ch], V[ch]);
        const double* Ml = sec + FL_SEC_LANE + 4 * lane;               // A_k^(FL_C lane)

        if (!WRITE && tid == FL_T - 1) {                // the tile is full: its end state lies after the last chunk
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                double e[2];
                fl_mv(Ml + 4, V[ch], P[ch], e);
                state[(tile * CH + ch) * n2 + 2 * s] = e[0];
                state[(tile * CH + ch) * n2 + 2 * s + 1] = e[1];
            }
        }
        // the chunk again from its true state; its output is the next section's input
        if (cl > 0 && (WRITE || s + 1 < S)) {
            double z[CH][2];
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) fl_mv(Ml, V[ch], Pex[ch], z[ch]);
            if (cl == FL_C) fl_run<CH, true, true>(c, v, FL_C, z);
            else fl_run<CH, true, false>(c, v, cl, z);
        }
    }
    if (!WRITE) return;

    // the one rounding, back through the staged layout (every lane read its chunk before the
    // sections' barriers), and the tile's own frames stored where they were read
#pragma unroll
    for (int k = 0; k < FL_C; ++k)
        if (k < cl) {
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) chunk[k * CH + ch] = (float)v[k][ch];
        }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FL_C; ++k) {
        const int f = k * FL_T + tid;
        if (f < lt) {
            const int pos = ((f / FL_C) * FL_ROW + (f % FL_C)) * CH;
            if (CH == 2) {
                v2f w;
                w.x = lds[pos]; w.y = lds[pos + CH - 1];
                reinterpret_cast<v2f*>(xs)[step * f] = w;
            } else {
                xs[step * f] = lds[pos];
            }
        }
    }
}

// the ordered scan over a signal's tiles, one workgroup of FL_NS lanes per (signal, channel), in
// place: lane i carries state word i and row i of A^FL_TILE
__global__ void __launch_bounds__(64)
k_filter_scan(const int64_t* __restrict__ meta, int n_sig, int channels, int S, const double* __restrict__ tab,
              double* state) {
    const int i = threadIdx.x;
    const int p = blockIdx.x / channels, ch = blockIdx.x - p * channels;
    if (i >= FL_NS || p >= n_sig) return;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t t0 = tile_base[p], t1 = tile_base[p + 1];
    const int n2 = 2 * S;
    const bool live = i < n2;                           // the words past 2S stay zero
    double M[FL_NS];
#pragma unroll
    for (int j = 0; j < FL_NS; ++j) M[j] = tab[FL_TAB_JOINT + FL_NS * i + j];
    double s = 0.0;
    constexpr int B = 4;                                // tiles fetched ahead of the chain
    for (int64_t tb = t0; tb < t1; tb += B) {
        double e[B];
#pragma unroll
        for (int b = 0; b < B; ++b)                     // the last tile's end state is never written: not read
            e[b] = live && tb + b + 1 < t1 ? state[((tb + b) * channels + ch) * n2 + i] : 0.0;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (tb + b >= t1) break;
            if (live) state[((tb + b) * channels + ch) * n2 + i] = s;
            double r = M[0] * __shfl(s, 0, FL_NS);
#pragma unroll
            for (int j = 1; j < FL_NS; ++j) r += M[j] * __shfl(s, j, FL_NS);
            s = live ? r + e[b] : 0.0;
        }
    }
}
