// kernels_flac.h — the device side of msg_flac (TU k_flac.hip).  The definition, the chunk helpers
// and the host loop are in flac.h; DESIGN.md "4n. FLAC" explains the decomposition.
//
//   k_flac_plan<CH>     read-only, one workgroup per (signal, block): the block's samples into LDS
//                       (rows of 16 + 1 words), then per channel (L, R, mid, side; one for mono) the
//                       range and the five sums of |r_o| over the lanes' chunks, the order, the
//                       residuals in registers, the sums of the finest partitions, every coarser
//                       level's sums and k0, the three exact bit counts per partition and level,
//                       the cheapest parameter and partition order; lane 0 picks the assignment and
//                       writes the block's FlacPlan with the frame's exact bytes.
//   k_flac_scan         one workgroup per signal: the exclusive prefix of its frames' bytes over
//                       blocks of FLAC_T frames (a wave scan, the waves through LDS, the blocks in
//                       order), and the record: bytes, frames, smallest and largest frame, counts.
//   k_flac_offsets      one workgroup: the prefix over the signals of their bytes rounded up to 16.
//   k_flac_pack<CH>     one workgroup per (signal, block): the samples again, a zeroed frame in LDS,
//                       per subframe the code lengths of the lanes' chunks, their workgroup prefix,
//                       each sample's one bit and low bits ORed in (the unary zeros are there),
//                       the header by lane 0, CRC-16 from the lanes' chunk CRCs shifted by
//                       x^(8 bytes after the chunk) and XORed, the frame stored with 4-byte stores.
//   k_flac_md5          one wave per signal: 4 KB of the PCM staged into LDS by the wave, the
//                       chain walked by lane 0.  Launched only when the MD5 is asked for.
#pragma once
#include <hip/hip_runtime.h>
#include "flac.h"
#include "sig_tiles.h"

struct FlacAddLds {
    MSG_DEV void add(unsigned long long* p, unsigned long long v) const { if (v) atomicAdd(p, v); }
    MSG_DEV void lo(int32_t* p, int32_t v) const { atomicMin(p, v); }
    MSG_DEV void hi(int32_t* p, int32_t v) const { atomicMax(p, v); }
};
// OR into the frame's words; a word outside the frame is never touched
struct FlacOrLds {
    uint32_t* base;
    int words;
    MSG_DEV void operator()(uint32_t* p, uint32_t v) const {
        if ((uint64_t)(p - base) < (uint64_t)words) atomicOr(p, v);
    }
};

// word w of the block at base (16-byte aligned); avail: the bytes from base to the signal's end
MSG_DEV int32_t flac_load_dev(const uint8_t* base, int bits, int64_t w, int64_t avail) {
    if (bits == 16) return reinterpret_cast<const int16_t*>(base)[w];
    const int64_t a = 3 * w, d = a >> 2;
    if (4 * d + 8 > avail) return flac_load(base, 24, w);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(base);
    const uint64_t v = (uint64_t)q[d] | ((uint64_t)q[d + 1] << 32);
    return (int32_t)((uint32_t)(v >> (8 * (int)(a & 3))) << 8) >> 8;
}

// what both sweeps know of their block
struct FlacBlock {
    int p;                                      // the signal
    int64_t j;                                  // the block in it
    int bn;                                     // its samples
};
template <int CH>
MSG_DEV FlacBlock flac_block_load(const uint8_t* __restrict__ pcm, const int64_t* __restrict__ meta, int n_sig, int bits, int B,
                                  int32_t* l, int32_t* r) {
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t tile = blockIdx.x;
    FlacBlock b;
    b.p = sig_owner(tile_base, n_sig, tile);
    b.j = tile - tile_base[b.p];
    const int64_t n = meta[n_sig + b.p], left = n - b.j * B;
    b.bn = (int)(left < B ? left : B);
    const int bps = bits >> 3;
    const uint8_t* base = pcm + meta[b.p] + b.j * B * CH * bps;
    const int64_t avail = left * CH * bps;
    for (int w = threadIdx.x; w < b.bn * CH; w += FLAC_T) {
        const int32_t v = flac_load_dev(base, bits, w, avail);
        if (CH == 2) ((w & 1) ? r : l)[flac_pos(w >> 1)] = v;
        else l[flac_pos(w)] = v;
    }
    return b;
}

template <int CH>
__global__ void __launch_bounds__(FLAC_T)
k_flac_plan(const uint8_t* __restrict__ pcm, const int64_t* __restrict__ meta, int n_sig, int bits, int B, int sr,
            FlacPlan* __restrict__ plan) {
    __shared__ int32_t xl[FLAC_XS];
    __shared__ int32_t xr[CH == 2 ? FLAC_XS : 1];
    __shared__ FlacWork W;
    __shared__ FlacBest best[4];
    const int tid = threadIdx.x;
    const FlacBlock b = flac_block_load<CH>(pcm, meta, n_sig, bits, B, xl, xr);
    const int bn = b.bn, cw = (bn + FLAC_T - 1) / FLAC_T;
    const int i0 = tid * cw < bn ? tid * cw : bn, i1 = i0 + cw < bn ? i0 + cw : bn;
    const FlacAddLds add{};
    for (int c = 0; c < (CH == 2 ? 4 : 1); ++c) {
        const FlacX x{xl, CH == 2 ? xr : xl, c};
        const int d = bits + (c == 3 ? 1 : 0);
        if (tid < 128) flac_work_zero(&W, tid);
        if (tid == 0) flac_work_init(&W);
        __syncthreads();                                // the samples are in LDS too
        flac_chunk_abs(x, i0, i1, &W, add);
        __syncthreads();
        const int o = flac_order(W.abs), pm = flac_pmax(bn, o);
        if (bn > 4 && W.mn != W.mx) {                   // the same for every lane
            uint32_t u[FLAC_C];
            flac_chunk_S(x, i0, i1, o, pm, bn, u, &W, add);
            __syncthreads();
            if (tid < 127) flac_entry_k0(&W, bn, o, pm, bits, tid);
            __syncthreads();
            flac_chunk_E(u, i0, i1, pm, bn, &W, add);
            __syncthreads();
            if (tid < 127) flac_entry_pick(&W, bn, o, pm, bits, tid);
            __syncthreads();
        }
        if (tid == 0) flac_finish(&W, bn, d, bits, o, pm, &best[c]);
        __syncthreads();                                // W is zeroed again
    }
    if (tid == 0) {
        uint8_t hdr[FLAC_HDR_MAX];
        const int hb = flac_header(hdr, B, bn, sr, CH == 2 ? 0 : -1, bits, b.j);
        flac_assign(best, CH, hb, &plan[blockIdx.x]);
    }
}

MSG_DEV int64_t flac_shfl_up(int64_t v, int o) { return (int64_t)__shfl_up((long long)v, (unsigned)o, 64); }

// The prefix of a signal's frame bytes, and its record but for byte_off and the MD5.
__global__ void __launch_bounds__(FLAC_T)
k_flac_scan(const int64_t* __restrict__ meta, int n_sig, int channels, const FlacPlan* __restrict__ plan,
            int64_t* __restrict__ pre, FlacRec* __restrict__ rec) {
    __shared__ int64_t wt[FLAC_T / 64];
    __shared__ int32_t red[9];                          // smallest, largest, constant, verbatim, fixed, four assignments
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int64_t* tile_base = meta + 2 * (int64_t)n_sig;
    const int64_t t0 = tile_base[p], T = tile_base[p + 1] - t0;
    if (tid < 9) red[tid] = tid == 0 ? INT32_MAX : 0;
    __syncthreads();
    int32_t mn = INT32_MAX, mx = 0, cnt[7] = {0, 0, 0, 0, 0, 0, 0};
    int64_t c = 0;                                      // the bytes in front of this block of frames
    for (int64_t base = 0; base < T; base += FLAC_T) {
        const int64_t u = base + tid;
        int64_t v = 0;
        if (u < T) {
            const FlacPlan& q = plan[t0 + u];
            v = q.bytes;
            mn = q.bytes < mn ? q.bytes : mn;
            mx = q.bytes > mx ? q.bytes : mx;
            for (int s = 0; s < channels; ++s) cnt[q.sub[s].type] += 1;
            if (channels == 2) cnt[3 + q.assign] += 1;
        }
        int64_t inc = v;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int64_t w = flac_shfl_up(inc, 1 << j);
            if (lane >= (1 << j)) inc += w;
        }
        if (lane == 63) wt[wave] = inc;
        __syncthreads();
        int64_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < FLAC_T / 64; ++w) {
            if (w < wave) before += wt[w];
            all += wt[w];
        }
        if (u < T) pre[t0 + u] = c + before + inc - v;
        c += all;
        __syncthreads();                                // wt is written again
    }
    if (T > 0) {
        atomicMin(&red[0], mn);
        atomicMax(&red[1], mx);
        for (int k = 0; k < 7; ++k)
            if (cnt[k]) atomicAdd(&red[2 + k], cnt[k]);
    }
    __syncthreads();
    if (tid == 0) {
        FlacRec r;
        r.byte_off = 0;
        r.bytes = c;
        r.frames = T;
        r.samples = meta[n_sig + p];
        r.min_frame = T > 0 ? red[0] : 0;
        r.max_frame = red[1];
        for (int k = 0; k < 16; ++k) r.md5[k] = 0;
        r.constant = red[2]; r.verbatim = red[3]; r.fixed = red[4]; r.flags = 0;
        for (int k = 0; k < 4; ++k) r.assign[k] = red[5 + k];
        rec[p] = r;
    }
}

// byte_off of every signal: the prefix of the signals' bytes, each rounded up to 16.
__global__ void __launch_bounds__(FLAC_T)
k_flac_offsets(int n_sig, FlacRec* __restrict__ rec) {
    __shared__ int64_t wt[FLAC_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t c = 0;
    for (int base = 0; base < n_sig; base += FLAC_T) {
        const int u = base + tid;
        const int64_t v = u < n_sig ? (rec[u].bytes + 15) & ~(int64_t)15 : 0;
        int64_t inc = v;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int64_t w = flac_shfl_up(inc, 1 << j);
            if (lane >= (1 << j)) inc += w;
        }
        if (lane == 63) wt[wave] = inc;
        __syncthreads();
        int64_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < FLAC_T / 64; ++w) {
            if (w < wave) before += wt[w];
            all += wt[w];
        }
        if (u < n_sig) rec[u].byte_off = c + before + inc - v;
        c += all;
        __syncthreads();
    }
}

template <int CH>
__global__ void __launch_bounds__(FLAC_T)
k_flac_pack(const uint8_t* __restrict__ pcm, const int64_t* __restrict__ meta, int n_sig, int bits, int B, int sr,
            const FlacPlan* __restrict__ plan, const int64_t* __restrict__ pre, const FlacRec* __restrict__ rec,
            uint8_t* __restrict__ out, int64_t out_bytes) {
    __shared__ int32_t xl[FLAC_XS];
    __shared__ int32_t xr[CH == 2 ? FLAC_XS : 1];
    __shared__ uint32_t fw[FLAC_FRAME_WORDS];
    __shared__ FlacPlan P;
    __shared__ int32_t wsum[FLAC_T / 64];
    __shared__ uint32_t wcrc[FLAC_T / 64];
    static_assert(sizeof(FlacPlan) % 4 == 0, "the plan is copied by words");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FlacBlock b = flac_block_load<CH>(pcm, meta, n_sig, bits, B, xl, xr);
    if (tid < (int)(sizeof(FlacPlan) / 4))
        reinterpret_cast<uint32_t*>(&P)[tid] = reinterpret_cast<const uint32_t*>(&plan[blockIdx.x])[tid];
    __syncthreads();
    const int bn = b.bn, cw = (bn + FLAC_T - 1) / FLAC_T;
    const int i0 = tid * cw < bn ? tid * cw : bn, i1 = i0 + cw < bn ? i0 + cw : bn;
    const int total = P.bytes;                          // the frame, CRC-16 included
    if (total < 4 || total > (int)flac_frame_bound(bn, CH, bits)) return;      // never by the definition
    const int words = (total + 3) / 4 + 1;
    for (int k = tid; k < words; k += FLAC_T) fw[k] = 0;
    __syncthreads();
    const FlacOrLds orr{fw, words};

    uint8_t hdr[FLAC_HDR_MAX];
    const int hb = flac_header(hdr, B, bn, sr, P.assign, bits, b.j);
    if (tid < hb) flac_put(orr, fw, 8 * tid, hdr[tid], 8);
    int64_t pos = 8 * hb;
    for (int s = 0; s < CH; ++s) {
        const int c = flac_assign_chan(P.assign, s), d = bits + (c == 3 ? 1 : 0);
        const FlacX x{xl, CH == 2 ? xr : xl, c};
        const FlacBest& sub = P.sub[s];
        const int64_t first = flac_sub_head(x, sub, d, bits, pos, fw, orr, tid == 0);
        if (sub.type == FLAC_TYPE_CONSTANT) {
            pos = first + d;
        } else if (sub.type == FLAC_TYPE_VERBATIM) {
            for (int i = tid; i < bn; i += FLAC_T) flac_put(orr, fw, first + (int64_t)i * d, (uint32_t)x(i) & flac_mask(d), d);
            pos = first + (int64_t)bn * d;
        } else {
            const int o = sub.order;
            if (tid < o) flac_put(orr, fw, first + (int64_t)tid * d, (uint32_t)x(tid) & flac_mask(d), d);
            uint32_t u[FLAC_C];
            const int32_t len = flac_chunk_len(x, i0, i1, sub, bn, bits, u);
            int32_t inc = len;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int32_t w = __shfl_up(inc, (unsigned)(1 << j), 64);
                if (lane >= (1 << j)) inc += w;
            }
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();
            int32_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < FLAC_T / 64; ++w) {
                if (w < wave) before += wsum[w];
                all += wsum[w];
            }
            const int64_t base = first + (int64_t)o * d + 6;
            flac_chunk_pack(u, i0, i1, sub, bn, bits, base + before + inc - len, fw, orr);
            pos = base + all;
            __syncthreads();                            // wsum is written again
        }
    }
    __syncthreads();                                    // the frame's bits are in
    const int nb = total - 2;                           // (pos + 7) >> 3 by the plan
    {
        const int m = (nb + FLAC_T - 1) / FLAC_T;
        const int a0 = tid * m < nb ? tid * m : nb, a1 = a0 + m < nb ? a0 + m : nb;
        uint32_t crc = 0;
        for (int a = a0; a < a1; ++a) crc = flac_crc16(crc, flac_byte(fw, a));
        if (crc) crc = flac_mulmod16(crc, flac_xpow16((uint32_t)(nb - a1)));
#pragma unroll
        for (int sft = 32; sft > 0; sft >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, sft, 64);
        if (lane == 0) wcrc[wave] = crc;
        __syncthreads();
        if (tid == 0) {
            uint32_t all = 0;
            for (int w = 0; w < FLAC_T / 64; ++w) all ^= wcrc[w];
            if ((int64_t)nb * 8 >= pos) flac_put(orr, fw, (int64_t)nb * 8, all, 16);
        }
        __syncthreads();
    }
    const int64_t at = rec[b.p].byte_off + pre[blockIdx.x];
    if (at < 0 || at + total > out_bytes) return;       // never by msg_flac's size check
    uint8_t* dst = out + at;
    const int head = (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3), h = head < total ? head : total;
    const int nd = (total - h) >> 2;
    if (tid < h) dst[tid] = (uint8_t)flac_byte(fw, tid);
    for (int k = tid; k < nd; k += FLAC_T) {
        const int a = h + 4 * k;
        reinterpret_cast<uint32_t*>(dst + h)[k] =
            flac_byte(fw, a) | (flac_byte(fw, a + 1) << 8) | (flac_byte(fw, a + 2) << 16) | (flac_byte(fw, a + 3) << 24);
    }
    const int tail = h + 4 * nd;
    if (tid < total - tail) dst[tail + tid] = (uint8_t)flac_byte(fw, tail + tid);
}

// MD5 of every signal's packed PCM bytes: one wave per signal.
__global__ void __launch_bounds__(64)
k_flac_md5(const uint8_t* __restrict__ pcm, const int64_t* __restrict__ meta, int n_sig, int frame_bytes,
           FlacRec* __restrict__ rec) {
    __shared__ uint32_t buf[1024];
    const int lane = threadIdx.x, p = blockIdx.x;
    const uint8_t* base = pcm + meta[p];
    const int64_t nbytes = meta[n_sig + p] * frame_bytes, full = nbytes >> 6;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(base);
    uint32_t st[4];
    flac_md5_init(st);
    for (int64_t blk = 0; blk < full; blk += 64) {
        const int cnt = (int)(full - blk < 64 ? full - blk : 64);
        for (int k = lane; k < cnt * 16; k += 64) buf[k] = src[blk * 16 + k];
        __syncthreads();
        if (lane == 0)
            for (int q = 0; q < cnt; ++q) flac_md5_block(st, buf + 16 * q);
        __syncthreads();
    }
    if (lane == 0) {
        uint8_t tail[64];
        const int rest = (int)(nbytes - (full << 6));
        for (int i = 0; i < 64; ++i) tail[i] = i < rest ? base[(full << 6) + i] : 0;
        uint8_t md[16];
        flac_md5_finish(st, tail, rest, (uint64_t)nbytes, md);
        for (int i = 0; i < 16; ++i) rec[p].md5[i] = md[i];
        rec[p].flags |= 1;
    }
}
