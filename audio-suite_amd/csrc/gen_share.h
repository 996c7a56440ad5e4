// gen_share.h — host: which events of a batch generate their grain, and which run
// the float32 spectral chain on it (specshare, below).
//
// The reference draws event i of a render from default_rng(seed + i) (MS:650-686),
// and a batch of variants (seeds x unfolds x stretches, msgpu/batch.py) repeats
// seeds and runs them consecutively: the variants of one seed draw the same
// streams, and seeds s and s + 1 share every stream but one.  k_gen_normal<false>
// writes the same grain for two events whose generator keys are equal, so only
// the first event of the batch with a key (its owner) goes on the generator's
// list, and every event reads the micro slot of its owner (EventRt::micro_off).
//
// The key is everything the kernel's output depends on, compared bitwise: the
// stream seed + index, the event's n and gen_sr, and of the preset the mode
// after the fallback mapping (MS:686), ring_hz, ring_decay_ms and micro_ms
// (GenBasicConst, kernels_core.h).  A field the kernel comes to read belongs here.
//
// The lookup is a flat array, not a hash: presets of one class (the preset's
// part of the key) whose stream intervals [seed, seed + n_events) overlap form
// a cluster, whose streams span no more than its events; a preset that
// overlaps no other is never looked up (a batch of unrelated seeds costs the
// sort check and one sweep over the presets).  Pure host code, shared with the
// host-only build (host_san.cpp) and reached by tests through
// msg_debug_gen_owners (host_abi.inc).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/msgpu.h"

namespace genshare {

// The preset's part of a generator key.
struct ClassKey {
    int32_t mode;
    uint64_t ring_hz, ring_decay_ms, micro_ms;   // the doubles' bits
    bool operator==(const ClassKey& o) const {
        return mode == o.mode && ring_hz == o.ring_hz && ring_decay_ms == o.ring_decay_ms && micro_ms == o.micro_ms;
    }
    bool operator<(const ClassKey& o) const {
        if (mode != o.mode) return mode < o.mode;
        if (ring_hz != o.ring_hz) return ring_hz < o.ring_hz;
        if (ring_decay_ms != o.ring_decay_ms) return ring_decay_ms < o.ring_decay_ms;
        return micro_ms < o.micro_ms;
    }
};
inline uint64_t bits_of(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}
inline ClassKey class_key(const msg_preset& p) {
    return {p.gen_mode == MSG_GEN_FALLBACK ? (int32_t)MSG_GEN_NOISE_BURST : p.gen_mode, bits_of(p.ring_hz),
            bits_of(p.ring_decay_ms), bits_of(p.micro_ms)};
}

// Buffers kept between batches (grow-only).
struct Scratch {
    std::vector<ClassKey> key;        // per listed preset
    std::vector<int32_t> order;       // listed presets with events, by (class, seed)
    std::vector<int32_t> cluster;     // per listed preset: its cluster, -1 = shares with nobody
    std::vector<int64_t> lo;          // per cluster: its first stream
    std::vector<int64_t> base, size;  // per cluster: its range of head
    std::vector<int32_t> head;        // per stream of a cluster: the newest owner drawing it, -1 = none yet
    std::vector<int32_t> next;        // per owner slot: the next owner of the same stream (another n or gen_sr)
};

// owner[slot] for every event of the presets list[0, L) (indices into presets;
// events of preset p are events[slot_base[p] + k], k < n_events[p], and
// nslots bounds every slot): the slot of the first event in list order with
// the same generator key, the event's own slot when it is that event.
// share == false: every event its own owner.  Returns the number of owners.
inline int64_t assign(const msg_preset* presets, const int32_t* list, int L, const msg_event* events,
                      const int32_t* slot_base, const int32_t* n_events, int64_t nslots, bool share, int32_t* owner,
                      Scratch& S) {
    int64_t total = 0;
    for (int i = 0; i < L; ++i) total += n_events[list[i]];
    auto own = [&](int p) {
        for (int32_t k = 0, s = slot_base[p]; k < n_events[p]; ++k) owner[s + k] = s + k;
    };
    if (!share || L < 2) {
        for (int i = 0; i < L; ++i) own(list[i]);
        return total;
    }
    // streams are formed as the kernel forms them, (uint64_t)(seed + index): seeds
    // whose interval could wrap are left out of the sharing
    const int64_t seed_max = INT64_MAX - ((int64_t)1 << 32);
    S.key.resize(L);
    S.cluster.assign(L, -1);
    S.order.clear();
    for (int i = 0; i < L; ++i) {
        const msg_preset& p = presets[list[i]];
        S.key[i] = class_key(p);
        if (n_events[list[i]] > 0 && p.seed >= 0 && p.seed <= seed_max) S.order.push_back(i);
    }
    auto before = [&](int32_t a, int32_t b) {
        if (!(S.key[a] == S.key[b])) return S.key[a] < S.key[b];
        return presets[list[a]].seed < presets[list[b]].seed;
    };
    if (!std::is_sorted(S.order.begin(), S.order.end(), before))
        std::stable_sort(S.order.begin(), S.order.end(), before);
    // clusters: runs of one class whose intervals overlap the union of the run so far
    S.lo.clear(); S.base.clear(); S.size.clear();
    int64_t flat = 0;
    for (size_t a = 0; a < S.order.size();) {
        const int32_t i0 = S.order[a];
        const int64_t lo = presets[list[i0]].seed;
        int64_t hi = lo + n_events[list[i0]];
        size_t z = a + 1;
        while (z < S.order.size() && S.key[S.order[z]] == S.key[i0] && presets[list[S.order[z]]].seed < hi) {
            hi = std::max(hi, presets[list[S.order[z]]].seed + n_events[list[S.order[z]]]);
            ++z;
        }
        if (z - a > 1) {
            const int32_t c = (int32_t)S.lo.size();
            for (size_t q = a; q < z; ++q) S.cluster[S.order[q]] = c;
            S.lo.push_back(lo);
            S.base.push_back(flat);
            S.size.push_back(hi - lo);          // <= the events of the run: each preset adds at most its own
            flat += hi - lo;
        }
        a = z;
    }
    S.head.assign((size_t)flat, -1);
    if (S.next.size() < (size_t)nslots) S.next.resize((size_t)nslots);
    int64_t owners = 0;
    for (int i = 0; i < L; ++i) {
        const int p = list[i];
        const int c = S.cluster[i];
        if (c < 0) { own(p); owners += n_events[p]; continue; }
        int32_t* head = S.head.data() + S.base[c];
        const int64_t d0 = presets[p].seed - S.lo[c];
        for (int32_t k = 0, s = slot_base[p]; k < n_events[p]; ++k) {
            const msg_event& e = events[s + k];
            const int64_t d = d0 + e.index;
            owner[s + k] = s + k;
            if (e.index < 0 || d >= S.size[c]) { ++owners; continue; }   // not a planned index: no sharing
            int32_t o = head[d];
            while (o >= 0 && (events[o].n != e.n || events[o].gen_sr != e.gen_sr)) o = S.next[o];
            if (o >= 0) { owner[s + k] = o; continue; }
            S.next[s + k] = head[d];
            head[d] = s + k;
            ++owners;
        }
    }
    return owners;
}

}  // namespace genshare

// ---------------------------------------------------------------------------
// Spectral sharing: which float32-chain events of a batch run a spectral kernel.
//
// The float32 spectral chain of an event (k_spec3, k_spectral_ct, k_spectral and
// its ops == 0 copy) reads the event's micro grain and, of its EventRt, ops, n,
// gen_sr, cutoff_gen, roll, stretch, tilt_alpha, env_tau and warp_power; amp,
// start, offset and len enter in the overlap-add only.  Two events with the
// same generator owner, the same bits in those fields and the same kernel route
// therefore get the same grain, bit for bit: the first event in list order with
// such a key (its spectral owner) runs, and every reader of the grain pool takes
// the owner's slot (the per-slot grain offsets).  An event that has a
// micro_last to write (mlast_off >= 0) always runs: it may own a key, it never
// borrows one.  A field the spectral kernels come to read belongs in same_key.
//
// The owners of a generator grain are chained off the generator owner's slot
// (head, next), so an event costs one step per distinct parameter set of its
// grain, and an event that is its own generator owner is never looked up.
// ---------------------------------------------------------------------------
enum : int32_t {
    SPEC_TILT_NOISE = 1, SPEC_TILT_SKEW = 2, SPEC_LOWPASS = 4, SPEC_STRETCH = 8, SPEC_WARP = 16,
};
constexpr int32_t SPEC3_N = 37500;   // k_spec3's grain length (spec3.h)

namespace specshare {

// Stages of the float32 chain one event runs (EventRt::ops).
inline int32_t spec_ops(const msg_preset& p, const msg_event& e) {
    int32_t ops = 0;
    if (p.gen_mode == MSG_GEN_NOISE_BURST || p.gen_mode == MSG_GEN_FALLBACK) ops |= SPEC_TILT_NOISE;
    if (p.gen_mode == MSG_GEN_SKEWED) ops |= SPEC_TILT_SKEW;
    if ((p.flags & MSG_F_BANDLIMIT) && e.n >= 8) ops |= SPEC_LOWPASS;
    if ((p.flags & MSG_F_NL_WARP) && e.n >= 16) ops |= SPEC_WARP;
    if (!(p.flags & MSG_F_PARTIAL_LOCK) && e.n >= 16 && std::fabs(e.stretch - 1.0) >= 1e-9) ops |= SPEC_STRETCH;
    return ops;
}

// The preset's constants of the tilt step.
struct PresetConsts { double tilt_alpha, env_tau; };
inline PresetConsts preset_consts(const msg_preset& pr) {
    const double tilt = pr.gen_mode == MSG_GEN_FALLBACK ? -3.0 : pr.noise_tilt;
    return {std::log(std::pow(10.0, tilt / 20.0)) / std::log(2.0),
            std::max(1e-6, (pr.micro_ms / 1000.0) * (pr.gen_mode == MSG_GEN_SKEWED ? 0.2 : 0.25))};
}

// The key's fields of one event, into an EventRt or the debug hook's record.
template <class Rec>
inline void key_fields(const msg_preset& pr, const msg_event& e, const PresetConsts& c, Rec& x) {
    x.n = e.n;
    x.gen_sr = e.gen_sr;
    x.ops = spec_ops(pr, e);
    x.cutoff_gen = e.cutoff_out * e.ufac;
    x.roll = pr.bandlimit_roll_hz;
    x.stretch = e.stretch;
    x.tilt_alpha = c.tilt_alpha;
    x.env_tau = c.env_tau;
    x.warp_power = pr.nl_warp_power;
}

template <class Rec> inline bool same_key(const Rec& a, const Rec& b) {
    using genshare::bits_of;
    return a.ops == b.ops && a.n == b.n && a.gen_sr == b.gen_sr && bits_of(a.cutoff_gen) == bits_of(b.cutoff_gen) &&
           bits_of(a.roll) == bits_of(b.roll) && bits_of(a.stretch) == bits_of(b.stretch) &&
           bits_of(a.tilt_alpha) == bits_of(b.tilt_alpha) && bits_of(a.env_tau) == bits_of(b.env_tau) &&
           bits_of(a.warp_power) == bits_of(b.warp_power);
}

// Kernel routes: the class of kernel an event alone would run (stage_event_records).
enum : int8_t { ROUTE_COPY = 0, ROUTE_RUNTIME = 1, ROUTE_SPEC3 = 2, ROUTE_CT = 3 /* + plan */ };

// Where the spectral kernels are not linked (the debug hook, the host-only build): the
// route is a function of the key's fields and, for k_spec3's length, of the parity of the
// event's grain offset and its micro offset (spec3_eligible), so the parity stands in.
inline int8_t route_standin(int32_t ops, int32_t n, int64_t grain_off, int64_t micro_off) {
    if (!ops) return ROUTE_COPY;
    return (int8_t)(ROUTE_RUNTIME + (n == SPEC3_N ? ((grain_off | micro_off) & 1) : 0));
}

struct Scratch {
    std::vector<int32_t> head;   // per generator-owner slot: the newest spectral owner of its grain
    std::vector<int32_t> next;   // per spectral-owner slot: the next owner of the same grain, -1 = none
};

// owner[slot] for every event of the presets list[0, L), as genshare::assign: the slot
// of the first event in list order with the same spectral key, the event's own slot when
// it runs itself.  rec[slot]: the key's fields and mlast_off; route[slot]: the kernel
// route; gen_owner: genshare::assign's result.  share == false: every event runs.
// Returns the number of events that run.
template <class Rec>
inline int64_t assign(const Rec* rec, const int8_t* route, const int32_t* gen_owner, const int32_t* list, int L,
                      const int32_t* slot_base, const int32_t* n_events, int64_t nslots, bool share,
                      int32_t* owner, Scratch& S) {
    int64_t runs = 0;
    if (!share) {
        for (int i = 0; i < L; ++i)
            for (int32_t k = 0, s = slot_base[list[i]]; k < n_events[list[i]]; ++k) owner[s + k] = s + k;
        for (int i = 0; i < L; ++i) runs += n_events[list[i]];
        return runs;
    }
    if (S.head.size() < (size_t)nslots) { S.head.resize((size_t)nslots); S.next.resize((size_t)nslots); }
    int32_t* const head = S.head.data();
    int32_t* const next = S.next.data();
    for (int i = 0; i < L; ++i) {
        const int p = list[i];
        for (int32_t k = 0, s = slot_base[p]; k < n_events[p]; ++k) {
            const int32_t e = s + k, g = gen_owner[e];
            owner[e] = e;
            ++runs;
            if (g == e) {                    // the grain's first event: a new chain, no lookup
                head[e] = e;
                next[e] = -1;
                continue;
            }
            int32_t o = head[g];
            while (o >= 0 && !(route[o] == route[e] && same_key(rec[o], rec[e]))) o = next[o];
            if (o < 0) {                     // a new parameter set of the grain
                next[e] = head[g];
                head[g] = e;
            } else if (rec[e].mlast_off < 0) {
                owner[e] = o;
                --runs;
            }
        }
    }
    return runs;
}

}  // namespace specshare
