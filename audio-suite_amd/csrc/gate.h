// gate.h — the delivery gate (msg_gate_apply / msg_gate_host): a downward expander with
// hysteresis, a hold and straight-line ramps in dB.  The definition, shared by the device kernels
// (kernels_gate.h), the entry points in signal_abi.inc and host_abi.inc and the host reference
// below (built into libmsgpu and into the host sanitizer build).  Plain C++.  DESIGN.md "4m. Gate".
// The math (dyn_log2, dyn_exp2), the level and the max-plus algebra (DynSeg, dyn_join, dyn_run,
// dyn_carry) are the compressor's, dynamics.h, unchanged.
//
// Inputs: one signal x of n frames, CH in {1, 2} interleaved float32 channels, linked.  Every
// envelope value is an int64 in [0, 2^40] in units of u = 2^-32 dB.
//
// 1. Level.  p[f] = max over the channels of |x| as a bit pattern (dyn_level).  A NaN or an
//    infinity anywhere leaves the whole signal as it was, state 2.
// 2. State.  p_open is the smallest float32 at or above 10^(threshold_db / 20), p_close the same
//    for threshold_db - hysteresis_db, both formed once per call on the host (gate_level_up).
//    s[f] = 1 if p >= p_open, 0 if p < p_close, else s[f - 1]; s[-1] = 0.  No logarithm decides
//    a state: the comparisons are of bit patterns of non-negative floats.
// 3. Hold.  sh[f] = 1 if s[f - k] = 1 for some 0 <= k <= hold_frames.
// 4. Openness.  RANGE = llround(range_db 2^32), 2^40 for range_db = +inf.  o[f] = RANGE where
//    sh = 1, elsewhere RANGE - r[f]: r = RANGE when ratio = +inf or p = 0, otherwise in float64
//    with contraction off under = threshold_db - (20 log10 2) dyn_log2(p),
//    v = (ratio - 1) under 2^32 + 0.5, r = 0 if !(v >= 1), RANGE if v >= RANGE, else (int64) v.
// 5. Closing (release), forward.   F[f] = max(F[f - 1] - release_step, o[f]), F[-1] = 0.
// 6. Opening (attack), backward.   B[f] = max(B[f + 1] - attack_step, o[f]),  B[n] = 0.
// 7. Envelope.  O = max(F, B) >= o, E = RANGE - O: a frame whose held state is open has E = 0.
// 8. Gain.  g = dyn_gain(E, 0), exactly 1 for E = 0 (the frame is not written), and 0 for
//    E = 2^40 (only range_db = +inf reaches it); y = x g in float32, in place.
//
// The state and the hold are one integer per frame, the age a[f]: the frames since the last frame
// with s = 1, saturated at hold_frames + 1; a[-1] = hold_frames + 1.  s[f] = 1 exactly when
// a[f] = 0, sh[f] = 1 exactly when a[f] <= hold_frames.  A frame acts on the age that enters it as
//     O (p >= p_open):   a -> 0
//     C (p <  p_close):  a -> min(a + 1, hold_frames + 1)
//     N (neither):       a -> a = 0 ? 0 : min(a + 1, hold_frames + 1)
// and a run of L frames acts as a -> (fixed || a = 0) ? K : min(a + L, hold_frames + 1)
// (GateSeg): with an O inside the result is fixed, K the age the run's tail leaves; with only C
// and N inside an open state stays open up to the first C, K = the frames from that C on, and a
// closed one grows by L; with only N inside K = 0.  Two runs in a row compose to another GateSeg
// (gate_join), exactly and associatively, so the ages may be scanned per lane chunk, per wave,
// per tile and over tiles in any grouping; steps 5 and 6 are the compressor's recurrences over o.
// Everything is integer, so the device's result is the sequential loop's below, bit for bit, for
// any tiling and any batch.
//
// Record (msg_gate_rec), integers only: max_e, sum_e16 = sum over frames of E >> 16,
// reduced_frames = frames with E > 0, open_frames = frames with sh = 1, opens = frames with
// sh[f] = 1 and sh[f - 1] = 0 (sh[-1] = 0); state 0 no frame reduced, 1 gated, 2 non-finite;
// hold_frames.
#pragma once
#include "dynamics.h"

struct GateRec {                                // layout of msg_gate_rec
    int64_t max_e, sum_e16, reduced_frames, open_frames, opens;
    int32_t state, hold_frames;
};
struct GateOpts {                               // layout of msg_gate_opts
    double threshold_db, hysteresis_db, ratio, range_db;
    int64_t attack_step, release_step;
    int32_t hold_frames, flags;
};
// what the kernels take by value
struct GatePar {
    double thr, slope;                          // slope = ratio - 1; unused when hard
    int64_t range, astep, rstep;
    uint32_t open_bits, close_bits;             // p_open and p_close as bit patterns
    int32_t hold;
    int32_t hard;                               // ratio = +inf: r = RANGE
    int32_t local;                              // no hysteresis and no hold: the state is the frame's own
};
// a run of frames as it acts on the age that enters it
struct GateSeg {
    int64_t L, K;
    int32_t fixed;
};

enum : int { GATE_N = 0, GATE_O = 1, GATE_C = 2 };

MSG_HD int gate_class(uint32_t p_bits, const GatePar& par) {
    return p_bits >= par.open_bits ? GATE_O : (p_bits < par.close_bits ? GATE_C : GATE_N);
}
MSG_HD int64_t gate_sat(int64_t a, int32_t hold) { return a > (int64_t)hold + 1 ? (int64_t)hold + 1 : a; }
// one frame
MSG_HD int64_t gate_age(int64_t a, int cls, int32_t hold) {
    if (cls == GATE_O || (cls == GATE_N && a == 0)) return 0;
    return gate_sat(a + 1, hold);
}
MSG_HD GateSeg gate_frame(int cls) { return GateSeg{1, cls == GATE_C ? 1 : 0, cls == GATE_O ? 1 : 0}; }
// a through a run
MSG_HD int64_t gate_through(const GateSeg& s, int64_t a, int32_t hold) {
    return (s.fixed || a == 0) ? s.K : gate_sat(a + s.L, hold);
}
// the run `first` followed by the run `then`; {0, 0, 0} is the empty run
MSG_HD GateSeg gate_join(const GateSeg& first, const GateSeg& then, int32_t hold) {
    if (then.fixed) return GateSeg{first.L + then.L, then.K, 1};
    return GateSeg{first.L + then.L, first.K == 0 ? then.K : gate_sat(first.K + then.L, hold), first.fixed};
}
// a run of cl frames with classes c[0 .. cl)
MSG_HD GateSeg gate_run(const int* c, int cl, int32_t hold) {
    GateSeg s{0, 0, 0};
    for (int k = 0; k < cl; ++k) s = gate_join(s, gate_frame(c[k]), hold);
    return s;
}

// r of step 4 from the level's bit pattern (finite)
MSG_HD int64_t gate_reduction(uint32_t p_bits, const GatePar& par) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (par.hard || p_bits == 0 || p_bits >= DYN_INF) return par.range;
    const double under = par.thr - 6.020599913279624 * dyn_log2(dyn_float(p_bits));
    const double v = par.slope * under * 4294967296.0 + 0.5;
    if (!(v >= 1.0)) return 0;
    return v >= (double)par.range ? par.range : (int64_t)v;
}
// o of step 4
MSG_HD int64_t gate_openness(bool held_open, uint32_t p_bits, const GatePar& par) {
    return held_open ? par.range : par.range - gate_reduction(p_bits, par);
}
// step 8
MSG_HD float gate_gain(int64_t e) { return e >= DYN_MAX ? 0.0f : dyn_gain(e, 0.0); }

// the smallest float32 at or above 10^(db / 20)
inline float gate_level_up(double db) {
    const double lin = std::pow(10.0, db / 20.0);
    float p = (float)lin;
    if ((double)p < lin) p = std::nextafterf(p, INFINITY);
    return p;
}
// nullptr, or why the options are refused
inline const char* gate_refused(const GateOpts& o) {
    if (o.flags != 0) return "flags must be 0";
    if (!std::isfinite(o.threshold_db) || o.threshold_db < -150.0 || o.threshold_db > 24.0)
        return "the threshold must be a finite number of dB from -150 to 24";
    if (!std::isfinite(o.hysteresis_db) || o.hysteresis_db < 0.0 || o.hysteresis_db > 48.0)
        return "the hysteresis must be a finite number of dB from 0 to 48";
    if (!(o.ratio >= 1.0)) return "the ratio must be at least 1";
    if (!(o.range_db > 0.0) || (o.range_db > 240.0 && !std::isinf(o.range_db)))
        return "the range must be a number of dB above 0 up to 240, or infinite";
    if (o.attack_step < 1 || o.attack_step > DYN_MAX || o.release_step < 1 || o.release_step > DYN_MAX)
        return "the attack and release steps must lie in 1 .. 2^40";
    if (o.hold_frames < 0) return "the hold must be a frame count from 0 up";
    return nullptr;
}
inline GatePar gate_par(const GateOpts& o) {
    GatePar par;
    par.thr = o.threshold_db;
    par.hard = std::isinf(o.ratio) ? 1 : 0;
    par.slope = par.hard ? 0.0 : o.ratio - 1.0;
    par.range = std::isinf(o.range_db) ? DYN_MAX : (int64_t)std::llround(o.range_db * 4294967296.0);
    par.astep = o.attack_step;
    par.rstep = o.release_step;
    par.open_bits = dyn_abs_bits(gate_level_up(o.threshold_db));
    par.close_bits = dyn_abs_bits(gate_level_up(o.threshold_db - o.hysteresis_db));
    par.hold = o.hold_frames;
    par.local = (o.hysteresis_db == 0.0 && o.hold_frames == 0) ? 1 : 0;
    return par;
}
MSG_HD void gate_finish(int64_t max_e, int64_t sum_e16, int64_t reduced, int64_t open_frames, int64_t opens,
                        const GatePar& par, GateRec* rec) {
    rec->max_e = max_e;
    rec->sum_e16 = sum_e16;
    rec->reduced_frames = reduced;
    rec->open_frames = open_frames;
    rec->opens = opens;
    rec->state = reduced > 0 ? 1 : 0;
    rec->hold_frames = par.hold;
}

// ---- the host reference: the definition as one sequential loop, x gated in place ----
// env: null, or n words that get E; held: null, or n bytes that get sh (both also for a
// non-finite signal, whose samples stay)
inline void gate_host(float* x, int channels, int64_t n, const GatePar& par, GateRec* rec, int64_t* env = nullptr,
                      uint8_t* held = nullptr) {
    gate_finish(0, 0, 0, 0, 0, par, rec);
    if (n <= 0) return;
    std::vector<int64_t> o((size_t)n), e((size_t)n);
    std::vector<uint8_t> sh((size_t)n);
    bool bad = false;
    int64_t a = (int64_t)par.hold + 1;
    for (int64_t f = 0; f < n; ++f) {
        const uint32_t p = dyn_level(x + f * channels, channels);
        bad = bad || p >= DYN_INF;
        a = gate_age(a, gate_class(p, par), par.hold);
        sh[(size_t)f] = a <= par.hold ? 1 : 0;
        o[(size_t)f] = gate_openness(sh[(size_t)f] != 0, p, par);
    }
    int64_t y = 0;
    for (int64_t f = 0; f < n; ++f) e[(size_t)f] = y = dyn_step(y, par.rstep, o[(size_t)f]);
    y = 0;
    for (int64_t f = n - 1; f >= 0; --f) {
        y = dyn_step(y, par.astep, o[(size_t)f]);
        e[(size_t)f] = par.range - dyn_max(e[(size_t)f], y);
    }
    if (env) std::memcpy(env, e.data(), (size_t)n * 8);
    if (held) std::memcpy(held, sh.data(), (size_t)n);
    if (bad) {
        rec->state = 2;
        return;
    }
    int64_t max_e = 0, sum = 0, reduced = 0, open_frames = 0, opens = 0;
    for (int64_t f = 0; f < n; ++f) {
        const int64_t v = e[(size_t)f];
        max_e = dyn_max(max_e, v);
        sum += v >> 16;
        reduced += v > 0 ? 1 : 0;
        open_frames += sh[(size_t)f];
        opens += (sh[(size_t)f] && !(f > 0 && sh[(size_t)(f - 1)])) ? 1 : 0;
        const float g = gate_gain(v);
        if (dyn_is_one(g)) continue;
        for (int c = 0; c < channels; ++c) x[f * channels + c] = x[f * channels + c] * g;
    }
    gate_finish(max_e, sum, reduced, open_frames, opens, par, rec);
}
