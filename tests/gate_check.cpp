// gate_check.cpp — csrc/gate.h in a stand-alone program for AddressSanitizer and UBSan
// (tests/test_gate_host.py builds and runs it).  Every case is evaluated twice: with the sequential
// host loop (gate_host), and tile by tile through the MSG_HD helpers the kernels use (gate_run per
// lane chunk, gate_join over chunks and over tiles, gate_through for the ages that enter; dyn_run,
// dyn_join and dyn_carry for the ramps), at tile sizes 16, 4096 and one that divides no length, the
// carries also grouped three tiles at a time, in place as the kernels work: the apply sweep forms a
// tile's classes from the buffer as it lies there, with the tiles before it or after it already
// overwritten, and reads no sample outside the tile.  The program exits non-zero unless the held
// states, the envelope, the samples and the record are equal in every case: this is where the
// state algebra is proved on the CPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "gate.h"

static int bad = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++bad;                                         \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static double uniform() {                       // xorshift64*, in [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1DULL) >> 11) / 9007199254740992.0;
}

static bool same(const GateSeg& a, const GateSeg& b) { return a.L == b.L && a.K == b.K && a.fixed == b.fixed; }

// the classes of one tile from the samples as they lie in x now, and its transfer from lane chunks
static GateSeg tile_transfer(const float* x, int channels, int64_t f0, int64_t lt, const GatePar& par, std::vector<int>& cls,
                             bool* nonfinite) {
    cls.resize((size_t)lt);
    for (int64_t k = 0; k < lt; ++k) {
        const uint32_t p = dyn_level(x + (f0 + k) * channels, channels);
        if (nonfinite) *nonfinite = *nonfinite || p >= DYN_INF;
        cls[(size_t)k] = gate_class(p, par);
    }
    GateSeg t{0, 0, 0};
    for (int64_t c0 = 0; c0 < lt; c0 += DYN_C)
        t = gate_join(t, gate_run(cls.data() + c0, (int)std::min<int64_t>(DYN_C, lt - c0), par.hold), par.hold);
    return t;
}

// the openness of one tile: the ages from the age that enters it, per lane chunk as the kernel walks
static void tile_openness(const float* x, int channels, int64_t f0, int64_t lt, const GatePar& par, int64_t age_in,
                          std::vector<int64_t>& o, std::vector<uint8_t>& sh) {
    std::vector<int> cls;
    tile_transfer(x, channels, f0, lt, par, cls, nullptr);
    o.resize((size_t)lt);
    sh.resize((size_t)lt);
    GateSeg before{0, 0, 0};
    for (int64_t c0 = 0; c0 < lt; c0 += DYN_C) {
        const int cl = (int)std::min<int64_t>(DYN_C, lt - c0);
        int64_t age = gate_through(before, age_in, par.hold);      // the exclusive scan's value for this chunk
        for (int k = 0; k < cl; ++k) {
            age = gate_age(age, cls[(size_t)(c0 + k)], par.hold);
            sh[(size_t)(c0 + k)] = age <= par.hold ? 1 : 0;
            o[(size_t)(c0 + k)] = gate_openness(age <= par.hold, dyn_level(x + (f0 + c0 + k) * channels, channels), par);
        }
        before = gate_join(before, gate_run(cls.data() + c0, cl, par.hold), par.hold);
        CHECK(gate_through(before, age_in, par.hold) == age, "frame %lld: a chunk's transfer against its walk", (long long)(f0 + c0));
    }
}

// the tiled evaluation: what the five kernels do, on the host and in place.  The apply sweep takes
// the tiles in ascending or descending order: a tile before or after this one has then already been
// overwritten with its output, as another workgroup of the launch may have done on the device.
static void tiled(float* x, int channels, int64_t n, const GatePar& par, int64_t tile, bool ascending, GateRec* rec, int64_t* env,
                  uint8_t* held) {
    gate_finish(0, 0, 0, 0, 0, par, rec);
    if (n <= 0) return;
    const int64_t T = (n + tile - 1) / tile;
    std::vector<int64_t> o, cf((size_t)T), cb((size_t)T), fin((size_t)T), bin((size_t)T), len((size_t)T), ain((size_t)T);
    std::vector<GateSeg> tr((size_t)T);
    std::vector<uint8_t> sh;
    std::vector<int> cls;
    bool nonfinite = false;
    // the state sweep and its scan, one by one and in blocks of three joined first
    for (int64_t t = 0; t < T; ++t) {
        len[(size_t)t] = std::min(tile, n - t * tile);
        tr[(size_t)t] = tile_transfer(x, channels, t * tile, len[(size_t)t], par, cls, &nonfinite);
        CHECK(tr[(size_t)t].L == len[(size_t)t], "tile %lld: the transfer's length", (long long)t);
    }
    int64_t a = (int64_t)par.hold + 1;
    for (int64_t t = 0; t < T; ++t) {
        ain[(size_t)t] = a;
        a = gate_through(tr[(size_t)t], a, par.hold);
    }
    a = (int64_t)par.hold + 1;
    for (int64_t t = 0; t < T; t += 3) {
        GateSeg blk{0, 0, 0};
        for (int64_t u = t; u < std::min(T, t + 3); ++u) {
            CHECK(gate_through(blk, a, par.hold) == ain[(size_t)u], "tile %lld: the grouped age", (long long)u);
            blk = gate_join(blk, tr[(size_t)u], par.hold);
        }
        a = gate_through(blk, a, par.hold);
    }
    // sweep 1: the tile's two summaries from its lane chunks; nothing is written to x
    for (int64_t t = 0; t < T; ++t) {
        const int64_t f0 = t * tile, lt = len[(size_t)t];
        tile_openness(x, channels, f0, lt, par, ain[(size_t)t], o, sh);
        DynSeg sf{0, 0}, sb{0, 0};
        for (int64_t c0 = 0; c0 < lt; c0 += DYN_C)
            sf = dyn_join(sf, dyn_run(o.data() + c0, (int)std::min<int64_t>(DYN_C, lt - c0), par.rstep, false));
        for (int64_t c0 = (lt - 1) / DYN_C * DYN_C; c0 >= 0; c0 -= DYN_C)
            sb = dyn_join(sb, dyn_run(o.data() + c0, (int)std::min<int64_t>(DYN_C, lt - c0), par.astep, true));
        cf[(size_t)t] = sf.C;
        cb[(size_t)t] = sb.C;
    }
    // the scan over tiles, one by one and in blocks of three joined first: the same carries
    int64_t c = 0;
    for (int64_t t = 0; t < T; ++t) {
        fin[(size_t)t] = c;
        c = dyn_carry(DynSeg{dyn_span(len[(size_t)t], par.rstep), cf[(size_t)t]}, c);
    }
    c = 0;
    for (int64_t t = T - 1; t >= 0; --t) {
        bin[(size_t)t] = c;
        c = dyn_carry(DynSeg{dyn_span(len[(size_t)t], par.astep), cb[(size_t)t]}, c);
    }
    c = 0;
    for (int64_t t = 0; t < T; t += 3) {
        DynSeg blk{0, 0};
        for (int64_t u = t; u < std::min(T, t + 3); ++u) {
            CHECK(dyn_carry(blk, c) == fin[(size_t)u], "tile %lld: the grouped closing carry", (long long)u);
            blk = dyn_join(blk, DynSeg{dyn_span(len[(size_t)u], par.rstep), cf[(size_t)u]});
        }
        c = dyn_carry(blk, c);
    }
    c = 0;
    for (int64_t t = T - 1; t >= 0; t -= 3) {
        DynSeg blk{0, 0};
        for (int64_t u = t; u > std::max<int64_t>(-1, t - 3); --u) {
            CHECK(dyn_carry(blk, c) == bin[(size_t)u], "tile %lld: the grouped opening carry", (long long)u);
            blk = dyn_join(blk, DynSeg{dyn_span(len[(size_t)u], par.astep), cb[(size_t)u]});
        }
        c = dyn_carry(blk, c);
    }
    // sweep 2: every tile from the age and the carries that enter it, its classes from x as it lies there now
    int64_t max_e = 0, sum = 0, reduced = 0, open_frames = 0, opens = 0;
    for (int64_t i = 0; i < T; ++i) {
        const int64_t t = ascending ? i : T - 1 - i, f0 = t * tile, lt = len[(size_t)t];
        tile_openness(x, channels, f0, lt, par, ain[(size_t)t], o, sh);
        int64_t y = fin[(size_t)t];
        for (int64_t k = 0; k < lt; ++k) env[f0 + k] = y = dyn_step(y, par.rstep, o[(size_t)k]);
        y = bin[(size_t)t];
        for (int64_t k = lt - 1; k >= 0; --k) {
            y = dyn_step(y, par.astep, o[(size_t)k]);
            env[f0 + k] = par.range - dyn_max(env[f0 + k], y);
        }
        bool prev = ain[(size_t)t] <= par.hold;
        for (int64_t k = 0; k < lt; ++k) {
            held[f0 + k] = sh[(size_t)k];
            if (!nonfinite) {
                open_frames += sh[(size_t)k];
                opens += sh[(size_t)k] && !prev ? 1 : 0;
            }
            prev = sh[(size_t)k] != 0;
        }
        if (nonfinite) continue;
        for (int64_t f = f0; f < f0 + lt; ++f) {
            max_e = dyn_max(max_e, env[f]);
            sum += env[f] >> 16;
            reduced += env[f] > 0 ? 1 : 0;
            const float g = gate_gain(env[f]);
            if (dyn_is_one(g)) continue;
            for (int ch = 0; ch < channels; ++ch) x[f * channels + ch] = x[f * channels + ch] * g;
        }
    }
    if (nonfinite) rec->state = 2;
    else gate_finish(max_e, sum, reduced, open_frames, opens, par, rec);
}

static void one_case(const char* name, const std::vector<float>& x, int channels, const GateOpts& o) {
    CHECK(gate_refused(o) == nullptr, "%s: refused: %s", name, gate_refused(o) ? gate_refused(o) : "");
    const GatePar par = gate_par(o);
    const int64_t n = (int64_t)x.size() / channels;
    // exactly-sized heap blocks: a read or write one element out is the sanitizer's
    std::unique_ptr<float[]> a(new float[x.size()]);
    std::unique_ptr<int64_t[]> ea(new int64_t[(size_t)n]);
    std::unique_ptr<uint8_t[]> ha(new uint8_t[(size_t)n]);
    std::copy(x.begin(), x.end(), a.get());
    GateRec ra;
    gate_host(a.get(), channels, n, par, &ra, ea.get(), ha.get());
    const int64_t tiles[3] = {16, DYN_TILE, 1000};
    for (const int64_t tile : tiles) {
        for (const bool ascending : {true, false}) {
            std::unique_ptr<float[]> b(new float[x.size()]);
            std::unique_ptr<int64_t[]> eb(new int64_t[(size_t)n]);
            std::unique_ptr<uint8_t[]> hb(new uint8_t[(size_t)n]);
            std::copy(x.begin(), x.end(), b.get());
            GateRec rb;
            tiled(b.get(), channels, n, par, tile, ascending, &rb, eb.get(), hb.get());
            const long long tl = (long long)tile;
            CHECK(std::memcmp(ha.get(), hb.get(), (size_t)n) == 0, "%s, tile %lld, ascending %d: the held states", name, tl, ascending);
            CHECK(std::memcmp(ea.get(), eb.get(), (size_t)n * 8) == 0, "%s, tile %lld, ascending %d: the envelope", name, tl, ascending);
            CHECK(std::memcmp(a.get(), b.get(), x.size() * 4) == 0, "%s, tile %lld, ascending %d: the samples", name, tl, ascending);
            CHECK(std::memcmp(&ra, &rb, sizeof(ra)) == 0, "%s, tile %lld, ascending %d: the record", name, tl, ascending);
        }
    }
    for (int64_t f = 0; f < n; ++f) {
        CHECK(ea[(size_t)f] >= 0 && ea[(size_t)f] <= par.range, "%s: E out of range", name);
        CHECK(!ha[(size_t)f] || ea[(size_t)f] == 0, "%s: an open frame attenuated", name);
    }
    std::printf("%-38s n %6lld ch %d  max_e %.4f dB  reduced %lld  open %lld  opens %lld  state %d\n", name, (long long)n, channels,
                (double)ra.max_e / 4294967296.0, (long long)ra.reduced_frames, (long long)ra.open_frames, (long long)ra.opens,
                ra.state);
}

// a bed around -60 dB with bursts between -56 and -20 dB: levels on all three sides of -40 / -46 dB
static std::vector<float> texture(int64_t n, int channels) {
    std::vector<float> x((size_t)(n * channels));
    for (auto& v : x) v = (float)((uniform() - 0.5) * 0.004);
    for (int64_t b = 0; b < std::max<int64_t>(1, n / 700); ++b) {
        const int64_t at = (int64_t)(uniform() * (double)n), ln = 1 + (int64_t)(uniform() * 400.0);
        const double amp = std::pow(10.0, (-56.0 + 36.0 * uniform()) / 20.0);
        for (int64_t f = at; f < std::min(n, at + ln); ++f)
            for (int ch = 0; ch < channels; ++ch) x[(size_t)(f * channels + ch)] = (float)((uniform() * 2.0 - 1.0) * amp);
    }
    return x;
}

// exhaustive over short class strings: the transfer of every split equals the walk, for every entering age
static void algebra() {
    for (const int hold : {0, 1, 3}) {
        for (int len = 0; len <= 7; ++len) {
            int total = 1;
            for (int i = 0; i < len; ++i) total *= 3;
            for (int code = 0; code < total; ++code) {
                int c[8] = {0}, v = code;
                for (int i = 0; i < len; ++i) { c[i] = v % 3; v /= 3; }
                const GateSeg whole = gate_run(c, len, hold);
                for (int cut = 0; cut <= len; ++cut)
                    CHECK(same(gate_join(gate_run(c, cut, hold), gate_run(c + cut, len - cut, hold), hold), whole), "split %d of %d", cut, len);
                for (int64_t a0 = 0; a0 <= hold + 1; ++a0) {
                    int64_t a = a0;
                    for (int i = 0; i < len; ++i) a = gate_age(a, c[i], hold);
                    CHECK(gate_through(whole, a0, hold) == a, "walk: hold %d len %d code %d age %lld", hold, len, code, (long long)a0);
                }
            }
        }
    }
}

int main() {
    static_assert(sizeof(GateRec) == 48 && sizeof(GateOpts) == 56, "the ABI's sizes");
    const double inf = std::numeric_limits<double>::infinity();
    const int64_t N = 3 * DYN_TILE + 5;
    const int64_t step10 = (int64_t)(10.0 * 4294967296.0 / 24000.0);      // 10 dB in 24000 frames: crosses every tile
    const GateOpts base{-40.0, 6.0, inf, 60.0, step10, step10, 0, 0};
    algebra();
    CHECK(gate_gain(0) == 1.0f && dyn_is_one(gate_gain(0)) && gate_gain(DYN_MAX) == 0.0f, "the gain at E = 0 and 2^40");
    CHECK((double)gate_level_up(-40.0) >= 0.01 && (double)std::nextafterf(gate_level_up(-40.0), 0.0f) < 0.01, "p_open");
    CHECK(gate_par(base).range == (int64_t)60 << 32, "RANGE");

    for (int channels = 1; channels <= 2; ++channels) {
        const std::vector<float> tex = texture(N, channels);
        one_case("texture, ramps across tiles", tex, channels, base);
        for (const int hold : {1, 100, 4096, 10000}) {
            GateOpts o = base;
            o.hold_frames = hold;
            o.release_step = step10 * 50;
            one_case("texture, hold", tex, channels, o);
        }
        {
            GateOpts o = base;
            o.hysteresis_db = 0.0;
            one_case("texture, no hysteresis, no hold", tex, channels, o);
            o.hold_frames = 37;
            one_case("texture, hold alone", tex, channels, o);
            o = base;
            o.attack_step = o.release_step = DYN_MAX;
            one_case("texture, instant", tex, channels, o);
            o.attack_step = o.release_step = 1;
            one_case("texture, one unit a frame", tex, channels, o);
            o = base;
            o.ratio = 2.0;
            o.range_db = 24.0;
            one_case("texture, ratio 2", tex, channels, o);
            o = base;
            o.range_db = inf;
            o.release_step = step10 * 400;
            one_case("texture, range inf", tex, channels, o);
            o = base;
            o.threshold_db = -150.0;
            one_case("texture, threshold under all", tex, channels, o);
        }
        for (const int64_t at : {(int64_t)0, (int64_t)DYN_TILE - 1, (int64_t)DYN_TILE, N - 1}) {    // an opener at the seams
            std::vector<float> x((size_t)(N * channels), 1e-4f);
            x[(size_t)(at * channels)] = 1.0f;
            one_case("one opening frame", x, channels, base);
            GateOpts o = base;
            o.hold_frames = 5000;
            one_case("one opening frame, hold 5000", x, channels, o);
        }
        {
            // an opener, more than two tiles between the thresholds, one closing frame
            std::vector<float> x((size_t)(N * channels), 0.007f);
            x[(size_t)(10 * channels)] = 0.5f;
            x[(size_t)((N - 100) * channels + channels - 1)] = 1e-4f;
            if (channels == 2) x[(size_t)((N - 100) * channels)] = 1e-4f;
            one_case("open through N tiles", x, channels, base);
            std::vector<float> z((size_t)(N * channels), 0.007f);       // never opens
            one_case("between the thresholds", z, channels, base);
        }
        for (const int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)DYN_TILE}) {
            std::vector<float> x((size_t)(n * channels), 0.9f);
            one_case("short signals, open", x, channels, base);
            std::vector<float> q((size_t)(n * channels), 1e-5f);
            one_case("short signals, shut", q, channels, base);
        }
        {
            std::vector<float> x = tex;
            x[(size_t)(5000 * channels + channels - 1)] = std::numeric_limits<float>::quiet_NaN();
            one_case("a NaN", x, channels, base);
            x = tex;
            x[(size_t)(123 * channels)] = -std::numeric_limits<float>::infinity();
            one_case("an infinity", x, channels, base);
        }
    }
    // refusals
    {
        GateOpts o = base;
        o.flags = 1;
        CHECK(gate_refused(o) != nullptr, "flags");
        o = base; o.threshold_db = 25.0;
        CHECK(gate_refused(o) != nullptr, "threshold");
        o = base; o.hysteresis_db = -1.0;
        CHECK(gate_refused(o) != nullptr, "hysteresis");
        o = base; o.ratio = 0.5;
        CHECK(gate_refused(o) != nullptr, "ratio");
        o = base; o.ratio = std::numeric_limits<double>::quiet_NaN();
        CHECK(gate_refused(o) != nullptr, "NaN ratio");
        o = base; o.range_db = 0.0;
        CHECK(gate_refused(o) != nullptr, "range 0");
        o = base; o.range_db = 241.0;
        CHECK(gate_refused(o) != nullptr, "range 241");
        o = base; o.range_db = std::numeric_limits<double>::quiet_NaN();
        CHECK(gate_refused(o) != nullptr, "NaN range");
        o = base; o.attack_step = 0;
        CHECK(gate_refused(o) != nullptr, "attack step");
        o = base; o.release_step = DYN_MAX + 1;
        CHECK(gate_refused(o) != nullptr, "release step");
        o = base; o.hold_frames = -1;
        CHECK(gate_refused(o) != nullptr, "hold");
    }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
