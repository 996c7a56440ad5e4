// dynamics_check.cpp — csrc/dynamics.h in a stand-alone program for AddressSanitizer and UBSan
// (tests/test_dynamics_host.py builds and runs it).  Every case is evaluated twice: with the
// sequential host loop (dyn_host), and tile by tile through the MSG_HD helpers the kernels use
// (dyn_run per lane chunk, dyn_join over chunks and over tiles in several groupings, dyn_carry
// for the carries), at tile sizes 16, 4096 and one that divides no length, in place as the kernels
// work: the second sweep forms a tile's demands from the buffer as it lies there, with the tiles
// before it or after it already overwritten, and takes the hold's halo from what the first sweep
// saved.  The program exits
// non-zero unless the envelope, the samples and the record are equal in every case: this is
// where the scan algebra is proved on the CPU.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "dynamics.h"

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

// One tile as a workgroup forms it: the demands of its own frames from the samples as they lie in x
// now, the demands of the `hold` frames before it either from the samples too (sweep 1, which saves
// them in `saved`) or from `saved` (sweep 2), and dh by doubling shifts over halo + tile.
static void form_tile(const float* x, int channels, int64_t f0, int64_t lt, const DynPar& par, int64_t* saved, bool from_saved,
                      std::vector<int64_t>& d, std::vector<int64_t>& dh, bool* nonfinite) {
    const int64_t H = par.hold;
    std::vector<int64_t> w((size_t)(H + lt));
    for (int64_t j = 0; j < H; ++j) {
        if (!from_saved) {
            const int64_t f = f0 - H + j;
            saved[j] = f >= 0 ? dyn_demand(dyn_level(x + f * channels, channels), par) : 0;
        }
        w[(size_t)j] = saved[j];
    }
    for (int64_t k = 0; k < lt; ++k) {
        const uint32_t p = dyn_level(x + (f0 + k) * channels, channels);
        if (nonfinite) *nonfinite = *nonfinite || p >= DYN_INF;
        w[(size_t)(H + k)] = dyn_demand(p, par);
    }
    d.assign(w.begin() + H, w.end());
    for (int64_t have = 1; have < H + 1;) {
        const int64_t s = std::min<int64_t>(have, H + 1 - have);
        for (int64_t i = H + lt - 1; i >= s; --i) w[(size_t)i] = dyn_max(w[(size_t)i], w[(size_t)(i - s)]);
        have += s;
    }
    dh.assign(w.begin() + H, w.end());
}

// the tiled evaluation: what the three kernels do, on the host and in place.  Sweep 2 takes the
// tiles in ascending or descending order: a tile before or after this one has then already been
// overwritten with its output, as another workgroup of the launch may have done on the device.
static void tiled(float* x, int channels, int64_t n, const DynPar& par, int64_t tile, bool ascending, DynRec* rec, int64_t* env) {
    dyn_finish(0, 0, 0, false, par, rec);
    if (n <= 0) return;
    const int64_t T = (n + tile - 1) / tile, H = par.hold;
    std::vector<int64_t> d, dh, cf((size_t)T), cb((size_t)T), fin((size_t)T), bin((size_t)T), len((size_t)T);
    std::vector<int64_t> halo((size_t)(T * H) + 1);
    bool nonfinite = false;
    // sweep 1: the tile's two summaries from its lane chunks; nothing is written to x
    for (int64_t t = 0; t < T; ++t) {
        const int64_t f0 = t * tile, lt = std::min(tile, n - f0);
        len[(size_t)t] = lt;
        form_tile(x, channels, f0, lt, par, halo.data() + t * H, false, d, dh, &nonfinite);
        DynSeg sf{0, 0}, sb{0, 0};
        for (int64_t c0 = 0; c0 < lt; c0 += DYN_C) {        // chunks in order; the attack joins them from the last
            const int cl = (int)std::min<int64_t>(DYN_C, lt - c0);
            sf = dyn_join(sf, dyn_run(dh.data() + c0, cl, par.rstep, false));
        }
        for (int64_t c0 = (lt - 1) / DYN_C * DYN_C; c0 >= 0; c0 -= DYN_C) {
            const int cl = (int)std::min<int64_t>(DYN_C, lt - c0);
            sb = dyn_join(sb, dyn_run(d.data() + c0, cl, par.astep, true));
        }
        CHECK(sf.R == dyn_span(lt, par.rstep) && sb.R == dyn_span(lt, par.astep), "tile %lld: the runs' lengths", (long long)t);
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
            CHECK(dyn_carry(blk, c) == fin[(size_t)u], "tile %lld: the grouped release carry", (long long)u);
            blk = dyn_join(blk, DynSeg{dyn_span(len[(size_t)u], par.rstep), cf[(size_t)u]});
        }
        c = dyn_carry(blk, c);
    }
    c = 0;
    for (int64_t t = T - 1; t >= 0; t -= 3) {
        DynSeg blk{0, 0};
        for (int64_t u = t; u > std::max<int64_t>(-1, t - 3); --u) {
            CHECK(dyn_carry(blk, c) == bin[(size_t)u], "tile %lld: the grouped attack carry", (long long)u);
            blk = dyn_join(blk, DynSeg{dyn_span(len[(size_t)u], par.astep), cb[(size_t)u]});
        }
        c = dyn_carry(blk, c);
    }
    // sweep 2: every tile from its carries, its own demands from x as it lies there now
    int64_t max_e = 0, sum = 0, reduced = 0;
    for (int64_t i = 0; i < T; ++i) {
        const int64_t t = ascending ? i : T - 1 - i, f0 = t * tile, lt = len[(size_t)t];
        form_tile(x, channels, f0, lt, par, halo.data() + t * H, true, d, dh, nullptr);
        int64_t y = fin[(size_t)t];
        for (int64_t k = 0; k < lt; ++k) env[f0 + k] = y = dyn_step(y, par.rstep, dh[(size_t)k]);
        y = bin[(size_t)t];
        for (int64_t k = lt - 1; k >= 0; --k) {
            y = dyn_step(y, par.astep, d[(size_t)k]);
            env[f0 + k] = dyn_max(env[f0 + k], y);
        }
        if (nonfinite) continue;
        for (int64_t f = f0; f < f0 + lt; ++f) {
            max_e = dyn_max(max_e, env[f]);
            sum += env[f] >> 16;
            reduced += env[f] > 0 ? 1 : 0;
            const float g = dyn_gain(env[f], par.makeup);
            if (dyn_is_one(g)) continue;
            for (int ch = 0; ch < channels; ++ch) x[f * channels + ch] = x[f * channels + ch] * g;
        }
    }
    if (nonfinite) rec->state = 2;
    else dyn_finish(max_e, sum, reduced, true, par, rec);
}

static void one_case(const char* name, const std::vector<float>& x, int channels, const DynOpts& o) {
    CHECK(dyn_refused(o) == nullptr, "%s: refused: %s", name, dyn_refused(o) ? dyn_refused(o) : "");
    const DynPar par = dyn_par(o);
    const int64_t n = (int64_t)x.size() / channels;
    // exactly-sized heap blocks: a read or write one element out is the sanitizer's
    std::unique_ptr<float[]> a(new float[x.size()]);
    std::unique_ptr<int64_t[]> ea(new int64_t[(size_t)n]);
    std::copy(x.begin(), x.end(), a.get());
    DynRec ra;
    dyn_host(a.get(), channels, n, par, &ra, ea.get());
    const int64_t tiles[3] = {16, DYN_TILE, 1000};
    for (const int64_t tile : tiles) {
        if (tile == 16 && par.hold > 256) continue;         // a halo of 256 tiles a tile: the same code, only slow
        for (const bool ascending : {true, false}) {
            std::unique_ptr<float[]> b(new float[x.size()]);
            std::unique_ptr<int64_t[]> eb(new int64_t[(size_t)n]);
            std::copy(x.begin(), x.end(), b.get());
            DynRec rb;
            tiled(b.get(), channels, n, par, tile, ascending, &rb, eb.get());
            const long long tl = (long long)tile;
            CHECK(std::memcmp(ea.get(), eb.get(), (size_t)n * 8) == 0, "%s, tile %lld, ascending %d: the envelope", name, tl, ascending);
            CHECK(std::memcmp(a.get(), b.get(), x.size() * 4) == 0, "%s, tile %lld, ascending %d: the samples", name, tl, ascending);
            CHECK(std::memcmp(&ra, &rb, sizeof(ra)) == 0, "%s, tile %lld, ascending %d: the record", name, tl, ascending);
        }
    }
    for (int64_t f = 0; f < n; ++f) CHECK(ea[(size_t)f] >= 0 && ea[(size_t)f] <= DYN_MAX, "%s: E out of range", name);
    std::printf("%-34s n %6lld ch %d  max_e %.4f dB  reduced %lld  state %d\n", name, (long long)n, channels,
                (double)ra.max_e / 4294967296.0, (long long)ra.reduced_frames, ra.state);
}

static std::vector<float> texture(int64_t n, int channels) {
    std::vector<float> x((size_t)(n * channels));
    for (auto& v : x) v = (float)((uniform() - 0.5) * 0.004);
    for (int64_t b = 0; b < std::max<int64_t>(1, n / 700); ++b) {
        const int64_t at = (int64_t)(uniform() * (double)n), ln = 1 + (int64_t)(uniform() * 400.0);
        const double amp = std::pow(10.0, (-36.0 + 33.0 * uniform()) / 20.0);
        for (int64_t f = at; f < std::min(n, at + ln); ++f)
            for (int ch = 0; ch < channels; ++ch) x[(size_t)(f * channels + ch)] = (float)((uniform() * 2.0 - 1.0) * amp);
    }
    return x;
}

int main() {
    static_assert(sizeof(DynRec) == 32 && sizeof(DynOpts) == 56, "the ABI's sizes");
    const int64_t N = 3 * DYN_TILE + 5;
    const int64_t step10 = (int64_t)(10.0 * 4294967296.0 / 24000.0);      // 10 dB in 24000 frames: crosses every tile
    const DynOpts base{-18.0, 3.0, 6.0, 0.0, step10, step10, 0, 0};
    // the math at its pinned points
    CHECK(dyn_exp2(0.0) == 1.0, "dyn_exp2(0) = %.17g", dyn_exp2(0.0));
    CHECK(dyn_log2(1.0f) == 0.0 && dyn_log2(2.0f) == 1.0 && dyn_log2(0.5f) == -1.0, "dyn_log2 at powers of two");
    CHECK(dyn_log2(std::numeric_limits<float>::denorm_min()) == -149.0, "dyn_log2 of the least denormal");
    CHECK(dyn_gain(0, 0.0) == 1.0f && dyn_is_one(dyn_gain(0, 0.0)), "the gain of E = 0");
    CHECK(dyn_span(1 << 30, DYN_MAX) == DYN_MAX && dyn_span(3, 5) == 15 && dyn_span(0, DYN_MAX) == 0, "dyn_span");
    CHECK(dyn_span(DYN_TILE, DYN_MAX / DYN_TILE) == DYN_MAX && dyn_span(DYN_TILE, DYN_MAX / DYN_TILE - 1) < DYN_MAX, "dyn_span at 2^40");

    for (int channels = 1; channels <= 2; ++channels) {
        const std::vector<float> tex = texture(N, channels);
        one_case("texture, release across tiles", tex, channels, base);
        for (const int hold : {1, 100, DYN_HOLD_MAX}) {
            DynOpts o = base;
            o.hold_frames = hold;
            o.release_step = step10 * 50;
            one_case("texture, hold", tex, channels, o);
        }
        {
            DynOpts o = base;
            o.attack_step = o.release_step = DYN_MAX;
            one_case("texture, instant", tex, channels, o);
            o.attack_step = o.release_step = 1;
            one_case("texture, one unit a frame", tex, channels, o);
            o = base;
            o.ratio = std::numeric_limits<double>::infinity();
            o.knee_db = 0.0;
            o.makeup_db = 6.5;
            one_case("texture, ratio inf, hard knee", tex, channels, o);
            o = base;
            o.threshold_db = 24.0;
            o.makeup_db = -3.0;
            one_case("texture, makeup alone", tex, channels, o);
        }
        for (const int64_t at : {(int64_t)0, (int64_t)DYN_TILE - 1, (int64_t)DYN_TILE, N - 1}) {    // a peak at the seams
            std::vector<float> x((size_t)(N * channels), 1e-4f);
            x[(size_t)(at * channels)] = 1.0f;
            one_case("one full-scale frame", x, channels, base);
            DynOpts o = base;
            o.hold_frames = DYN_HOLD_MAX;
            one_case("one full-scale frame, hold 4096", x, channels, o);
        }
        for (const int64_t n : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)DYN_TILE}) {
            std::vector<float> x((size_t)(n * channels), 0.9f);
            one_case("short signals", x, channels, base);
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
        DynOpts o = base;
        o.flags = 1;
        CHECK(dyn_refused(o) != nullptr, "flags");
        o = base; o.threshold_db = 25.0;
        CHECK(dyn_refused(o) != nullptr, "threshold");
        o = base; o.ratio = 0.5;
        CHECK(dyn_refused(o) != nullptr, "ratio");
        o = base; o.ratio = std::numeric_limits<double>::quiet_NaN();
        CHECK(dyn_refused(o) != nullptr, "NaN ratio");
        o = base; o.knee_db = 49.0;
        CHECK(dyn_refused(o) != nullptr, "knee");
        o = base; o.makeup_db = -48.5;
        CHECK(dyn_refused(o) != nullptr, "makeup");
        o = base; o.attack_step = 0;
        CHECK(dyn_refused(o) != nullptr, "attack step");
        o = base; o.release_step = DYN_MAX + 1;
        CHECK(dyn_refused(o) != nullptr, "release step");
        o = base; o.hold_frames = -1;
        CHECK(dyn_refused(o) != nullptr, "hold");
    }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
