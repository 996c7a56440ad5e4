// host_san.cpp — host-only build of libmsgpu's host entry points for the
// sanitizers (SURVEY §5 "race detection / sanitizers"): the render plan
// (plan.h, msg_plan_host), the NumPy stream primitives (nprng.h, msg_rng_*) and
// the host references of the render digest (digest.h, msg_digest_host) and of the
// loudness and true-peak measurements (loudness.h, msg_loudness_host; truepeak.h,
// msg_truepeak_host), of the PCM quantiser (pcm.h, msg_quantize_host) and of the
// look-ahead limiter (limit.h, msg_limit_host), of the edges pass (edges.h, msg_edges_host) and of the
// stereo meter and image (image.h, msg_stereo_meter_host, msg_stereo_host) and of the compressor
// (dynamics.h, msg_dynamics_host), of the gate (gate.h, msg_gate_host) and of the FLAC encoder (flac.h,
// msg_flac_host),
// compiled by g++ with -fsanitize=address,undefined into
// msgpu/libmsgpu_hostsan.so.  The device entry points are stubs that fail with
// MSG_E_DEVICE, so the ctypes binding (_lib.py) loads this library unchanged
// and tests/test_plan_host.py / tests/test_rng_host.py run against it
// (tests/test_host_sanitizers.py).  Never the product library.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "msg_common.h"
#include "ziggurat_tables.h"
#include "nprng.h"
#include "plan.h"
#include "gen_share.h"
#include "host_pool.h"
#include "digest.h"
#include "loudness.h"
#include "lrange.h"
#include "truepeak.h"
#include "pcm.h"
#include "pcm_shape.h"
#include "limit.h"
#include "edges.h"
#include "filter.h"
#include "image.h"
#include "dynamics.h"
#include "gate.h"
#include "flac.h"
#include "../../include/msgpu.h"

namespace {
const nprng::Zig kHostZig = {zig_ki_double, zig_wi_double, zig_fi_double,
                             zig_ke_double, zig_we_double, zig_fe_double};
thread_local std::string g_err;
int fail(msg_ctx*, int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int no_device() { return fail(nullptr, MSG_E_DEVICE, "host sanitizer build: no device entry points"); }
}  // namespace

extern "C" {
int msg_abi_version(void) { return MSG_ABI_VERSION; }
int msg_host_threads(void) { return HostPool::get().threads(); }
const char* msg_last_error(msg_ctx*) { return g_err.c_str(); }
msg_ctx* msg_create(int) { no_device(); return nullptr; }
void msg_destroy(msg_ctx*) {}
int msg_render_batch(msg_ctx*, const msg_preset*, int32_t, const double*, int64_t, const double* const*,
                     const int64_t*, int32_t,
                     const uint8_t* const*, const int32_t*, const int32_t*, int32_t, float*, const int64_t*, void*) {
    return no_device();
}
int msg_last_plan(msg_ctx*, msg_plan_info*, int32_t) { return no_device(); }
int msg_last_events(msg_ctx*, int32_t, msg_event*, int32_t, int32_t*) { return no_device(); }
int msg_last_meta(msg_ctx*, int32_t, double*, double*, int64_t, int64_t*) { return no_device(); }
int msg_last_grain64(msg_ctx*, int32_t, int32_t, double*, int64_t, int64_t*) { return no_device(); }
int msg_last_spec_routes(msg_ctx*, int64_t*, int32_t) { return no_device(); }
int msg_set_profiling(msg_ctx*, int32_t) { return no_device(); }
int msg_stage_times(msg_ctx*, float*, int32_t) { return no_device(); }
int msg_gate(msg_ctx*, msg_ctx*, int32_t, int32_t) { return no_device(); }
int msg_bench_fft(msg_ctx*, int32_t, int32_t, int32_t, float*) { return no_device(); }
int msg_fft64(msg_ctx*, int32_t, int32_t, const double*, double*) { return no_device(); }
int msg_fir(msg_ctx*, const float*, float*, int64_t, int32_t, const double*, int64_t, int32_t*, void*) {
    return no_device();
}
int msg_stft_mag_db(msg_ctx*, const void*, int32_t, int64_t, int32_t, int32_t, int32_t, int32_t, double*, int32_t*,
                    void*) {
    return no_device();
}
int msg_digest(msg_ctx*, const float*, const int64_t*, const int64_t*, int32_t, msg_digest_rec*, void*) {
    return no_device();
}
int msg_resample(msg_ctx*, const float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, const double*,
                 int64_t, float*, const int64_t*, void*) {
    return no_device();
}
int msg_loudness(msg_ctx*, const float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, msg_loudness_rec*,
                 void*) {
    return no_device();
}
int msg_loudness_range(msg_ctx*, const float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t,
                       msg_loudness_rec*, msg_lrange_rec*, double*, const int64_t*, void*) {
    return no_device();
}
int msg_loudness_gain(msg_ctx*, float*, int32_t, const int64_t*, const int64_t*, int32_t, msg_loudness_rec*, double,
                      double, void*) {
    return no_device();
}
int msg_truepeak(msg_ctx*, const float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, msg_truepeak_rec*,
                 void*) {
    return no_device();
}
int msg_truepeak_gain(msg_ctx*, float*, int32_t, const int64_t*, const int64_t*, int32_t, msg_loudness_rec*,
                      msg_truepeak_rec*, double, double, double, void*) {
    return no_device();
}
int msg_quantize(msg_ctx*, const float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, uint64_t,
                 const uint64_t*, void*, const int64_t*, msg_pcm_rec*, void*) {
    return no_device();
}
int msg_quantize_shaped(msg_ctx*, const float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, int32_t,
                        uint64_t, const uint64_t*, void*, const int64_t*, msg_pcm_rec*, void*) {
    return no_device();
}
int msg_limit(msg_ctx*, float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, double, int32_t,
              const msg_truepeak_rec*, msg_limit_rec*, void*) {
    return no_device();
}
int msg_edges(msg_ctx*, float*, int32_t, const int64_t*, const int64_t*, int32_t, const msg_edges_opts*, msg_edges_rec*,
              void*) {
    return no_device();
}
int msg_filter(msg_ctx*, float*, int32_t, const int64_t*, const int64_t*, int32_t, const msg_filter_opts*, void*) {
    return no_device();
}
int msg_stereo_meter(msg_ctx*, const float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, msg_stereo_rec*,
                     void*) {
    return no_device();
}
int msg_stereo(msg_ctx*, float*, int32_t, const int64_t*, const int64_t*, int32_t, const float*, const float*, float*,
               const int64_t*, const msg_stereo_rec*, void*) {
    return no_device();
}
int msg_dynamics(msg_ctx*, float*, int32_t, const int64_t*, const int64_t*, int32_t, const msg_dynamics_opts*,
                 msg_dynamics_rec*, void*) {
    return no_device();
}
int msg_gate_apply(msg_ctx*, float*, int32_t, const int64_t*, const int64_t*, int32_t, const msg_gate_opts*, msg_gate_rec*,
                   void*) {
    return no_device();
}
int msg_flac(msg_ctx*, const void*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, int32_t, int32_t, void*,
             int64_t, msg_flac_rec*, void*) {
    return no_device();
}
#include "host_abi.inc"
}  // extern "C"
