// C ABI, radiance queries (include/frayhip.h "radiance queries"): frayhip_shade_rays and frayhip_shade_rays_device.  Argument checks, the scene's
// kernel flag word and the `rendering` guard; the kernels and the batch loop are shade_impl<ST> of shade_variant.hip (one object per flag word).
// Stands behind trace(ray, rnd), main.cpp:286-293, and the integrator that debugRayTrace fires through a clicked pixel (main.cpp:426-435).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "shade.hpp"

namespace {

using namespace frayhip_detail;

const char* const kWho = "frayhip_shade_rays";

// Every check of both entries, in this order (the scene last); none touches the device.  `device`: the pointers are device memory (alignment is checked)
int check(frayhip_scene* s, int64_t n, const double* org, const double* dir, const frayhip_shade_request* r, const float* rgb, bool device)
{
    if (!r) return bad(kWho, "null request");
    if (!rgb) return bad(kWho, "null rgb");
    if (n < 0 || n > INT32_MAX) return bad(kWho, "n must be 0..INT32_MAX");
    if (n > 0 && (!org || !dir)) return bad(kWho, "null input array");
    if (r->spp < 1) return bad(kWho, "spp must be >= 1");
    if (r->sample_first < 0) return bad(kWho, "sample_first must be >= 0");
    if ((int64_t)r->sample_first + r->spp > INT32_MAX) return bad(kWho, "sample_first + spp overflows");
    if (r->rng_skip < 0 || r->rng_skip > 8) return bad(kWho, "rng_skip must be 0..8");
    if (device) {
        if (misaligned(org, 8) || misaligned(dir, 8)) return bad(kWho, "device pointer to doubles not 8-byte aligned");
        if (misaligned(r->keys, 4) || misaligned(rgb, 4)) return bad(kWho, "device pointer to keys / rgb not 4-byte aligned");
    }
    if (!s) return bad(kWho, "null scene");
    if (s->rendering) return bad(kWho, "the scene is rendering a frame (a query from inside its progress callback?)");
    return FRAYHIP_OK;
}

// The scene's flag word with the counting bit from the request; the stream is drained on every return.
int run(frayhip_scene* s, const ShadeCall& q, hipStream_t stream, frayhip_stats* st)
{
    Busy busy(s, stream);
    return for_flag_word(flag_word(s, q.stats), [&](auto w) { return shade_impl<decltype(w)::value>(s, q, stream, st); });
}

ShadeCall call_of(int64_t n, const double* org, const double* dir, const uint32_t* keys, const frayhip_shade_request* r, float* rgb)
{
    return ShadeCall{(int)n, org, dir, keys, r->seed, r->spp, r->sample_first, r->rng_skip, (r->flags & FRAYHIP_FRAME_STATS) != 0, rgb};
}

}  // namespace

extern "C" {

int frayhip_shade_rays_device(frayhip_scene* s, int64_t n, const double* d_origin, const double* d_dir, const frayhip_shade_request* r, float* d_rgb,
                              void* hip_stream, frayhip_stats* st)
{
    if (const int rc = check(s, n, d_origin, d_dir, r, d_rgb, true)) return rc;
    if (n == 0) return no_work(st);
    return run(s, call_of(n, d_origin, d_dir, r->keys, r, d_rgb), (hipStream_t)hip_stream, st);
}

int frayhip_shade_rays(frayhip_scene* s, int64_t n, const double* origin, const double* dir, const frayhip_shade_request* r, float* rgb, frayhip_stats* st)
{
    if (const int rc = check(s, n, origin, dir, r, rgb, false)) return rc;
    if (n == 0) return no_work(st);
    const size_t N = (size_t)n;
    // one allocation: origins, directions, colours, keys
    DeviceArrays B(std::string(kWho) + ": out of device memory");
    unsigned char* base;
    if (const int rc = B.alloc(base, N * (48 + 12 + (r->keys ? 4 : 0)))) return rc;
    double* d_in = (double*)base;
    float* d_rgb = (float*)(d_in + 6 * N);
    uint32_t* d_keys = r->keys ? (uint32_t*)(d_rgb + 3 * N) : nullptr;
    HIP_TRY(hipMemcpy(d_in, origin, 24 * N, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_in + 3 * N, dir, 24 * N, hipMemcpyHostToDevice));
    if (d_keys) HIP_TRY(hipMemcpy(d_keys, r->keys, 4 * N, hipMemcpyHostToDevice));
    if (const int rc = run(s, call_of(n, d_in, d_in + 3 * N, d_keys, r, d_rgb), nullptr, st)) return rc;
    HIP_TRY(hipMemcpy(rgb, d_rgb, 12 * N, hipMemcpyDeviceToHost));
    return FRAYHIP_OK;
}

}  // extern "C"
