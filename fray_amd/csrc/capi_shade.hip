// C ABI, radiance queries (include/frayhip.h "radiance queries"): frayhip_shade_rays and frayhip_shade_rays_device.  Argument checks, the scene's
// kernel flag word and the `rendering` guard; the kernels and the batch loop are shade_impl<ST> of shade_variant.hip (one object per flag word).
// Stands behind trace(ray, rnd), main.cpp:286-293, and the integrator that debugRayTrace fires through a clicked pixel (main.cpp:426-435).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "shade.hpp"

namespace {

using frayhip_detail::set_error;
using frayhip_detail::ShadeCall;

const char* const kWho = "frayhip_shade_rays";

int bad(const std::string& why)
{
    set_error(std::string(kWho) + ": " + why);
    return FRAYHIP_E_ARG;
}
bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// Every check of both entries, in this order (the scene last); none touches the device.  `device`: the pointers are device memory (alignment is checked)
int check(frayhip_scene* s, int64_t n, const double* org, const double* dir, const frayhip_shade_request* r, const float* rgb, bool device)
{
    if (!r) return bad("null request");
    if (!rgb) return bad("null rgb");
    if (n < 0 || n > INT32_MAX) return bad("n must be 0..INT32_MAX");
    if (n > 0 && (!org || !dir)) return bad("null input array");
    if (r->spp < 1) return bad("spp must be >= 1");
    if (r->sample_first < 0) return bad("sample_first must be >= 0");
    if ((int64_t)r->sample_first + r->spp > INT32_MAX) return bad("sample_first + spp overflows");
    if (r->rng_skip < 0 || r->rng_skip > 8) return bad("rng_skip must be 0..8");
    if (device) {
        if (misaligned(org, 8) || misaligned(dir, 8)) return bad("device pointer to doubles not 8-byte aligned");
        if (misaligned(r->keys, 4) || misaligned(rgb, 4)) return bad("device pointer to keys / rgb not 4-byte aligned");
    }
    if (!s) return bad("null scene");
    if (s->rendering) return bad("the scene is rendering a frame (a query from inside its progress callback?)");
    return FRAYHIP_OK;
}

// the flag word the scene was created with (render_dispatch, capi.hip), with the counting bit from the request.  The scene is held as a frame holds
// it (`rendering`), so that nothing re-enters it; on an early return the stream is drained first.
int run(frayhip_scene* s, const ShadeCall& q, hipStream_t stream, frayhip_stats* st)
{
    using namespace frayhip_detail;
    struct Busy {
        frayhip_scene* s;
        hipStream_t stream;
        Busy(frayhip_scene* x, hipStream_t y) : s(x), stream(y) { s->rendering = true; }
        ~Busy() { (void)hipStreamSynchronize(stream); s->rendering = false; }
    } busy(s, stream);
    const int w = (s->extGeometry ? 2 : s->kdMeshes ? 4 : s->textured ? 8 : 0) | (q.stats ? 1 : 0);
    switch (w) {
        case 0: return shade_impl<0>(s, q, stream, st);
        case 1: return shade_impl<1>(s, q, stream, st);
        case 2: return shade_impl<2>(s, q, stream, st);
        case 3: return shade_impl<3>(s, q, stream, st);
        case 4: return shade_impl<4>(s, q, stream, st);
        case 5: return shade_impl<5>(s, q, stream, st);
        case 8: return shade_impl<8>(s, q, stream, st);
        default: return shade_impl<9>(s, q, stream, st);
    }
}

ShadeCall call_of(int64_t n, const double* org, const double* dir, const uint32_t* keys, const frayhip_shade_request* r, float* rgb)
{
    return ShadeCall{(int)n, org, dir, keys, r->seed, r->spp, r->sample_first, r->rng_skip, (r->flags & FRAYHIP_FRAME_STATS) != 0, rgb};
}

int no_work(frayhip_stats* st)
{
    if (st) *st = frayhip_stats{};
    return FRAYHIP_OK;
}

// Device buffers of the host entry, freed on every return
struct DeviceBuffer {
    void* p = nullptr;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes)
    {
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error(std::string(kWho) + ": out of device memory"); return FRAYHIP_E_NOMEM; }
        return FRAYHIP_OK;
    }
};

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
    DeviceBuffer B;
    if (const int rc = B.alloc(N * (48 + 12 + (r->keys ? 4 : 0)))) return rc;
    double* d_in = (double*)B.p;
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
