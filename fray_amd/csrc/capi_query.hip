// C ABI, ray queries (include/frayhip.h "ray queries"): frayhip_camera_rays, frayhip_trace_rays, frayhip_visible and their _device forms.
// Argument checks, the scene's kernel flag word, events and counters; the closest-hit and visibility kernels are in query_variant.hip (one
// object per flag word), the camera-ray kernel is here.  Stands behind Camera::getScreenRay (camera.cpp:59-92), the closest-hit loops that
// debugRayTrace fires through a pixel (main.cpp:250-271, 426-435) and visible() (main.cpp:64-80).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "query.hpp"
#include "kernels.hpp"

namespace {

using namespace frayhip_detail;

// Camera::getScreenRay for film positions xy[n][2], or for every integer pixel in row-major order (xy null): the frame's screen_ray on the frame's camera record
__global__ __launch_bounds__(256) void k_camera_rays(DCamera C, long long n, int W, const double* __restrict__ xy, int eye, double* __restrict__ org,
                                                     double* __restrict__ dir)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        double x, y;
        if (xy) { x = xy[2 * i]; y = xy[2 * i + 1]; }
        else { x = (double)(int)(i % W); y = (double)(int)(i / W); }
        V3 o, d;
        screen_ray(C, x, y, o, d, eye);
        if (org) { org[3 * i] = o.x; org[3 * i + 1] = o.y; org[3 * i + 2] = o.z; }
        if (dir) { dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z; }
    }
}

// The checks of every entry, in the order they are made (none touches the device): count and inputs, then the scene.
int check_count(const char* who, int64_t n, std::initializer_list<const void*> inputs)
{
    if (n < 0 || n > INT32_MAX) return bad(who, "n must be 0..INT32_MAX");
    for (const void* p : inputs) if (n > 0 && !p) return bad(who, "null input array");
    return FRAYHIP_OK;
}
int check_scene(const char* who, frayhip_scene* s)
{
    if (!s) return bad(who, "null scene");
    if (s->rendering) return bad(who, "the scene is rendering a frame (a query from inside its progress callback?)");
    return FRAYHIP_OK;
}
int check_doubles(const char* who, std::initializer_list<const void*> ps)
{
    for (const void* p : ps) if (misaligned(p, 8)) return bad(who, "device pointer to doubles not 8-byte aligned");
    return FRAYHIP_OK;
}

enum Kind { CLOSEST = 0, VISIBLE = 1 };

void launch(const frayhip_scene* s, Kind kind, bool stats, hipStream_t stream, const QueryArgs& A)
{
    for_flag_word(flag_word(s, stats), [&](auto w) {
        if (kind == CLOSEST) launch_query_closest<decltype(w)::value>(stream, A); else launch_query_visible<decltype(w)::value>(stream, A);
    });
}

constexpr int64_t kLaunchRays = (int64_t)1 << 30;      // rays per launch (claim_items counts items in an int)

// The one device path of trace_rays / visible (device pointers; the host entries copy around it).  Arguments are checked by the caller.
int run_query(frayhip_scene* sc, Kind kind, int64_t n, const double* a, const double* b, int32_t* id, double* dist, double* rec, uint8_t* vis, int flags,
              hipStream_t stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    Busy busy(sc, stream);
    std::vector<hipEvent_t>& pool = kind == CLOSEST ? sc->evPool : sc->evPoolShadow;
    HIP_TRY(hipMemsetAsync(sc->d_stats, 0, kStatsBytes, stream));
    DCursors* cursors = (DCursors*)((unsigned char*)sc->d_stats + kCursorOffset);
    HIP_TRY(hipEventRecord(sc->evA, stream));
    size_t nEvents = 0;
    for (int64_t done = 0; done < n; done += kLaunchRays) {
        const int m = (int)std::min(kLaunchRays, n - done);
        if (done > 0) HIP_TRY(hipMemsetAsync(cursors, 0, sizeof(DCursors), stream));
        const QueryArgs A{sc->S, m, a + 3 * done, b + 3 * done, id ? id + done : nullptr, dist ? dist + done : nullptr, rec ? rec + 9 * done : nullptr,
                          vis ? vis + done : nullptr, sc->d_stats, cursors};
        hipEvent_t e0 = pool_event(pool, nEvents), e1 = pool_event(pool, nEvents + 1);
        if (!e0 || !e1) return FRAYHIP_E_HIP;
        HIP_TRY(hipEventRecord(e0, stream));
        launch(sc, kind, (flags & FRAYHIP_FRAME_STATS) != 0, stream, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(e1, stream));
        nEvents += 2;
    }
    HIP_TRY(hipEventRecord(sc->evB, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    busy.armed = false;
    DStats d;
    HIP_TRY(hipMemcpy(&d, sc->d_stats, sizeof d, hipMemcpyDeviceToHost));
    if (d.rngOverflow) { set_error("frayhip_trace_rays / frayhip_visible: a CsgOp operand produced more intersections than the device path holds"); return FRAYHIP_E_UNSUPPORTED; }
    if (st) {
        frayhip_stats o = finish_stats(sc, &d, 1, kind == CLOSEST ? nEvents : 0, kind == VISIBLE ? nEvents : 0, t0);
        o.samples = o.texture_fetches = 0;          // a query takes no camera sample and shades nothing
        *st = o;
    }
    return FRAYHIP_OK;
}

int run_camera(frayhip_scene* s, int64_t n, const double* xy, int eye, double* org, double* dir, hipStream_t stream)
{
    Busy busy(s, stream);
    const DCamera C = camera_begin_frame(s->camera, s->settings.frameWidth, s->settings.frameHeight);
    hipLaunchKernelGGL(k_camera_rays, dim3(grid_for((size_t)n)), dim3(256), 0, stream, C, (long long)n, s->settings.frameWidth, xy, eye, org, dir);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    busy.armed = false;
    return FRAYHIP_OK;
}

int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind k)
{
    if (!bytes || !dst) return FRAYHIP_OK;
    HIP_TRY(hipMemcpy(dst, src, bytes, k));
    return FRAYHIP_OK;
}

}  // namespace

extern "C" {

int frayhip_camera_rays_device(frayhip_scene* s, int64_t n, const double* d_xy, int eye, double* d_origin, double* d_dir, void* hip_stream)
{
    const char* who = "frayhip_camera_rays";
    if (const int rc = check_count(who, n, {})) return rc;             // xy may be null (every pixel)
    if (eye < 0 || eye > 2) return bad(who, "eye must be 0 (CENTER), 1 (LEFT) or 2 (RIGHT)");
    if (!d_origin && !d_dir) return bad(who, "no output");
    if (const int rc = check_doubles(who, {d_xy, d_origin, d_dir})) return rc;
    if (const int rc = check_scene(who, s)) return rc;
    if (!d_xy && n != (int64_t)s->settings.frameWidth * s->settings.frameHeight) return bad(who, "xy == NULL needs n == frameWidth * frameHeight");
    if (n == 0) return FRAYHIP_OK;
    return run_camera(s, n, d_xy, eye, d_origin, d_dir, (hipStream_t)hip_stream);
}

int frayhip_camera_rays(frayhip_scene* s, int64_t n, const double* xy, int eye, double* origin, double* dir)
{
    const char* who = "frayhip_camera_rays";
    if (const int rc = check_count(who, n, {})) return rc;
    if (eye < 0 || eye > 2) return bad(who, "eye must be 0 (CENTER), 1 (LEFT) or 2 (RIGHT)");
    if (!origin && !dir) return bad(who, "no output");
    if (const int rc = check_scene(who, s)) return rc;
    if (!xy && n != (int64_t)s->settings.frameWidth * s->settings.frameHeight) return bad(who, "xy == NULL needs n == frameWidth * frameHeight");
    if (n == 0) return FRAYHIP_OK;
    const size_t N = (size_t)n;
    DeviceArrays B("ray query: out of device memory");
    double *d_xy, *d_o, *d_d;
    if (int rc = B.alloc(d_xy, 2 * N, xy != nullptr)) return rc;
    if (int rc = B.alloc(d_o, 3 * N, origin != nullptr)) return rc;
    if (int rc = B.alloc(d_d, 3 * N, dir != nullptr)) return rc;
    if (int rc = copy(d_xy, xy, 16 * N, hipMemcpyHostToDevice)) return rc;
    if (int rc = run_camera(s, n, d_xy, eye, d_o, d_d, nullptr)) return rc;
    if (int rc = copy(origin, d_o, 24 * N, hipMemcpyDeviceToHost)) return rc;
    return copy(dir, d_d, 24 * N, hipMemcpyDeviceToHost);
}

int frayhip_trace_rays_device(frayhip_scene* s, int64_t n, const double* d_origin, const double* d_dir, int flags, int32_t* d_hit_id, double* d_hit_dist,
                              double* d_hit_rec, void* hip_stream, frayhip_stats* st)
{
    const char* who = "frayhip_trace_rays";
    if (const int rc = check_count(who, n, {d_origin, d_dir})) return rc;
    if (!d_hit_id && !d_hit_dist && !d_hit_rec) return bad(who, "no output (hit_id, hit_dist and hit_rec are all NULL)");
    if (const int rc = check_doubles(who, {d_origin, d_dir, d_hit_dist, d_hit_rec})) return rc;
    if (misaligned(d_hit_id, 4)) return bad(who, "device pointer to int32 not 4-byte aligned");
    if (const int rc = check_scene(who, s)) return rc;
    if (n == 0) return no_work(st);
    return run_query(s, CLOSEST, n, d_origin, d_dir, d_hit_id, d_hit_dist, d_hit_rec, nullptr, flags, (hipStream_t)hip_stream, st);
}

int frayhip_trace_rays(frayhip_scene* s, int64_t n, const double* origin, const double* dir, int flags, int32_t* hit_id, double* hit_dist, double* hit_rec,
                       frayhip_stats* st)
{
    const char* who = "frayhip_trace_rays";
    if (const int rc = check_count(who, n, {origin, dir})) return rc;
    if (!hit_id && !hit_dist && !hit_rec) return bad(who, "no output (hit_id, hit_dist and hit_rec are all NULL)");
    if (const int rc = check_scene(who, s)) return rc;
    if (n == 0) return no_work(st);
    const size_t N = (size_t)n;
    DeviceArrays B("ray query: out of device memory");
    double *d_in, *d_dist, *d_rec;
    int32_t* d_id;
    if (int rc = B.alloc(d_in, 6 * N, true)) return rc;
    if (int rc = B.alloc(d_id, N, hit_id != nullptr)) return rc;
    if (int rc = B.alloc(d_dist, N, hit_dist != nullptr)) return rc;
    if (int rc = B.alloc(d_rec, 9 * N, hit_rec != nullptr)) return rc;
    if (int rc = copy(d_in, origin, 24 * N, hipMemcpyHostToDevice)) return rc;
    if (int rc = copy(d_in + 3 * N, dir, 24 * N, hipMemcpyHostToDevice)) return rc;
    if (int rc = run_query(s, CLOSEST, n, d_in, d_in + 3 * N, d_id, d_dist, d_rec, nullptr, flags, nullptr, st)) return rc;
    if (int rc = copy(hit_id, d_id, 4 * N, hipMemcpyDeviceToHost)) return rc;
    if (int rc = copy(hit_dist, d_dist, 8 * N, hipMemcpyDeviceToHost)) return rc;
    return copy(hit_rec, d_rec, 72 * N, hipMemcpyDeviceToHost);
}

int frayhip_visible_device(frayhip_scene* s, int64_t n, const double* d_a, const double* d_b, int flags, uint8_t* d_vis, void* hip_stream, frayhip_stats* st)
{
    const char* who = "frayhip_visible";
    if (const int rc = check_count(who, n, {d_a, d_b})) return rc;
    if (!d_vis) return bad(who, "no output (vis is NULL)");
    if (const int rc = check_doubles(who, {d_a, d_b})) return rc;
    if (const int rc = check_scene(who, s)) return rc;
    if (n == 0) return no_work(st);
    return run_query(s, VISIBLE, n, d_a, d_b, nullptr, nullptr, nullptr, d_vis, flags, (hipStream_t)hip_stream, st);
}

int frayhip_visible(frayhip_scene* s, int64_t n, const double* a, const double* b, int flags, uint8_t* vis, frayhip_stats* st)
{
    const char* who = "frayhip_visible";
    if (const int rc = check_count(who, n, {a, b})) return rc;
    if (!vis) return bad(who, "no output (vis is NULL)");
    if (const int rc = check_scene(who, s)) return rc;
    if (n == 0) return no_work(st);
    const size_t N = (size_t)n;
    DeviceArrays B("ray query: out of device memory");
    double* d_in;
    uint8_t* d_vis;
    if (int rc = B.alloc(d_in, 6 * N, true)) return rc;
    if (int rc = B.alloc(d_vis, N, true)) return rc;
    if (int rc = copy(d_in, a, 24 * N, hipMemcpyHostToDevice)) return rc;
    if (int rc = copy(d_in + 3 * N, b, 24 * N, hipMemcpyHostToDevice)) return rc;
    if (int rc = run_query(s, VISIBLE, n, d_in, d_in + 3 * N, nullptr, nullptr, nullptr, d_vis, flags, nullptr, st)) return rc;
    return copy(vis, d_vis, N, hipMemcpyDeviceToHost);
}

}  // extern "C"
