// C ABI, adaptive frames (include/frayhip.h "adaptive frames"): frayhip_render_adaptive and frayhip_render_device_adaptive.  Argument checks, the
// scene's kernel flag word and the `rendering` guard; the ladder, the kernels and the batch loop are adaptive_impl<ST> of adaptive_variant.hip (one
// object per flag word).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "adaptive.hpp"

namespace {

using frayhip_detail::set_error;
using frayhip_detail::AdaptiveCall;

int bad(const char* who, const std::string& why)
{
    set_error(std::string(who) + ": " + why);
    return FRAYHIP_E_ARG;
}

// the frame's samples per pixel (main.cpp:395-400, render_impl)
int frame_spp(const frayhip_scene* s)
{
    int spp = s->settings.wantAA ? 5 : 1;
    if (s->camera.dof) spp = std::max(spp, s->camera.numDOFSamples);
    if (s->settings.gi) spp = std::max(spp, s->settings.numPaths);
    return spp;
}

// Every check of both entries, in this order; none touches the device.  FRAYHIP_E_ARG for the arguments, FRAYHIP_E_UNSUPPORTED for a frame the
// adaptive path does not render (Whitted, stereo, long generators), then the sample counts against the frame's.
int check(const char* who, frayhip_scene* s, const frayhip_frame* f, const frayhip_adaptive* a, const float* rgb)
{
    if (!f) return bad(who, "null frame");
    if (!a) return bad(who, "null request");
    if (!rgb) return bad(who, "null rgb");
    if (f->mode != FRAYHIP_MODE_RENDER) return bad(who, "mode must be FRAYHIP_MODE_RENDER");
    if (a->min_spp < 2) return bad(who, "min_spp must be >= 2");
    if (std::isnan(a->threshold) || a->threshold < 0) return bad(who, "threshold must be >= 0 (and not NaN)");
    if (!std::isfinite(a->err_floor) || !(a->err_floor > 0)) return bad(who, "err_floor must be finite and > 0");
    if (!s) return bad(who, "null scene");
    if (s->rendering) return bad(who, "the scene is rendering a frame (a call from inside its progress callback?)");
    const int W = s->settings.frameWidth, H = s->settings.frameHeight;
    const int nb = frayhip_bucket_count(W, H, f->bucket_first, f->bucket_stride > 0 ? f->bucket_stride : 1);
    if (nb < 0) return bad(who, "bad bucket_first / bucket_stride");
    if (!s->settings.gi) {
        set_error(std::string(who) + ": adaptive frames are path-traced; a Whitted frame (gi off) is not supported");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if (s->camera.stereoSeparation > 0) {
        set_error(std::string(who) + ": stereo frames are not supported");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if (s->settings.maxTraceDepth >= 0 && 8 + 10 * ((long long)s->settings.maxTraceDepth + 2) > 227) {
        set_error(std::string(who) + ": path tracing with maxTraceDepth >= 20 (generators past 227 words) is not supported by adaptive frames");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if ((long long)nb * 2304 > (1ll << 30)) {
        set_error(std::string(who) + ": more than 2^30 pixels in one call (shard the frame with bucket_first / bucket_stride)");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if (a->min_spp > frame_spp(s)) return bad(who, "min_spp must be <= the frame's spp (" + std::to_string(frame_spp(s)) + ")");
    return FRAYHIP_OK;
}

AdaptiveCall call_of(frayhip_scene* s, const frayhip_frame* f, const frayhip_adaptive* a, float* rgb, int32_t* spp, float* err)
{
    AdaptiveCall q;
    q.bucketFirst = f->bucket_first;
    q.bucketStride = f->bucket_stride > 0 ? f->bucket_stride : 1;
    q.seed = f->seed;
    q.sppChunk = f->spp_chunk;
    q.stats = (f->flags & FRAYHIP_FRAME_STATS) != 0;
    q.spp = frame_spp(s);
    q.minSpp = a->min_spp;
    q.threshold = a->threshold;
    q.errFloor = a->err_floor;
    q.rgb = rgb; q.sppOut = spp; q.errOut = err;
    return q;
}

// the flag word the scene was created with (render_dispatch, capi.hip), with the counting bit from the frame.  The scene is held as a frame holds
// it (`rendering`), so that nothing re-enters it; on an early return the stream is drained first.
int run(frayhip_scene* s, AdaptiveCall& q, hipStream_t stream, frayhip_adaptive* a, frayhip_stats* st)
{
    using namespace frayhip_detail;
    struct Busy {
        frayhip_scene* s;
        hipStream_t stream;
        Busy(frayhip_scene* x, hipStream_t y) : s(x), stream(y) { s->rendering = true; }
        ~Busy() { (void)hipStreamSynchronize(stream); s->rendering = false; }
    } busy(s, stream);
    const int w = (s->extGeometry ? 2 : s->kdMeshes ? 4 : s->textured ? 8 : 0) | (q.stats ? 1 : 0);
    int rc;
    switch (w) {
        case 0: rc = adaptive_impl<0>(s, q, stream, st); break;
        case 1: rc = adaptive_impl<1>(s, q, stream, st); break;
        case 2: rc = adaptive_impl<2>(s, q, stream, st); break;
        case 3: rc = adaptive_impl<3>(s, q, stream, st); break;
        case 4: rc = adaptive_impl<4>(s, q, stream, st); break;
        case 5: rc = adaptive_impl<5>(s, q, stream, st); break;
        case 8: rc = adaptive_impl<8>(s, q, stream, st); break;
        default: rc = adaptive_impl<9>(s, q, stream, st); break;
    }
    if (rc == FRAYHIP_OK) { a->rungs = q.rungs; a->samples = q.samples; }
    return rc;
}

// Device buffers of the host entry, freed on every return
struct DeviceBuffer {
    void* p = nullptr;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes)
    {
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; set_error("frayhip_render_adaptive: out of device memory"); return FRAYHIP_E_NOMEM; }
        return FRAYHIP_OK;
    }
};

}  // namespace

extern "C" {

int frayhip_render_device_adaptive(frayhip_scene* s, const frayhip_frame* f, frayhip_adaptive* a, float* d_rgb, int32_t* d_spp, float* d_err,
                                   void* hip_stream, frayhip_stats* st)
{
    if (const int rc = check("frayhip_render_device_adaptive", s, f, a, d_rgb)) return rc;
    AdaptiveCall q = call_of(s, f, a, d_rgb, d_spp, d_err);
    return run(s, q, (hipStream_t)hip_stream, a, st);
}

int frayhip_render_adaptive(frayhip_scene* s, const frayhip_frame* f, frayhip_adaptive* a, float* rgb, int32_t* spp_out, float* err_out, frayhip_stats* st)
{
    if (const int rc = check("frayhip_render_adaptive", s, f, a, rgb)) return rc;
    const size_t n = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    // one allocation: colours, then sample counts and errors when asked for
    DeviceBuffer B;
    if (const int rc = B.alloc(n * (12 + (spp_out ? 4 : 0) + (err_out ? 4 : 0)))) return rc;
    float* d_rgb = (float*)B.p;
    int32_t* d_spp = spp_out ? (int32_t*)(d_rgb + 3 * n) : nullptr;
    float* d_err = err_out ? (float*)((char*)B.p + n * (12 + (spp_out ? 4 : 0))) : nullptr;
    // pixels outside this call's buckets keep what the caller had in the buffers (render_host's rule)
    if (f->bucket_stride > 1 || f->bucket_first != 0) {
        HIP_TRY(hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice));
        if (d_spp) HIP_TRY(hipMemcpy(d_spp, spp_out, n * 4, hipMemcpyHostToDevice));
        if (d_err) HIP_TRY(hipMemcpy(d_err, err_out, n * 4, hipMemcpyHostToDevice));
    }
    AdaptiveCall q = call_of(s, f, a, d_rgb, d_spp, d_err);
    if (const int rc = run(s, q, nullptr, a, st)) return rc;
    HIP_TRY(hipMemcpy(rgb, d_rgb, n * 12, hipMemcpyDeviceToHost));
    if (d_spp) HIP_TRY(hipMemcpy(spp_out, d_spp, n * 4, hipMemcpyDeviceToHost));
    if (d_err) HIP_TRY(hipMemcpy(err_out, d_err, n * 4, hipMemcpyDeviceToHost));
    return FRAYHIP_OK;
}

}  // extern "C"
