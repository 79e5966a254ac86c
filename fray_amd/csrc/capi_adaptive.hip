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

using namespace frayhip_detail;

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
    const int nb = frame_record(s, f->bucket_first, f->bucket_stride, f->seed).nBuckets;
    if (const int rc = check_bucket_range(who, nb)) return rc;
    if (!s->settings.gi) return unsupported(who, "adaptive frames are path-traced; a Whitted frame (gi off) is not supported");
    if (const int rc = refuse_stereo(who, s)) return rc;
    if (const int rc = refuse_long_generators(who, s, "adaptive frames")) return rc;
    if (const int rc = check_pixel_cap(who, nb)) return rc;
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

// The scene's flag word with the counting bit from the frame; the stream is drained on every return.
int run(frayhip_scene* s, AdaptiveCall& q, hipStream_t stream, frayhip_adaptive* a, frayhip_stats* st)
{
    Busy busy(s, stream);
    const int rc = for_flag_word(flag_word(s, q.stats), [&](auto w) { return adaptive_impl<decltype(w)::value>(s, q, stream, st); });
    if (rc == FRAYHIP_OK) { a->rungs = q.rungs; a->samples = q.samples; }
    return rc;
}

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
    DeviceArrays B("frayhip_render_adaptive: out of device memory");
    unsigned char* base;
    if (const int rc = B.alloc(base, n * (12 + (spp_out ? 4 : 0) + (err_out ? 4 : 0)))) return rc;
    float* d_rgb = (float*)base;
    int32_t* d_spp = spp_out ? (int32_t*)(d_rgb + 3 * n) : nullptr;
    float* d_err = err_out ? (float*)(base + n * (12 + (spp_out ? 4 : 0))) : nullptr;
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
