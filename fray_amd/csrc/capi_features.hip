// C ABI, feature frames (include/frayhip.h "feature frames"): frayhip_render_features and frayhip_render_features_device.  Argument checks, the
// frame record, the scene's kernel flag word, events and counters; the kernel is k_features<ST> of features_variant.hip (one object per flag word).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <string>

#include "features.hpp"
#include "kernels.hpp"

namespace {

using namespace frayhip_detail;

// maxTraceDepth < 0: every feature of the call's pixels is 0
__global__ __launch_bounds__(256) void k_features_zero(DFrame F, int nItems, float* __restrict__ feat)
{
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        float* o = feat + ((size_t)y * F.W + x) * FRAYHIP_FEAT_CHANNELS;
        for (int k = 0; k < FRAYHIP_FEAT_CHANNELS; k++) o[k] = 0.0f;
    }
}

// Every check of both entries, in this order; none touches the device.  FRAYHIP_E_ARG for the arguments, FRAYHIP_E_UNSUPPORTED for a frame
// whose rays the feature pass does not reproduce (stereo, long generators).
int check(const char* who, frayhip_scene* s, const frayhip_frame* f, int n, const float* feat, bool device)
{
    if (!f) return bad(who, "null frame");
    if (!feat) return bad(who, "null feat");
    if (device && misaligned(feat, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
    if (f->mode != FRAYHIP_MODE_RENDER) return bad(who, "mode must be FRAYHIP_MODE_RENDER");
    if (n < 1) return bad(who, "n_samples must be >= 1");
    if (!s) return bad(who, "null scene");
    if (s->rendering) return bad(who, "the scene is rendering a frame (a call from inside its progress callback?)");
    const int nb = frame_record(s, f->bucket_first, f->bucket_stride, f->seed).nBuckets;
    if (const int rc = check_bucket_range(who, nb)) return rc;
    if (n > frame_spp(s)) return bad(who, "n_samples must be <= the frame's spp (" + std::to_string(frame_spp(s)) + ")");
    if (const int rc = refuse_stereo(who, s)) return rc;
    if (const int rc = refuse_long_generators(who, s, "feature frames")) return rc;
    return check_pixel_cap(who, nb);
}

// The one device path of both entries (d_feat: device, frame-sized).  The scene is held as a frame holds it (`rendering`), so that nothing
// re-enters it; on an early return the stream is drained first.  Nothing of the last frame's record is written.
int run(frayhip_scene* sc, const frayhip_frame* f, int n, float* d_feat, hipStream_t stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    Busy busy(sc, stream);
    const DFrame F = frame_record(sc, f->bucket_first, f->bucket_stride, f->seed);
    const int W = F.W, H = F.H, nItems = F.nBuckets * 2304;
    const DScene S = frame_scene(sc);
    const DCamera C = camera_begin_frame(sc->camera, W, H);
    const bool stats = (f->flags & FRAYHIP_FRAME_STATS) != 0;

    HIP_TRY(hipMemsetAsync(sc->d_stats, 0, kStatsBytes, stream));
    DCursors* cursors = (DCursors*)((unsigned char*)sc->d_stats + kCursorOffset);
    HIP_TRY(hipEventRecord(sc->evA, stream));
    size_t nEvents = 0;
    if (nItems > 0 && S.maxTraceDepth < 0) {
        hipLaunchKernelGGL(k_features_zero, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, d_feat);
        HIP_TRY(hipGetLastError());
    } else if (nItems > 0) {
        hipEvent_t e0 = pool_event(sc->evPool, 0), e1 = pool_event(sc->evPool, 1);
        if (!e0 || !e1) return FRAYHIP_E_HIP;
        const FeatureArgs A{S, C, F, nItems, n, d_feat, sc->d_stats, cursors};
        HIP_TRY(hipEventRecord(e0, stream));
        for_flag_word(flag_word(sc, stats), [&](auto w) { launch_features<decltype(w)::value>(stream, A); });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(e1, stream));
        nEvents = 2;
    }
    HIP_TRY(hipEventRecord(sc->evB, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    DStats d;
    HIP_TRY(hipMemcpy(&d, sc->d_stats, sizeof d, hipMemcpyDeviceToHost));
    if (d.rngOverflow) {
        set_error("frayhip_render_features: a camera sample left the supported envelope (a lens sample past 227 generator words, or a CsgOp operand "
                  "with more intersections than the device path holds)");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if (st) {
        frayhip_stats o = finish_stats(sc, &d, 1, nEvents, 0, t0);
        // every pixel of the call takes n samples; counted here, with or without the counting variant
        long long pixels = 0;
        for (int k = 0; k < F.nBuckets; k++) {
            int bx, by;
            frayhip_bucket_xy(W, H, F.bucketFirst + k * F.bucketStride, &bx, &by);
            pixels += (long long)(std::min(W, (bx + 1) * 48) - bx * 48) * (std::min(H, (by + 1) * 48) - by * 48);
        }
        o.samples = (uint64_t)pixels * (uint64_t)n;
        *st = o;
    }
    return FRAYHIP_OK;
}

}  // namespace

extern "C" {

int frayhip_render_features_device(frayhip_scene* s, const frayhip_frame* f, int n_samples, float* d_feat, void* hip_stream, frayhip_stats* st)
{
    if (const int rc = check("frayhip_render_features_device", s, f, n_samples, d_feat, true)) return rc;
    return run(s, f, n_samples, d_feat, (hipStream_t)hip_stream, st);
}

int frayhip_render_features(frayhip_scene* s, const frayhip_frame* f, int n_samples, float* feat, frayhip_stats* st)
{
    if (const int rc = check("frayhip_render_features", s, f, n_samples, feat, false)) return rc;
    const size_t count = (size_t)s->settings.frameWidth * s->settings.frameHeight * FRAYHIP_FEAT_CHANNELS, bytes = count * sizeof(float);
    DeviceArrays B("frayhip_render_features: out of device memory");
    float* d;
    if (const int rc = B.alloc(d, count)) return rc;
    // pixels outside this call's buckets keep what the caller had in the buffer (render_host's rule)
    if (f->bucket_stride > 1 || f->bucket_first != 0) HIP_TRY(hipMemcpy(d, feat, bytes, hipMemcpyHostToDevice));
    if (const int rc = run(s, f, n_samples, d, nullptr, st)) return rc;
    HIP_TRY(hipMemcpy(feat, d, bytes, hipMemcpyDeviceToHost));
    return FRAYHIP_OK;
}

}  // extern "C"
