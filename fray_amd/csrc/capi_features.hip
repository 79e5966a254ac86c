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

using frayhip_detail::set_error;
using frayhip_detail::FeatureArgs;

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
    if (device && ((uintptr_t)feat & 3)) return bad(who, "device pointer to floats not 4-byte aligned");
    if (f->mode != FRAYHIP_MODE_RENDER) return bad(who, "mode must be FRAYHIP_MODE_RENDER");
    if (n < 1) return bad(who, "n_samples must be >= 1");
    if (!s) return bad(who, "null scene");
    if (s->rendering) return bad(who, "the scene is rendering a frame (a call from inside its progress callback?)");
    const int W = s->settings.frameWidth, H = s->settings.frameHeight;
    const int nb = frayhip_bucket_count(W, H, f->bucket_first, f->bucket_stride > 0 ? f->bucket_stride : 1);
    if (nb < 0) return bad(who, "bad bucket_first / bucket_stride");
    if (n > frame_spp(s)) return bad(who, "n_samples must be <= the frame's spp (" + std::to_string(frame_spp(s)) + ")");
    if (s->camera.stereoSeparation > 0) {
        set_error(std::string(who) + ": stereo frames are not supported");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if (s->settings.gi && s->settings.maxTraceDepth >= 0 && 8 + 10 * ((long long)s->settings.maxTraceDepth + 2) > 227) {
        set_error(std::string(who) + ": path tracing with maxTraceDepth >= 20 (generators past 227 words) is not supported by feature frames");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if ((long long)nb * 2304 > (1ll << 30)) {
        set_error(std::string(who) + ": more than 2^30 pixels in one call (shard the frame with bucket_first / bucket_stride)");
        return FRAYHIP_E_UNSUPPORTED;
    }
    return FRAYHIP_OK;
}

// The one device path of both entries (d_feat: device, frame-sized).  The scene is held as a frame holds it (`rendering`), so that nothing
// re-enters it; on an early return the stream is drained first.  Nothing of the last frame's record is written.
int run(frayhip_scene* sc, const frayhip_frame* f, int n, float* d_feat, hipStream_t stream, frayhip_stats* st)
{
    using namespace frayhip_detail;
    const auto t0 = std::chrono::steady_clock::now();
    struct Busy {
        frayhip_scene* s;
        hipStream_t stream;
        Busy(frayhip_scene* x, hipStream_t y) : s(x), stream(y) { s->rendering = true; }
        ~Busy() { (void)hipStreamSynchronize(stream); s->rendering = false; }
    } busy(sc, stream);
    const frayhip_settings& set = sc->settings;
    const int W = set.frameWidth, H = set.frameHeight;
    DFrame F{};
    F.W = W; F.H = H;
    F.BW = (W - 1) / 48 + 1; F.BH = (H - 1) / 48 + 1;
    F.bucketStride = f->bucket_stride > 0 ? f->bucket_stride : 1;
    F.bucketFirst = f->bucket_first;
    F.nBuckets = frayhip_bucket_count(W, H, F.bucketFirst, F.bucketStride);
    F.spp = frame_spp(sc);
    F.seed = f->seed;
    F.jitter = (sc->camera.dof || set.gi) ? 1 : 0;
    const int nItems = F.nBuckets * 2304;
    DScene S = sc->S;
    S.ambient[0] = set.ambientLight[0]; S.ambient[1] = set.ambientLight[1]; S.ambient[2] = set.ambientLight[2];
    S.maxTraceDepth = set.maxTraceDepth;
    S.gi = set.gi;
    S.saturation = set.saturation;
    const DCamera C = camera_begin_frame(sc->camera, W, H);
    const bool stats = (f->flags & FRAYHIP_FRAME_STATS) != 0;

    HIP_TRY(hipMemsetAsync(sc->d_stats, 0, kStatsBytes, stream));
    DCursors* cursors = (DCursors*)((unsigned char*)sc->d_stats + kCursorOffset);
    HIP_TRY(hipEventRecord(sc->evA, stream));
    size_t nEvents = 0;
    if (nItems > 0 && set.maxTraceDepth < 0) {
        hipLaunchKernelGGL(k_features_zero, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, d_feat);
        HIP_TRY(hipGetLastError());
    } else if (nItems > 0) {
        hipEvent_t e0 = pool_event(sc->evPool, 0), e1 = pool_event(sc->evPool, 1);
        if (!e0 || !e1) return FRAYHIP_E_HIP;
        const FeatureArgs A{S, C, F, nItems, n, d_feat, sc->d_stats, cursors};
        HIP_TRY(hipEventRecord(e0, stream));
        // the flag word the scene was created with (render_dispatch, capi.hip), with the counting bit from the frame
        switch ((sc->extGeometry ? 2 : sc->kdMeshes ? 4 : sc->textured ? 8 : 0) | (stats ? 1 : 0)) {
            case 0: launch_features<0>(stream, A); break;
            case 1: launch_features<1>(stream, A); break;
            case 2: launch_features<2>(stream, A); break;
            case 3: launch_features<3>(stream, A); break;
            case 4: launch_features<4>(stream, A); break;
            case 5: launch_features<5>(stream, A); break;
            case 8: launch_features<8>(stream, A); break;
            default: launch_features<9>(stream, A); break;
        }
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
        frayhip_stats o{};
        o.closest_rays = d.closest; o.shadow_rays = d.shadow; o.node_tests = d.node; o.kd_inner_visits = d.kdInner; o.leaf_refs = d.leafRefs;
        o.tri_tests = d.tri; o.prim_tests = d.prim; o.smooth_hits = d.smooth; o.texture_fetches = d.tex;
        // every pixel of the call takes n samples; counted here, with or without the counting variant
        long long pixels = 0;
        for (int k = 0; k < F.nBuckets; k++) {
            int bx, by;
            frayhip_bucket_xy(W, H, F.bucketFirst + k * F.bucketStride, &bx, &by);
            pixels += (long long)(std::min(W, (bx + 1) * 48) - bx * 48) * (std::min(H, (by + 1) * 48) - by * 48);
        }
        o.samples = (uint64_t)pixels * (uint64_t)n;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, sc->evA, sc->evB);
        o.ms_kernels = ms;
        if (nEvents) {
            float m2 = 0;
            (void)hipEventElapsedTime(&m2, sc->evPool[0], sc->evPool[1]);
            o.ms_trace = m2;
            o.trace_launches = 1;
        }
        o.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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
    const size_t bytes = (size_t)s->settings.frameWidth * s->settings.frameHeight * FRAYHIP_FEAT_CHANNELS * sizeof(float);
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) { (void)hipGetLastError(); set_error("frayhip_render_features: out of device memory"); return FRAYHIP_E_NOMEM; }
    struct Free { void* p; ~Free() { (void)hipFree(p); } } guard{d};
    // pixels outside this call's buckets keep what the caller had in the buffer (render_host's rule)
    if (f->bucket_stride > 1 || f->bucket_first != 0) HIP_TRY(hipMemcpy(d, feat, bytes, hipMemcpyHostToDevice));
    if (const int rc = run(s, f, n_samples, (float*)d, nullptr, st)) return rc;
    HIP_TRY(hipMemcpy(feat, d, bytes, hipMemcpyDeviceToHost));
    return FRAYHIP_OK;
}

}  // extern "C"
