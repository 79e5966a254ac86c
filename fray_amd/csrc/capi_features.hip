// C ABI, feature frames (include/frayhip.h "feature frames", "specular feature frames", "motion frames"): frayhip_render_features,
// frayhip_render_features_specular, frayhip_render_features_motion and their _device entries.  Argument checks, the frame record, the scene's
// kernel flag word, the motion frame's table of previous transforms, events and counters; the kernels are k_features<ST, MOTION> of
// features_variant.hip and k_features_specular<ST> of features_specular_variant.hip (one object per flag word each).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "features_specular.hpp"
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
// ... and of the motion frame
__global__ __launch_bounds__(256) void k_motion_zero(DFrame F, int nItems, float* __restrict__ motion)
{
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        float* o = motion + ((size_t)y * F.W + x) * FRAYHIP_MOTION_CHANNELS;
        for (int k = 0; k < FRAYHIP_MOTION_CHANNELS; k++) o[k] = 0.0f;
    }
}

// ... and of the specular frame's plane of bounce counts
__global__ __launch_bounds__(256) void k_plane_zero(DFrame F, int nItems, float* __restrict__ plane)
{
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        plane[(size_t)y * F.W + x] = 0.0f;
    }
}

// The specular frame's request: the bounce limit, and where the plane of counts goes (device, or null)
struct SpecularCall {
    int maxBounces;
    float* d_bounces;
};

// Whether any node's own shader is Refl or Refr, from the host copies frayhip_scene_update keeps current: looked up per call
bool has_specular_node(const frayhip_scene* sc, int nNodes)
{
    const DNode* const nodes = host_nodes(sc);
    const DShader* const shaders = host_shaders(sc);
    for (int i = 0; i < nNodes; i++) {
        const int kind = shaders[nodes[i].shader].kind;
        if (kind == 3 || kind == 4) return true;
    }
    return false;
}

// The motion frame's request: the caller's previous transforms (host), and where the frame goes (device)
struct MotionCall {
    const frayhip_transform* prevT;
    float* d_motion;
};

// Every check of both entries, in this order; none touches the device.  FRAYHIP_E_ARG for the arguments, FRAYHIP_E_UNSUPPORTED for a frame
// whose rays the feature pass does not reproduce (stereo, long generators).
// spec: the specular entries' request (their scene-free checks sit with the others'), or null.
int check(const char* who, frayhip_scene* s, const frayhip_frame* f, int n, const float* feat, bool device, const SpecularCall* spec = nullptr)
{
    if (!f) return bad(who, "null frame");
    if (!feat) return bad(who, "null feat");
    if (device && misaligned(feat, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
    if (f->mode != FRAYHIP_MODE_RENDER) return bad(who, "mode must be FRAYHIP_MODE_RENDER");
    if (n < 1) return bad(who, "n_samples must be >= 1");
    if (spec) {
        if (spec->maxBounces < 1 || spec->maxBounces > FRAYHIP_SPECULAR_MAX_BOUNCES)
            return bad(who, "max_bounces must be 1 .. " + std::to_string(FRAYHIP_SPECULAR_MAX_BOUNCES) + " (" + std::to_string(spec->maxBounces) + ")");
        if (device && misaligned(spec->d_bounces, 4)) return bad(who, "device pointer to floats not 4-byte aligned (bounces)");
    }
    if (!s) return bad(who, "null scene");
    if (s->rendering) return bad(who, "the scene is rendering a frame (a call from inside its progress callback?)");
    const int nb = frame_record(s, f->bucket_first, f->bucket_stride, f->seed).nBuckets;
    if (const int rc = check_bucket_range(who, nb)) return rc;
    if (n > frame_spp(s)) return bad(who, "n_samples must be <= the frame's spp (" + std::to_string(frame_spp(s)) + ")");
    if (const int rc = refuse_stereo(who, s)) return rc;
    if (const int rc = refuse_long_generators(who, s, "feature frames")) return rc;
    return check_pixel_cap(who, nb);
}

// ... and what the motion entries add, after them (the scene is known to be there)
int check_motion(const char* who, frayhip_scene* s, const frayhip_transform* prevT, int nPrev, const float* feat, const float* motion, bool device)
{
    if (!prevT) return bad(who, "null prev_T");
    if (!motion) return bad(who, "null motion");
    if (device && misaligned(motion, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
    if (nPrev != s->S.nNodes) return bad(who, "n_prev (" + std::to_string(nPrev) + ") is not the scene's node count (" + std::to_string(s->S.nNodes) + ")");
    for (int i = 0; i < nPrev; i++) {
        const double* v = prevT[i].offset;                   // offset[3], m[9], invM[9]: 21 doubles back to back
        static_assert(sizeof(frayhip_transform) == 21 * sizeof(double), "frayhip_transform is 21 doubles");
        for (int k = 0; k < 21; k++)
            if (!std::isfinite(v[k])) return bad(who, "prev_T[" + std::to_string(i) + "] has a non-finite value");
    }
    const size_t n = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    const uintptr_t a = (uintptr_t)feat, b = (uintptr_t)motion;
    if (a < b + n * 4 * FRAYHIP_MOTION_CHANNELS && b < a + n * 4 * FRAYHIP_FEAT_CHANNELS) return bad(who, "feat and motion must not overlap");
    return FRAYHIP_OK;
}

// ... and what the specular entries add once the scene is known to be there
int check_specular(const char* who, frayhip_scene* s, const float* feat, const float* bounces)
{
    if (!bounces) return FRAYHIP_OK;
    const size_t n = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    const uintptr_t a = (uintptr_t)feat, b = (uintptr_t)bounces;
    if (a < b + n * 4 && b < a + n * 4 * FRAYHIP_FEAT_CHANNELS) return bad(who, "feat and bounces must not overlap");
    return FRAYHIP_OK;
}

// The one device path of both entries (d_feat: device, frame-sized).  The scene is held as a frame holds it (`rendering`), so that nothing
// re-enters it; on an early return the stream is drained first.  Nothing of the last frame's record is written.
// mc: the motion frame's request, or null; spec: the specular frame's, or null (never both).
int run(frayhip_scene* sc, const frayhip_frame* f, int n, float* d_feat, hipStream_t stream, frayhip_stats* st, const MotionCall* mc = nullptr,
        const SpecularCall* spec = nullptr)
{
    const auto t0 = std::chrono::steady_clock::now();
    Busy busy(sc, stream);
    const DFrame F = frame_record(sc, f->bucket_first, f->bucket_stride, f->seed);
    const int W = F.W, H = F.H, nItems = F.nBuckets * 2304;
    const DScene S = frame_scene(sc);
    const DCamera C = camera_begin_frame(sc->camera, W, H);
    const bool stats = (f->flags & FRAYHIP_FRAME_STATS) != 0;

    // The motion frame's table of the call: per node the previous {offset, m}, then a byte per node -- moved when any of the transform's 21
    // doubles differs by bit pattern from the node's now (the host copy of the node table, which frayhip_scene_update keeps current).  Both
    // copies belong to the scene and are reused; the device one grows only when the node count asks for it, so a call in a sequence
    // allocates nothing.
    const DPrevXform* d_prev = nullptr;
    const unsigned char* d_moved = nullptr;
    if (mc && nItems > 0 && S.maxTraceDepth >= 0) {
        const int nn = S.nNodes;
        const DNode* const nodes = host_nodes(sc);
        std::vector<unsigned char>& tab = sc->motionTabHost;
        tab.resize((size_t)nn * (sizeof(DPrevXform) + 1) + 1);
        DPrevXform* const prev = (DPrevXform*)tab.data();
        unsigned char* const moved = tab.data() + (size_t)nn * sizeof(DPrevXform);
        for (int i = 0; i < nn; i++) {
            const frayhip_transform& T = mc->prevT[i];
            memcpy(prev[i].off, T.offset, sizeof prev[i].off);
            memcpy(prev[i].m, T.m, sizeof prev[i].m);
            const DXform& X = nodes[i].T;
            moved[i] = memcmp(X.off, T.offset, sizeof X.off) != 0 || memcmp(X.m, T.m, sizeof X.m) != 0 || memcmp(X.inv, T.invM, sizeof X.inv) != 0;
        }
        if (sc->motionTabBytes < tab.size()) {
            if (sc->d_motionTab) (void)hipFree(sc->d_motionTab);
            sc->d_motionTab = nullptr;
            sc->motionTabBytes = 0;
            if (hipMalloc(&sc->d_motionTab, tab.size()) != hipSuccess) {
                (void)hipGetLastError();
                set_error("frayhip_render_features_motion: out of device memory");
                return FRAYHIP_E_NOMEM;
            }
            sc->motionTabBytes = tab.size();
        }
        unsigned char* const d_tab = (unsigned char*)sc->d_motionTab;
        HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, stream));
        d_prev = (const DPrevXform*)d_tab;
        d_moved = d_tab + (size_t)nn * sizeof(DPrevXform);
    }

    HIP_TRY(hipMemsetAsync(sc->d_stats, 0, kStatsBytes, stream));
    DCursors* cursors = (DCursors*)((unsigned char*)sc->d_stats + kCursorOffset);
    HIP_TRY(hipEventRecord(sc->evA, stream));
    size_t nEvents = 0;
    if (nItems > 0 && S.maxTraceDepth < 0) {
        hipLaunchKernelGGL(k_features_zero, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, d_feat);
        HIP_TRY(hipGetLastError());
        if (mc) {
            hipLaunchKernelGGL(k_motion_zero, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, mc->d_motion);
            HIP_TRY(hipGetLastError());
        }
        if (spec && spec->d_bounces) {
            hipLaunchKernelGGL(k_plane_zero, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, spec->d_bounces);
            HIP_TRY(hipGetLastError());
        }
    } else if (nItems > 0) {
        hipEvent_t e0 = pool_event(sc->evPool, 0), e1 = pool_event(sc->evPool, 1);
        if (!e0 || !e1) return FRAYHIP_E_HIP;
        const FeatureArgs A{S, C, F, nItems, n, d_feat, sc->d_stats, cursors, mc ? mc->d_motion : nullptr, d_prev, d_moved};
        HIP_TRY(hipEventRecord(e0, stream));
        if (spec && has_specular_node(sc, S.nNodes)) {
            const SpecularFeatureArgs SA{S, C, F, nItems, n, spec->maxBounces, d_feat, spec->d_bounces, sc->d_stats, cursors};
            for_flag_word(flag_word(sc, stats), [&](auto w) { launch_features_specular<decltype(w)::value>(stream, SA); });
            HIP_TRY(hipGetLastError());
        } else {
            // (a specular call on a scene without a Refl / Refr node: no chain can start, so the first-hit kernel and a zero plane)
            for_flag_word(flag_word(sc, stats), [&](auto w) { launch_features<decltype(w)::value>(stream, A, mc != nullptr); });
            HIP_TRY(hipGetLastError());
            if (spec && spec->d_bounces) {
                hipLaunchKernelGGL(k_plane_zero, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, spec->d_bounces);
                HIP_TRY(hipGetLastError());
            }
        }
        HIP_TRY(hipEventRecord(e1, stream));
        nEvents = 2;
    }
    HIP_TRY(hipEventRecord(sc->evB, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    DStats d;
    HIP_TRY(hipMemcpy(&d, sc->d_stats, sizeof d, hipMemcpyDeviceToHost));
    if (d.rngOverflow) {
        set_error(std::string(mc ? "frayhip_render_features_motion" : spec ? "frayhip_render_features_specular" : "frayhip_render_features") + ": a camera sample left the supported envelope (a lens sample past 227 generator words, or a CsgOp operand "
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

int frayhip_render_features_specular_device(frayhip_scene* s, const frayhip_frame* f, int n_samples, int max_bounces, float* d_feat, float* d_bounces,
                                            void* hip_stream, frayhip_stats* st)
{
    const char* who = "frayhip_render_features_specular_device";
    const SpecularCall spec{max_bounces, d_bounces};
    if (const int rc = check(who, s, f, n_samples, d_feat, true, &spec)) return rc;
    if (const int rc = check_specular(who, s, d_feat, d_bounces)) return rc;
    return run(s, f, n_samples, d_feat, (hipStream_t)hip_stream, st, nullptr, &spec);
}

int frayhip_render_features_specular(frayhip_scene* s, const frayhip_frame* f, int n_samples, int max_bounces, float* feat, float* bounces, frayhip_stats* st)
{
    const char* who = "frayhip_render_features_specular";
    const SpecularCall asked{max_bounces, bounces};
    if (const int rc = check(who, s, f, n_samples, feat, false, &asked)) return rc;
    if (const int rc = check_specular(who, s, feat, bounces)) return rc;
    const size_t px = (size_t)s->settings.frameWidth * s->settings.frameHeight, nf = px * FRAYHIP_FEAT_CHANNELS;
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d;
    if (const int rc = B.alloc(d, nf + (bounces ? px : 0))) return rc;
    float* const db = bounces ? d + nf : nullptr;
    // pixels outside this call's buckets keep what the caller had in the buffers
    if (f->bucket_stride > 1 || f->bucket_first != 0) {
        HIP_TRY(hipMemcpy(d, feat, nf * sizeof(float), hipMemcpyHostToDevice));
        if (bounces) HIP_TRY(hipMemcpy(db, bounces, px * sizeof(float), hipMemcpyHostToDevice));
    }
    const SpecularCall spec{max_bounces, db};
    if (const int rc = run(s, f, n_samples, d, nullptr, st, nullptr, &spec)) return rc;
    HIP_TRY(hipMemcpy(feat, d, nf * sizeof(float), hipMemcpyDeviceToHost));
    if (bounces) HIP_TRY(hipMemcpy(bounces, db, px * sizeof(float), hipMemcpyDeviceToHost));
    return FRAYHIP_OK;
}

int frayhip_render_features_motion_device(frayhip_scene* s, const frayhip_frame* f, int n_samples, const frayhip_transform* prev_T, int n_prev,
                                          float* d_feat, float* d_motion, void* hip_stream, frayhip_stats* st)
{
    const char* who = "frayhip_render_features_motion_device";
    if (const int rc = check(who, s, f, n_samples, d_feat, true)) return rc;
    if (const int rc = check_motion(who, s, prev_T, n_prev, d_feat, d_motion, true)) return rc;
    const MotionCall mc{prev_T, d_motion};
    return run(s, f, n_samples, d_feat, (hipStream_t)hip_stream, st, &mc);
}

int frayhip_render_features_motion(frayhip_scene* s, const frayhip_frame* f, int n_samples, const frayhip_transform* prev_T, int n_prev,
                                   float* feat, float* motion, frayhip_stats* st)
{
    const char* who = "frayhip_render_features_motion";
    if (const int rc = check(who, s, f, n_samples, feat, false)) return rc;
    if (const int rc = check_motion(who, s, prev_T, n_prev, feat, motion, false)) return rc;
    const size_t px = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    const size_t nf = px * FRAYHIP_FEAT_CHANNELS, nm = px * FRAYHIP_MOTION_CHANNELS;
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d;
    if (const int rc = B.alloc(d, nf + nm)) return rc;
    float* const dm = d + nf;
    // pixels outside this call's buckets keep what the caller had in the buffers
    if (f->bucket_stride > 1 || f->bucket_first != 0) {
        HIP_TRY(hipMemcpy(d, feat, nf * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dm, motion, nm * sizeof(float), hipMemcpyHostToDevice));
    }
    const MotionCall mc{prev_T, dm};
    if (const int rc = run(s, f, n_samples, d, nullptr, st, &mc)) return rc;
    HIP_TRY(hipMemcpy(feat, d, nf * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(motion, dm, nm * sizeof(float), hipMemcpyDeviceToHost));
    return FRAYHIP_OK;
}

}  // extern "C"
