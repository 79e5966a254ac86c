// Host-side plumbing shared by the C entry points (capi*.hip, denoise.hip) and the per-flag-word drivers (render_impl, shade_impl, adaptive_impl):
// the `rendering` guard, the kernel flag word and its dispatch, the frame's records, the refusals the entries share, the counters of a call and
// the device arrays of a host entry.  Nothing here is device code.  Small things are inline; the rest is defined once in capi.hip.
#pragma once
#include <chrono>
#include <cstdint>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "render_state.hpp"

// The kernel flag words: bit 0 work counters, then Cube / CSG geometry (2), KD-tree meshes (4) or textures (8).  X(word, ...) once per word.
#define FRAY_FOR_EACH_ST(X, ...) X(0, __VA_ARGS__) X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__) X(8, __VA_ARGS__) X(9, __VA_ARGS__)
// `extern template` of a function template over the flag word, e.g. FRAY_EXTERN_ST(int shade_impl, (frayhip_scene*, const ShadeCall&)): each
// word's instantiation is in an object of its own (Makefile, ST_RULE)
#define FRAY_EXTERN_ONE(st, decl, args) extern template decl<st> args;
#define FRAY_EXTERN_ST(decl, args) FRAY_FOR_EACH_ST(FRAY_EXTERN_ONE, decl, args)

namespace frayhip_detail {

// who + ": " + why to frayhip_last_error()
int bad(const char* who, const std::string& why);              // FRAYHIP_E_ARG
int unsupported(const char* who, const std::string& why);      // FRAYHIP_E_UNSUPPORTED
inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
inline int no_work(frayhip_stats* st)
{
    if (st) *st = frayhip_stats{};
    return FRAYHIP_OK;
}

// A call holds the scene (`rendering`), so that nothing re-enters it from a progress callback; on a return while `armed` the stream is drained first.
struct Busy {
    frayhip_scene* s;
    hipStream_t stream;
    bool armed;
    Busy(frayhip_scene* x, hipStream_t st, bool drain = true) : s(x), stream(st), armed(drain) { s->rendering = true; }
    ~Busy() { if (armed) (void)hipStreamSynchronize(stream); s->rendering = false; }
};

// The flag word the scene was created with, and the counting bit of the call
inline int flag_word(const frayhip_scene* s, bool stats) { return (s->extGeometry ? 2 : s->kdMeshes ? 4 : s->textured ? 8 : 0) | (stats ? 1 : 0); }
// fn(std::integral_constant<int, ST>{}) for the flag word w
template <class Fn>
auto for_flag_word(int w, Fn&& fn)
{
#define FRAY_ST_CASE(k, ...) case k: return fn(std::integral_constant<int, k>{});
    switch (w) { FRAY_FOR_EACH_ST(FRAY_ST_CASE) }
#undef FRAY_ST_CASE
    __builtin_unreachable();
}

// acc: the accumulation request of frayhip_render_samples (accum.hpp), nullptr on every other entry
struct AccumCall;
template <int ST>
int render_impl(frayhip_scene* sc, const frayhip_frame* f, float* d_rgb, int32_t* d_id, double* d_dist, hipStream_t stream, frayhip_stats* st, const Progress* prog,
                AccumCall* acc);
FRAY_EXTERN_ST(int render_impl, (frayhip_scene*, const frayhip_frame*, float*, int32_t*, double*, hipStream_t, frayhip_stats*, const Progress*, AccumCall*))

// The frame's samples per pixel (main.cpp:395-400)
int frame_spp(const frayhip_scene* s);
// The scene record of a frame: the scene's with the view's ambient light, maxTraceDepth, gi and saturation
DScene frame_scene(const frayhip_scene* s);
// The host copy of the uploaded scene's node table (frayhip_scene_update keeps it current): S.nNodes records, inner pointers not to be followed
const DNode* host_nodes(const frayhip_scene* s);
// ... and of its shader table (S.nShaders records), kept current the same way
const DShader* host_shaders(const frayhip_scene* s);
// Size and bucket grid of a frame; frame_record: with the call's buckets (stride <= 0: 1; nBuckets < 0: a bad range) and the frame's spp, seed and jitter
inline DFrame frame_grid(int W, int H)
{
    DFrame F{};
    F.W = W; F.H = H;
    F.BW = (W - 1) / 48 + 1; F.BH = (H - 1) / 48 + 1;
    return F;
}
DFrame frame_record(const frayhip_scene* s, int bucketFirst, int bucketStride, uint32_t seed);
// Random words a camera sample may draw from one generator: lens samples and ten per Lambert bounce.  Up to 227 the generators are three registers.
inline bool long_generators(int maxTraceDepth) { return 8 + 10 * ((long long)maxTraceDepth + 2) > 227; }

// The refusals the frame entries share; 0 or the code, with the text set.  `by`: who does not support it ("adaptive frames").
int check_bucket_range(const char* who, int nBuckets);                                     // FRAYHIP_E_ARG
int check_pixel_cap(const char* who, int nBuckets);                                        // FRAYHIP_E_UNSUPPORTED, as the next two
int refuse_stereo(const char* who, const frayhip_scene* s);
int refuse_long_generators(const char* who, const frayhip_scene* s, const char* by);      // path tracing only

// The counters of a finished call: the sum of its DStats blocks (one, or the closest-hit and the any-hit kernels'), ms_kernels from evA / evB,
// ms_trace / ms_shadow and the launch counts from the first nTrace / nShadow events of the two pools (pairs), ms_total since t0.
frayhip_stats finish_stats(frayhip_scene* sc, const DStats* blocks, int nBlocks, size_t nTraceEvents, size_t nShadowEvents, std::chrono::steady_clock::time_point t0);

// Device arrays of a host entry, freed on every return.  `oom`: the text of a failed allocation.
struct DeviceArrays {
    std::string oom;
    std::vector<void*> ptrs;
    explicit DeviceArrays(std::string text) : oom(std::move(text)) {}
    DeviceArrays(const DeviceArrays&) = delete;
    ~DeviceArrays() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T> int alloc(T*& p, size_t count, bool want = true)
    {
        p = nullptr;
        if (!want || count == 0) return FRAYHIP_OK;
        void* q = nullptr;
        if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); set_error(oom); return FRAYHIP_E_NOMEM; }
        ptrs.push_back(q);
        p = (T*)q;
        return FRAYHIP_OK;
    }
};

// Carving a workspace into 256-byte aligned arrays
inline size_t r256(size_t b) { return (b + 255) / 256 * 256; }
struct Carve {
    unsigned char* p;
    unsigned char* take(size_t bytes) { unsigned char* r = p; p += r256(bytes); return r; }
};

}  // namespace frayhip_detail
