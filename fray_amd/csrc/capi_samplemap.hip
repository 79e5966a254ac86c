// C ABI, sample maps (include/frayhip.h "sample maps"): frayhip_render_samples_map and frayhip_render_samples_map_device, and the same for a pair of
// component states (frayhip_render_components_map and frayhip_render_components_map_device).  Argument checks, the
// scene's kernel flag word and the `rendering` guard; the layers, the kernels and the batch loop are samplemap_impl<ST> of samplemap_variant.hip
// (one object per flag word).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "samplemap.hpp"

namespace {

using namespace frayhip_detail;

bool overlaps(const void* a, size_t an, const void* b, size_t bn)
{
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

const char* kBadPlanes = "a pixel of the call's buckets has add < 0, count < 0 or count + add > 2^24";

// The second state of a component call and its two optional outputs
struct Indirect { const float *accum, *rgb, *noise; };

// Every check of the entries but the planes' values, in this order; none touches the device.  FRAYHIP_E_ARG for the arguments,
// FRAYHIP_E_UNSUPPORTED for a frame the map path does not render (Whitted, stereo, long generators).  `b`: the indirect state of a component call
// (accum, rgb and noise are then its direct state's), nullptr for a single-state call.
int check(const char* who, frayhip_scene* s, const frayhip_frame* f, const frayhip_samples_map* m, const float* accum, const int32_t* count, const int32_t* add,
          const float* rgb, const float* noise, const Indirect* b, bool device)
{
    if (!f) return bad(who, "null frame");
    if (!m) return bad(who, "null request");
    if (!accum) return bad(who, b ? "null accum_direct" : "null accum");
    if (b && !b->accum) return bad(who, "null accum_indirect");
    if (!count) return bad(who, "null count");
    if (!add) return bad(who, "null add");
    if (f->mode != FRAYHIP_MODE_RENDER) return bad(who, "mode must be FRAYHIP_MODE_RENDER");
    if (device) {
        if (misaligned(accum, 16) || (b && misaligned(b->accum, 16))) return bad(who, "device pointer to the state not 16-byte aligned");
        if (misaligned(count, 4) || misaligned(add, 4) || misaligned(rgb, 4) || misaligned(noise, 4) || (b && (misaligned(b->rgb, 4) || misaligned(b->noise, 4))))
            return bad(who, "device pointer to a plane not 4-byte aligned");
    }
    // the buffers, in the order the overlap messages name them; two that begin at one address overlap whatever the frame's size
    struct Buf { const void* p; size_t bytes; const char* name; };
    const Buf one[5] = {{accum, 16, "accum"}, {count, 4, "count"}, {add, 4, "add"}, {rgb, 12, "rgb"}, {noise, 4, "noise"}};
    const Buf two[8] = {{accum, 16, "accum_direct"}, {b ? b->accum : nullptr, 16, "accum_indirect"}, {count, 4, "count"}, {add, 4, "add"},
                        {rgb, 12, "rgb_direct"}, {b ? b->rgb : nullptr, 12, "rgb_indirect"}, {noise, 4, "noise_direct"}, {b ? b->noise : nullptr, 4, "noise_indirect"}};
    const Buf* bufs = b ? two : one;
    const int nBufs = b ? 8 : 5;
    auto overlap = [&](size_t n) -> std::string {          // n: the frame's pixels, 0: equal addresses only; empty: none
        for (int j = 1; j < nBufs; j++)
            for (int i = 0; i < j; i++)
                if (n ? overlaps(bufs[j].p, n * bufs[j].bytes, bufs[i].p, n * bufs[i].bytes) : (bufs[j].p && bufs[j].p == bufs[i].p))
                    return std::string(bufs[j].name) + " must not overlap " + bufs[i].name;
        return std::string();
    };
    {
        const std::string why = overlap(0);
        if (!why.empty()) return bad(who, why);
    }
    if (!s) return bad(who, "null scene");
    if (s->rendering) return bad(who, "the scene is rendering a frame (a call from inside its progress callback?)");
    const DFrame F = frame_record(s, f->bucket_first, f->bucket_stride, f->seed);
    if (const int rc = check_bucket_range(who, F.nBuckets)) return rc;
    const std::string why = overlap((size_t)F.W * F.H);
    if (!why.empty()) return bad(who, why);
    if (!s->settings.gi) return unsupported(who, "sample maps are path-traced; a Whitted frame (gi off) is not supported");
    if (const int rc = refuse_stereo(who, s)) return rc;
    if (const int rc = refuse_long_generators(who, s, b ? "component sample maps" : "sample maps")) return rc;
    if (const int rc = check_pixel_cap(who, F.nBuckets)) return rc;
    return FRAYHIP_OK;
}

// The host entry's check of the planes, over the pixels of the call's buckets (kernels.hpp item_pixel's bucket walk)
bool planes_ok(const DFrame& F, const int32_t* count, const int32_t* add)
{
    for (int k = 0; k < F.nBuckets; k++) {
        const int b = F.bucketFirst + k * F.bucketStride;
        const int by = b / F.BW, bx = (b - by * F.BW + FRAYHIP_BUCKET_SKEW * by) % F.BW;
        const int x1 = std::min(bx * 48 + 48, (int)F.W), y1 = std::min(by * 48 + 48, (int)F.H);
        for (int y = by * 48; y < y1; y++)
            for (int x = bx * 48; x < x1; x++) {
                const size_t p = (size_t)y * F.W + x;
                if (add[p] < 0 || count[p] < 0 || (long long)count[p] + add[p] > (long long)kMapMaxSamples) return false;
            }
    }
    return true;
}

SampleMapCall call_of(const frayhip_frame* f, float* accum, int32_t* count, const int32_t* add, float* rgb, float* noise)
{
    SampleMapCall q;
    q.bucketFirst = f->bucket_first;
    q.bucketStride = f->bucket_stride > 0 ? f->bucket_stride : 1;
    q.seed = f->seed;
    q.sppChunk = f->spp_chunk;
    q.stats = (f->flags & FRAYHIP_FRAME_STATS) != 0;
    q.accum = accum; q.count = count; q.add = add; q.rgb = rgb; q.noise = noise;
    return q;
}

// The scene's flag word with the counting bit from the frame; the stream is drained on every return.
int run(const char* who, frayhip_scene* s, SampleMapCall& q, hipStream_t stream, frayhip_samples_map* m, frayhip_stats* st)
{
    Busy busy(s, stream);
    const int rc = for_flag_word(flag_word(s, q.stats), [&](auto w) { return samplemap_impl<decltype(w)::value>(s, q, stream, st); });
    if (q.badPlanes) return bad(who, kBadPlanes);
    if (rc == FRAYHIP_OK) { m->samples = q.samples; m->count_min = q.countMin; m->count_max = q.countMax; }
    return rc;
}

}  // namespace

extern "C" {

int frayhip_render_samples_map_device(frayhip_scene* s, const frayhip_frame* f, frayhip_samples_map* m, float* d_accum, int32_t* d_count, const int32_t* d_add,
                                      float* d_rgb, float* d_noise, void* hip_stream, frayhip_stats* st)
{
    const char* who = "frayhip_render_samples_map_device";
    if (const int rc = check(who, s, f, m, d_accum, d_count, d_add, d_rgb, d_noise, nullptr, true)) return rc;
    SampleMapCall q = call_of(f, d_accum, d_count, d_add, d_rgb, d_noise);
    return run(who, s, q, (hipStream_t)hip_stream, m, st);
}

int frayhip_render_samples_map(frayhip_scene* s, const frayhip_frame* f, frayhip_samples_map* m, float* accum, int32_t* count, const int32_t* add, float* rgb,
                               float* noise, frayhip_stats* st)
{
    const char* who = "frayhip_render_samples_map";
    if (const int rc = check(who, s, f, m, accum, count, add, rgb, noise, nullptr, false)) return rc;
    if (!planes_ok(frame_record(s, f->bucket_first, f->bucket_stride, f->seed), count, add)) return bad(who, kBadPlanes);
    const size_t n = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    DeviceArrays B("frayhip_render_samples_map: out of device memory");
    float *d_accum, *d_rgb, *d_noise;
    int32_t *d_count, *d_add;
    if (const int rc = B.alloc(d_accum, 4 * n)) return rc;
    if (const int rc = B.alloc(d_count, n)) return rc;
    if (const int rc = B.alloc(d_add, n)) return rc;
    if (const int rc = B.alloc(d_rgb, 3 * n, rgb != nullptr)) return rc;
    if (const int rc = B.alloc(d_noise, n, noise != nullptr)) return rc;
    // the state and the planes go in whole; rgb and noise only when the call renders a subset of the buckets, so that the other pixels keep
    // their values (render_host's rule)
    HIP_TRY(hipMemcpy(d_accum, accum, n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, count, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_add, add, n * 4, hipMemcpyHostToDevice));
    if (f->bucket_stride > 1 || f->bucket_first != 0) {
        if (d_rgb) HIP_TRY(hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice));
        if (d_noise) HIP_TRY(hipMemcpy(d_noise, noise, n * 4, hipMemcpyHostToDevice));
    }
    SampleMapCall q = call_of(f, d_accum, d_count, d_add, d_rgb, d_noise);
    if (const int rc = run(who, s, q, nullptr, m, st)) return rc;
    HIP_TRY(hipMemcpy(accum, d_accum, n * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count, d_count, n * 4, hipMemcpyDeviceToHost));
    if (d_rgb) HIP_TRY(hipMemcpy(rgb, d_rgb, n * 12, hipMemcpyDeviceToHost));
    if (d_noise) HIP_TRY(hipMemcpy(noise, d_noise, n * 4, hipMemcpyDeviceToHost));
    return FRAYHIP_OK;
}

int frayhip_render_components_map_device(frayhip_scene* s, const frayhip_frame* f, frayhip_samples_map* m, float* d_accum_direct, float* d_accum_indirect,
                                         int32_t* d_count, const int32_t* d_add, float* d_rgb_direct, float* d_rgb_indirect, float* d_noise_direct,
                                         float* d_noise_indirect, void* hip_stream, frayhip_stats* st)
{
    const char* who = "frayhip_render_components_map_device";
    const Indirect indirect{d_accum_indirect, d_rgb_indirect, d_noise_indirect};
    if (const int rc = check(who, s, f, m, d_accum_direct, d_count, d_add, d_rgb_direct, d_noise_direct, &indirect, true)) return rc;
    SampleMapCall q = call_of(f, d_accum_direct, d_count, d_add, d_rgb_direct, d_noise_direct);
    q.accumIndirect = d_accum_indirect; q.rgbIndirect = d_rgb_indirect; q.noiseIndirect = d_noise_indirect;
    return run(who, s, q, (hipStream_t)hip_stream, m, st);
}

int frayhip_render_components_map(frayhip_scene* s, const frayhip_frame* f, frayhip_samples_map* m, float* accum_direct, float* accum_indirect, int32_t* count,
                                  const int32_t* add, float* rgb_direct, float* rgb_indirect, float* noise_direct, float* noise_indirect, frayhip_stats* st)
{
    const char* who = "frayhip_render_components_map";
    const Indirect indirect{accum_indirect, rgb_indirect, noise_indirect};
    if (const int rc = check(who, s, f, m, accum_direct, count, add, rgb_direct, noise_direct, &indirect, false)) return rc;
    if (!planes_ok(frame_record(s, f->bucket_first, f->bucket_stride, f->seed), count, add)) return bad(who, kBadPlanes);
    const size_t n = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    DeviceArrays B("frayhip_render_components_map: out of device memory");
    // per state: the state, its rgb and its noise (frayhip_render_samples_map's copy-in rule for each)
    float* host[2][3] = {{accum_direct, rgb_direct, noise_direct}, {accum_indirect, rgb_indirect, noise_indirect}};
    float* dev[2][3];
    const size_t floats[3] = {4 * n, 3 * n, n};
    int32_t *d_count, *d_add;
    const bool subset = f->bucket_stride > 1 || f->bucket_first != 0;
    for (int k = 0; k < 2; k++)
        for (int c = 0; c < 3; c++) {
            if (const int rc = B.alloc(dev[k][c], floats[c], host[k][c] != nullptr)) return rc;
            if (dev[k][c] && (subset || c == 0)) HIP_TRY(hipMemcpy(dev[k][c], host[k][c], floats[c] * 4, hipMemcpyHostToDevice));
        }
    if (const int rc = B.alloc(d_count, n)) return rc;
    if (const int rc = B.alloc(d_add, n)) return rc;
    HIP_TRY(hipMemcpy(d_count, count, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_add, add, n * 4, hipMemcpyHostToDevice));
    SampleMapCall q = call_of(f, dev[0][0], d_count, d_add, dev[0][1], dev[0][2]);
    q.accumIndirect = dev[1][0]; q.rgbIndirect = dev[1][1]; q.noiseIndirect = dev[1][2];
    if (const int rc = run(who, s, q, nullptr, m, st)) return rc;
    for (int k = 0; k < 2; k++)
        for (int c = 0; c < 3; c++)
            if (dev[k][c]) HIP_TRY(hipMemcpy(host[k][c], dev[k][c], floats[c] * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count, d_count, n * 4, hipMemcpyDeviceToHost));
    return FRAYHIP_OK;
}

}  // extern "C"
