// C ABI, resumable frames (include/frayhip.h "resumable frames"): frayhip_render_samples and frayhip_render_samples_device, component frames
// ("component frames": frayhip_render_components and frayhip_render_components_device), and the device code behind them.  The frame's running per-pixel sum is a caller-held buffer (the state: one float4 row per pixel, row-major: sum.r, sum.g, sum.b and
// the second moment of the samples' luminance), so any call can render samples [first, first + count) of a frame that earlier calls began.  The
// tracing is the frame's own (render_impl<ST> with an accumulation request, accum.hpp); the kernels here take the place of its resolves.  FP32
// throughout; the Makefile builds this object with -ffp-contract=off, so every sum and product below is rounded where it is written
// (tests/samples_ref.py restates it in numpy).
//
//   k_acc_resolve_terms   the mono path tracer's resolve (k_pt_resolve_terms' arithmetic): per pixel, the row is read, every sample of the batch is folded
//                         from its terms innermost first and added in sample order, with the square of its luminance, and the row is written back
//   k_acc_resolve_terms_split  the same into two states (include/frayhip.h "component frames": frayhip_render_components): a sample's term 0, as it
//                         is stored, into the direct state, and the fold of its terms 1 .. n-1 into the indirect one; their FP32 sum is the colour above
//   k_acc_resolve         the same over per-sample colours (k_pt_resolve's arithmetic: stereo frames, blended and saturated as there; the Whitted paths)
//   k_acc_black           maxTraceDepth < 0: +0 per sample, and the samples counted as k_black counts them
//   k_acc_mean            rgb = sum / (float)N and the noise estimate of the call's pixels: previews, the end of a call, a cancelled call
// A batch's resolve moves 16 bytes per pixel in and 16 out, whatever its number of samples (the split one 32 and 32); the frame's own moves 12 and 12
// between batches.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>

#include "accum.hpp"
#include "entry_support.hpp"
#include "kernels.hpp"

static_assert(FRAYHIP_ACCUM_CHANNELS == 4, "a state row is one float4");

// Color::intensity (color.h:79-82) in the order the header gives: ((r + g) + b) / 3
FD float acc_lum(C3 c) { return ((c.r + c.g) + c.b) / 3.0f; }

// The row of pixel (x, y) at the head of batch s0: the frame's sum starts as c3(0, 0, 0) and its first addition is 0 + c_0
FD float4 acc_load(const DFrame& F, const float4* accum, int x, int y, int s0)
{
    return s0 == 0 ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : accum[(size_t)y * F.W + x];
}
FD void acc_add(float4& row, C3 c)
{
    const C3 a = c3(row.x, row.y, row.z) + c;
    const float l = acc_lum(c);
    row.x = a.r; row.y = a.g; row.z = a.b;
    row.w = row.w + l * l;
}

static __global__ __launch_bounds__(256) void k_acc_resolve_terms(DFrame F, int nItems, int s0, int chunk, TermBuf TB, float4* __restrict__ accum)
{
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        float4 row = acc_load(F, accum, x, y, s0);
        for (int s = 0; s < chunk; s++) {
            const uint32_t slot = (uint32_t)s * (uint32_t)nItems + (uint32_t)item;
            const int n = (int)TB.n[slot];
            C3 result = c3(0, 0, 0);
            if (n <= 8) {
                // up to eight terms: every load issued before the first addition, as k_pt_resolve_terms does (the same additions in the same order)
                float tr[8], tg[8], tb[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    tr[k] = tg[k] = tb[k] = 0.0f;
                    if (k < n) {
                        const size_t q = (size_t)k * 3 * TB.nPaths + slot;
                        tr[k] = TB.t[q]; tg[k] = TB.t[q + TB.nPaths]; tb[k] = TB.t[q + 2 * (size_t)TB.nPaths];
                    }
                }
#pragma unroll
                for (int k = 7; k >= 0; k--)
                    if (k < n) result = c3(tr[k], tg[k], tb[k]) + result;
            } else {
                for (int k = n - 1; k >= 0; k--) {
                    const size_t q = (size_t)k * 3 * TB.nPaths + slot;
                    result = c3(TB.t[q], TB.t[q + TB.nPaths], TB.t[q + 2 * (size_t)TB.nPaths]) + result;
                }
            }
            acc_add(row, result);
        }
        accum[(size_t)y * F.W + x] = row;
    }
}

// Two rows per pixel.  The additions are k_acc_resolve_terms' but for the last one of a sample, t[0] + fold(t[1 .. n-1]), which is left to the caller:
// d = t[0] goes into `direct` and the fold, begun at c3(0, 0, 0), into `indirect` (n == 1: +0).
static __global__ __launch_bounds__(256) void k_acc_resolve_terms_split(DFrame F, int nItems, int s0, int chunk, TermBuf TB, float4* __restrict__ direct,
                                                                 float4* __restrict__ indirect)
{
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        float4 rowD = acc_load(F, direct, x, y, s0), rowI = acc_load(F, indirect, x, y, s0);
        for (int s = 0; s < chunk; s++) {
            const uint32_t slot = (uint32_t)s * (uint32_t)nItems + (uint32_t)item;
            const int n = (int)TB.n[slot];
            C3 first = c3(0, 0, 0), result = c3(0, 0, 0);
            if (n <= 8) {
                // up to eight terms: every load issued before the first addition
                float tr[8], tg[8], tb[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    tr[k] = tg[k] = tb[k] = 0.0f;
                    if (k < n) {
                        const size_t q = (size_t)k * 3 * TB.nPaths + slot;
                        tr[k] = TB.t[q]; tg[k] = TB.t[q + TB.nPaths]; tb[k] = TB.t[q + 2 * (size_t)TB.nPaths];
                    }
                }
#pragma unroll
                for (int k = 7; k >= 1; k--)
                    if (k < n) result = c3(tr[k], tg[k], tb[k]) + result;
                first = c3(tr[0], tg[0], tb[0]);
            } else {
                for (int k = n - 1; k >= 1; k--) {
                    const size_t q = (size_t)k * 3 * TB.nPaths + slot;
                    result = c3(TB.t[q], TB.t[q + TB.nPaths], TB.t[q + 2 * (size_t)TB.nPaths]) + result;
                }
                first = c3(TB.t[slot], TB.t[slot + TB.nPaths], TB.t[slot + 2 * (size_t)TB.nPaths]);
            }
            acc_add(rowD, first);
            acc_add(rowI, result);
        }
        direct[(size_t)y * F.W + x] = rowD;
        indirect[(size_t)y * F.W + x] = rowI;
    }
}

static __global__ __launch_bounds__(256) void k_acc_resolve(DFrame F, DCamera C, float saturation, int nItems, int s0, int chunk, const float* __restrict__ sampleRad,
                                                     const float* __restrict__ sampleRadR, float4* __restrict__ accum)
{
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        float4 row = acc_load(F, accum, x, y, s0);
        for (int s = 0; s < chunk; s++) {
            const size_t q = ((size_t)s * nItems + item) * 3;
            C3 cl = c3(sampleRad[q], sampleRad[q + 1], sampleRad[q + 2]);
            if (sampleRadR) {                                 // anaglyph blend, main.cpp:306-317, as k_pt_resolve writes it
                C3 cr = c3(sampleRadR[q], sampleRadR[q + 1], sampleRadR[q + 2]);
                if (saturation != 1) {                        // Color::adjustSaturation, color.h:127-133
                    float ml = (cl.r + cl.g + cl.b) / 3.0f, mr = (cr.r + cr.g + cr.b) / 3.0f;
                    cl = c3(ml + (cl.r - ml) * saturation, ml + (cl.g - ml) * saturation, ml + (cl.b - ml) * saturation);
                    cr = c3(mr + (cr.r - mr) * saturation, mr + (cr.g - mr) * saturation, mr + (cr.b - mr) * saturation);
                }
                cl = cl * ldc(C.leftMask) + cr * ldc(C.rightMask);
            }
            acc_add(row, cl);
        }
        accum[(size_t)y * F.W + x] = row;
    }
}

static __global__ __launch_bounds__(256) void k_acc_black(DFrame F, int nItems, int s0, int chunk, int eyes, float4* __restrict__ accum, DStats* st)
{
    unsigned long long n = 0;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        float4 row = acc_load(F, accum, x, y, s0);
        acc_add(row, c3(0, 0, 0));          // chunk >= 1 additions of +0: the second and later ones change nothing (x + 0 == x once -0 has become +0)
        accum[(size_t)y * F.W + x] = row;
        n += (unsigned long long)(chunk * eyes);
    }
    if (n) atomicAdd(&st->samples, n);
}

static __global__ __launch_bounds__(256) void k_acc_mean(DFrame F, int nItems, int n, const float4* __restrict__ accum, float* __restrict__ rgb, float* __restrict__ noise)
{
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        const size_t p = (size_t)y * F.W + x;
        const float4 row = accum[p];
        const C3 a = c3(row.x, row.y, row.z) / (float)n;          // the frame's own division
        if (rgb) { rgb[p * 3] = a.r; rgb[p * 3 + 1] = a.g; rgb[p * 3 + 2] = a.b; }
        if (noise) {
            const float lbar = acc_lum(a);
            const float v = fmaxf(0.0f, row.w / (float)n - lbar * lbar);
            noise[p] = n >= 2 ? v / (float)(n - 1) : lbar * lbar;
        }
    }
}

namespace {

using namespace frayhip_detail;

bool overlaps(const void* a, size_t an, const void* b, size_t bn)
{
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

constexpr int kMaxSamples = 1 << 24;          // (float)N is exact up to here

// The buffers of one state: the state and its two optional outputs
struct StateBufs { const float *accum, *rgb, *noise; };

// Every check of the entries, in this order; none touches the device.  `b` is the second state of a component call (a is then its direct state, b its
// indirect one), nullptr for a resumable call.
int check(const char* who, frayhip_scene* s, const frayhip_frame* f, const frayhip_samples* r, const frayhip_progressive* p, const StateBufs& a, const StateBufs* b,
          bool device)
{
    if (!f) return bad(who, "null frame");
    if (!r) return bad(who, "null request");
    if (!a.accum) return bad(who, b ? "null accum_direct" : "null accum");
    if (b && !b->accum) return bad(who, "null accum_indirect");
    if (f->mode != FRAYHIP_MODE_RENDER) return bad(who, "mode must be FRAYHIP_MODE_RENDER");
    if (r->sample_first < 0) return bad(who, "sample_first must be >= 0");
    if (r->sample_count < 1) return bad(who, "sample_count must be >= 1");
    if ((long long)r->sample_first + r->sample_count > kMaxSamples) return bad(who, "sample_first + sample_count must be <= 2^24");
    if (p && std::isnan(p->preview_ms)) return bad(who, "preview_ms is NaN");
    if (b && p && p->preview_ms >= 0) return bad(who, "previews are not offered: preview_ms must be negative");
    if (device) {
        if (misaligned(a.accum, 16) || (b && misaligned(b->accum, 16))) return bad(who, "device pointer to the state not 16-byte aligned");
        if (misaligned(a.rgb, 4) || misaligned(a.noise, 4) || (b && (misaligned(b->rgb, 4) || misaligned(b->noise, 4))))
            return bad(who, "device pointer to floats not 4-byte aligned");
    }
    // the buffers, in the order the overlap messages name them; two of a component call that begin at one address overlap whatever the frame's size
    struct Buf { const float* p; size_t floats; const char* name; };
    const Buf one[3] = {{a.accum, 4, "accum"}, {a.rgb, 3, "rgb"}, {a.noise, 1, "noise"}};
    const Buf two[6] = {{a.accum, 4, "accum_direct"}, {b ? b->accum : nullptr, 4, "accum_indirect"}, {a.rgb, 3, "rgb_direct"},
                        {b ? b->rgb : nullptr, 3, "rgb_indirect"}, {a.noise, 1, "noise_direct"}, {b ? b->noise : nullptr, 1, "noise_indirect"}};
    const Buf* bufs = b ? two : one;
    const int nBufs = b ? 6 : 3;
    auto overlap = [&](size_t n) -> std::string {          // n: the frame's pixels, 0: equal addresses only; empty: none
        for (int j = 1; j < nBufs; j++)
            for (int i = 0; i < j; i++)
                if (n ? overlaps(bufs[j].p, 4 * n * bufs[j].floats, bufs[i].p, 4 * n * bufs[i].floats) : (bufs[j].p && bufs[j].p == bufs[i].p))
                    return std::string(bufs[j].name) + " must not overlap " + bufs[i].name;
        return std::string();
    };
    if (b) {
        const std::string why = overlap(0);
        if (!why.empty()) return bad(who, why);
    }
    if (!s) return bad(who, "null scene");
    if (s->rendering) return bad(who, "the scene is rendering a frame (a call from inside its progress callback?)");
    if (b) {
        // a Whitted frame has no term list, and a stereo frame's resolve blends per-sample eye colours
        if (!s->settings.gi) return unsupported(who, "component frames need a path-traced frame (settings.gi)");
        if (s->camera.stereoSeparation > 0) return unsupported(who, "component frames are not offered for stereo frames");
    }
    const DFrame F = frame_record(s, f->bucket_first, f->bucket_stride, f->seed);
    if (const int rc = check_bucket_range(who, F.nBuckets)) return rc;
    if (const int rc = check_pixel_cap(who, F.nBuckets)) return rc;
    if (!F.jitter && r->sample_first + r->sample_count > F.spp)
        return bad(who, "a frame without jittered samples has only its " + std::to_string(F.spp) + " sample(s): sample_first + sample_count is beyond them");
    const std::string why = overlap((size_t)F.W * F.H);
    if (!why.empty()) return bad(who, why);
    return FRAYHIP_OK;
}

// The scene's flag word with the counting bit from the frame; render_impl drains its lanes itself on an early return.
int run(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const Progress* prog, AccumCall& q, float* d_rgb, hipStream_t stream, frayhip_stats* st)
{
    Busy busy(s, stream, false);
    const int rc = for_flag_word(flag_word(s, (f->flags & FRAYHIP_FRAME_STATS) != 0), [&](auto w) {
        return render_impl<decltype(w)::value>(s, f, d_rgb, nullptr, nullptr, stream, st, prog, &q);
    });
    if (rc == FRAYHIP_OK || rc == FRAYHIP_E_CANCELLED) r->samples_done = q.done;
    return rc;
}

}  // namespace

namespace frayhip_detail {

void launch_acc_resolve_terms(int grid, hipStream_t stream, const DFrame& F, int nItems, int s0, int chunk, const TermBuf& TB, float* accum)
{
    hipLaunchKernelGGL(k_acc_resolve_terms, dim3(grid), dim3(256), 0, stream, F, nItems, s0, chunk, TB, (float4*)accum);
}
void launch_acc_resolve_terms_split(int grid, hipStream_t stream, const DFrame& F, int nItems, int s0, int chunk, const TermBuf& TB, float* direct, float* indirect)
{
    hipLaunchKernelGGL(k_acc_resolve_terms_split, dim3(grid), dim3(256), 0, stream, F, nItems, s0, chunk, TB, (float4*)direct, (float4*)indirect);
}
void launch_acc_resolve(int grid, hipStream_t stream, const DFrame& F, const DCamera& C, float saturation, int nItems, int s0, int chunk, const float* sampleRad,
                        const float* sampleRadR, float* accum)
{
    hipLaunchKernelGGL(k_acc_resolve, dim3(grid), dim3(256), 0, stream, F, C, saturation, nItems, s0, chunk, sampleRad, sampleRadR, (float4*)accum);
}
void launch_acc_black(int grid, hipStream_t stream, const DFrame& F, int nItems, int s0, int chunk, int eyes, float* accum, DStats* st)
{
    hipLaunchKernelGGL(k_acc_black, dim3(grid), dim3(256), 0, stream, F, nItems, s0, chunk, eyes, (float4*)accum, st);
}
void launch_acc_mean(int grid, hipStream_t stream, const DFrame& F, int nItems, int n, const float* accum, float* rgb, float* noise)
{
    hipLaunchKernelGGL(k_acc_mean, dim3(grid), dim3(256), 0, stream, F, nItems, n, (const float4*)accum, rgb, noise);
}

}  // namespace frayhip_detail

extern "C" {

int frayhip_render_samples_device(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p, float* d_accum, float* d_rgb,
                                  float* d_noise, void* hip_stream, frayhip_stats* st)
{
    if (const int rc = check("frayhip_render_samples_device", s, f, r, p, StateBufs{d_accum, d_rgb, d_noise}, nullptr, true)) return rc;
    AccumCall q;
    q.first = r->sample_first; q.count = r->sample_count; q.accum = d_accum; q.noise = d_noise;
    const Progress prog{p, nullptr};
    return run(s, f, r, p ? &prog : nullptr, q, d_rgb, (hipStream_t)hip_stream, st);
}

int frayhip_render_samples(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p, float* accum, float* rgb, float* noise,
                           frayhip_stats* st)
{
    const char* who = "frayhip_render_samples";
    if (const int rc = check(who, s, f, r, p, StateBufs{accum, rgb, noise}, nullptr, false)) return rc;
    const size_t n = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    DeviceArrays B("frayhip_render_samples: out of device memory");
    float *d_accum, *d_rgb, *d_noise;
    if (const int rc = B.alloc(d_accum, 4 * n)) return rc;
    if (const int rc = B.alloc(d_rgb, 3 * n, rgb != nullptr)) return rc;
    if (const int rc = B.alloc(d_noise, n, noise != nullptr)) return rc;
    // the state goes in only when it holds samples; pixels outside this call's buckets keep what the caller had in all three buffers (render_host's rule)
    const bool subset = f->bucket_stride > 1 || f->bucket_first != 0;
    if (r->sample_first > 0 || subset) HIP_TRY(hipMemcpy(d_accum, accum, n * 16, hipMemcpyHostToDevice));
    if (subset) {
        if (d_rgb) HIP_TRY(hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice));
        if (d_noise) HIP_TRY(hipMemcpy(d_noise, noise, n * 4, hipMemcpyHostToDevice));
    }
    AccumCall q;
    q.first = r->sample_first; q.count = r->sample_count; q.accum = d_accum; q.noise = d_noise;
    const Progress prog{p, rgb};
    const int rc = run(s, f, r, p ? &prog : nullptr, q, d_rgb, nullptr, st);
    if (rc != FRAYHIP_OK && rc != FRAYHIP_E_CANCELLED) return rc;
    HIP_TRY(hipMemcpy(accum, d_accum, n * 16, hipMemcpyDeviceToHost));
    if (d_rgb && !p) HIP_TRY(hipMemcpy(rgb, d_rgb, n * 12, hipMemcpyDeviceToHost));          // with a progress request the frame was copied before the final callback
    if (d_noise) HIP_TRY(hipMemcpy(noise, d_noise, n * 4, hipMemcpyDeviceToHost));
    return rc;
}

int frayhip_render_components_device(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p, float* d_accum_direct,
                                     float* d_accum_indirect, float* d_rgb_direct, float* d_rgb_indirect, float* d_noise_direct, float* d_noise_indirect,
                                     void* hip_stream, frayhip_stats* st)
{
    const char* who = "frayhip_render_components_device";
    const StateBufs indirect{d_accum_indirect, d_rgb_indirect, d_noise_indirect};
    if (const int rc = check(who, s, f, r, p, StateBufs{d_accum_direct, d_rgb_direct, d_noise_direct}, &indirect, true)) return rc;
    AccumCall q;
    q.who = who;
    q.first = r->sample_first; q.count = r->sample_count;
    q.accum = d_accum_direct; q.rgb1 = d_rgb_direct; q.noise = d_noise_direct;
    q.accum2 = d_accum_indirect; q.rgb2 = d_rgb_indirect; q.noise2 = d_noise_indirect;
    const Progress prog{p, nullptr};
    return run(s, f, r, p ? &prog : nullptr, q, nullptr, (hipStream_t)hip_stream, st);
}

int frayhip_render_components(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p, float* accum_direct, float* accum_indirect,
                              float* rgb_direct, float* rgb_indirect, float* noise_direct, float* noise_indirect, frayhip_stats* st)
{
    const char* who = "frayhip_render_components";
    const StateBufs indirect{accum_indirect, rgb_indirect, noise_indirect};
    if (const int rc = check(who, s, f, r, p, StateBufs{accum_direct, rgb_direct, noise_direct}, &indirect, false)) return rc;
    const size_t n = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    DeviceArrays B("frayhip_render_components: out of device memory");
    // per state: the state, its rgb and its noise (frayhip_render_samples' copy-in rule for each)
    float* host[2][3] = {{accum_direct, rgb_direct, noise_direct}, {accum_indirect, rgb_indirect, noise_indirect}};
    float* dev[2][3];
    const size_t floats[3] = {4 * n, 3 * n, n};
    const bool subset = f->bucket_stride > 1 || f->bucket_first != 0;
    for (int k = 0; k < 2; k++)
        for (int c = 0; c < 3; c++) {
            if (const int rc = B.alloc(dev[k][c], floats[c], host[k][c] != nullptr)) return rc;
            if (dev[k][c] && (subset || (c == 0 && r->sample_first > 0))) HIP_TRY(hipMemcpy(dev[k][c], host[k][c], floats[c] * 4, hipMemcpyHostToDevice));
        }
    AccumCall q;
    q.who = who;
    q.first = r->sample_first; q.count = r->sample_count;
    q.accum = dev[0][0]; q.rgb1 = dev[0][1]; q.noise = dev[0][2];
    q.accum2 = dev[1][0]; q.rgb2 = dev[1][1]; q.noise2 = dev[1][2];
    const Progress prog{p, nullptr};
    const int rc = run(s, f, r, p ? &prog : nullptr, q, nullptr, nullptr, st);
    if (rc != FRAYHIP_OK && rc != FRAYHIP_E_CANCELLED) return rc;
    for (int k = 0; k < 2; k++)
        for (int c = 0; c < 3; c++)
            if (dev[k][c]) HIP_TRY(hipMemcpy(host[k][c], dev[k][c], floats[c] * 4, hipMemcpyDeviceToHost));
    return rc;
}

}  // extern "C"
