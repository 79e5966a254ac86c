// C ABI, resumable frames (include/frayhip.h "resumable frames"): frayhip_render_samples and frayhip_render_samples_device, and the device code
// behind them.  The frame's running per-pixel sum is a caller-held buffer (the state: one float4 row per pixel, row-major: sum.r, sum.g, sum.b and
// the second moment of the samples' luminance), so any call can render samples [first, first + count) of a frame that earlier calls began.  The
// tracing is the frame's own (render_impl<ST> with an accumulation request, accum.hpp); the kernels here take the place of its resolves.  FP32
// throughout; the Makefile builds this object with -ffp-contract=off, so every sum and product below is rounded where it is written
// (tests/samples_ref.py restates it in numpy).
//
//   k_acc_resolve_terms   the mono path tracer's resolve (k_pt_resolve_terms' arithmetic): per pixel, the row is read, every sample of the batch is folded
//                         from its terms innermost first and added in sample order, with the square of its luminance, and the row is written back
//   k_acc_resolve         the same over per-sample colours (k_pt_resolve's arithmetic: stereo frames, blended and saturated as there; the Whitted paths)
//   k_acc_black           maxTraceDepth < 0: +0 per sample, and the samples counted as k_black counts them
//   k_acc_mean            rgb = sum / (float)N and the noise estimate of the call's pixels: previews, the end of a call, a cancelled call
// A batch's resolve moves 16 bytes per pixel in and 16 out, whatever its number of samples; the frame's own moves 12 and 12 between batches.
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

// Every check of both entries, in this order; none touches the device.
int check(const char* who, frayhip_scene* s, const frayhip_frame* f, const frayhip_samples* r, const frayhip_progressive* p, const float* accum, const float* rgb,
          const float* noise, bool device)
{
    if (!f) return bad(who, "null frame");
    if (!r) return bad(who, "null request");
    if (!accum) return bad(who, "null accum");
    if (f->mode != FRAYHIP_MODE_RENDER) return bad(who, "mode must be FRAYHIP_MODE_RENDER");
    if (r->sample_first < 0) return bad(who, "sample_first must be >= 0");
    if (r->sample_count < 1) return bad(who, "sample_count must be >= 1");
    if ((long long)r->sample_first + r->sample_count > kMaxSamples) return bad(who, "sample_first + sample_count must be <= 2^24");
    if (p && std::isnan(p->preview_ms)) return bad(who, "preview_ms is NaN");
    if (device) {
        if (misaligned(accum, 16)) return bad(who, "device pointer to the state not 16-byte aligned");
        if (misaligned(rgb, 4) || misaligned(noise, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
    }
    if (!s) return bad(who, "null scene");
    if (s->rendering) return bad(who, "the scene is rendering a frame (a call from inside its progress callback?)");
    const DFrame F = frame_record(s, f->bucket_first, f->bucket_stride, f->seed);
    if (const int rc = check_bucket_range(who, F.nBuckets)) return rc;
    if (const int rc = check_pixel_cap(who, F.nBuckets)) return rc;
    if (!F.jitter && r->sample_first + r->sample_count > F.spp)
        return bad(who, "a frame without jittered samples has only its " + std::to_string(F.spp) + " sample(s): sample_first + sample_count is beyond them");
    const size_t n = (size_t)F.W * F.H;
    if (overlaps(rgb, 12 * n, accum, 16 * n)) return bad(who, "rgb must not overlap accum");
    if (overlaps(noise, 4 * n, accum, 16 * n)) return bad(who, "noise must not overlap accum");
    if (overlaps(noise, 4 * n, rgb, 12 * n)) return bad(who, "noise must not overlap rgb");
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
    if (const int rc = check("frayhip_render_samples_device", s, f, r, p, d_accum, d_rgb, d_noise, true)) return rc;
    AccumCall q;
    q.first = r->sample_first; q.count = r->sample_count; q.accum = d_accum; q.noise = d_noise;
    const Progress prog{p, nullptr};
    return run(s, f, r, p ? &prog : nullptr, q, d_rgb, (hipStream_t)hip_stream, st);
}

int frayhip_render_samples(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p, float* accum, float* rgb, float* noise,
                           frayhip_stats* st)
{
    const char* who = "frayhip_render_samples";
    if (const int rc = check(who, s, f, r, p, accum, rgb, noise, false)) return rc;
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

}  // extern "C"
