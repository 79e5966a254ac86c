// C ABI, change frames (include/frayhip.h "change frames"): frayhip_change_defaults, frayhip_change_frame and its _device entry.  Two resumable
// states that hold the same samples of one seed and view, taken before and after an edit of the scene, differ by exactly zero in a pixel none
// of whose paths met anything that changed; the change frame is the windowed relative difference of their luminance sums, which
// frayhip_temporal_accumulate_adaptive (temporal.hip) takes to shorten the history.  Scene-free, FP32 throughout; the Makefile builds this
// object as it builds denoise.o (-ffp-contract=off, correctly rounded divide), so every sum below is rounded where it is written
// (tests/change_ref.py restates it in numpy, and the two agree bit for bit).
//
//   k_ch_frame   per pixel: the window's sum of |lb - la| over its sum of max(la, lb), times the gain, clamped to 1.  The shape of k_tp_variance:
//                a 16x16 block stages the (d, m) pairs of the 22x22 texels its windows can reach in LDS (each state row read once, as a
//                float4), then each thread sums its (2 radius + 1)^2 window from the tile, j outer, i inner
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>

#include "entry_support.hpp"
#include "temporal_common.hpp"

struct ChangeCall {
    int W, H;
    const float4* before;       // one row a pixel: {sum.rgb, m2}
    const float4* after;
    const float4* motion;       // null, or two rows a pixel: row 0's w is `moved`
    float* change;
    int radius;
    float gain;
};

// A 16x16 block and the 22x22 texels the widest window reaches: {d, m}, 8 bytes a texel, 3872 bytes of LDS
#define FRAY_CH_MAX_RADIUS 3
#define FRAY_CH_TILE_SIDE 22            // 16 + 2 * FRAY_CH_MAX_RADIUS

static __global__ __launch_bounds__(256) void k_ch_frame(ChangeCall T)
{
    const int W = T.W, H = T.H;
    __shared__ float2 tile[FRAY_CH_TILE_SIDE * FRAY_CH_TILE_SIDE];
    const int tilesX = (W + 15) / 16;                // the tiles in row-major order along grid x, as k_tp_variance's
    const int bx = (int)(blockIdx.x % (unsigned)tilesX) * 16, by = (int)(blockIdx.x / (unsigned)tilesX) * 16;
    const int lx = (int)threadIdx.x & 15, ly = (int)threadIdx.x >> 4;
    const int x = bx + lx, y = by + ly;
    for (int t = (int)threadIdx.x; t < FRAY_CH_TILE_SIDE * FRAY_CH_TILE_SIDE; t += 256) {
        const int ty = t / FRAY_CH_TILE_SIDE, tx = t - ty * FRAY_CH_TILE_SIDE;
        const int xq = bx + tx - FRAY_CH_MAX_RADIUS, yq = by + ty - FRAY_CH_MAX_RADIUS;
        if (xq >= 0 && xq < W && yq >= 0 && yq < H) {
            const size_t q = (size_t)yq * W + xq;
            const float4 a = T.before[q], b = T.after[q];
            const float la = tp_lum(a.x, a.y, a.z), lb = tp_lum(b.x, b.y, b.z);
            float m = fmaxf(la, lb), d = fabsf(lb - la);
            bool keep = isfinite(la) && isfinite(lb) && m > 0.0f;
            if (keep && T.motion) keep = T.motion[2 * q].w == 0.0f;
            if (!keep) { d = 0.0f; m = 0.0f; }
            tile[t] = make_float2(d, m);
        }
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const int r = T.radius;
    float sd = 0.0f, sm = 0.0f;
    for (int j = -r; j <= r; j++) {
        const int yq = y + j;
        if (yq < 0 || yq >= H) continue;
        for (int i = -r; i <= r; i++) {
            const int xq = x + i;
            if (xq < 0 || xq >= W) continue;
            const float2 q = tile[(ly + FRAY_CH_MAX_RADIUS + j) * FRAY_CH_TILE_SIDE + (lx + FRAY_CH_MAX_RADIUS + i)];
            sd += q.x; sm += q.y;
        }
    }
    T.change[(size_t)y * W + x] = sm > 0.0f ? fminf(1.0f, T.gain * (sd / sm)) : 0.0f;
}

namespace {

using namespace frayhip_detail;
using namespace frayhip_temporal_detail;

// Every check of both entries, in this order; none touches the device
int check(const char* who, int W, int H, const float* before, const float* after, const float* motion, const struct frayhip_change* p, const float* change,
          bool device)
{
    if (W < 1 || H < 1) return bad(who, "width and height must be >= 1");
    if ((long long)W * H > (1ll << 30)) return bad(who, "more than 2^30 pixels");
    if (!before) return bad(who, "null accum_before");
    if (!after) return bad(who, "null accum_after");
    if (!p) return bad(who, "null parameters");
    if (!change) return bad(who, "null change");
    if (p->radius < 0 || p->radius > FRAY_CH_MAX_RADIUS) return bad(who, "radius must be 0..3");
    if (!std::isfinite(p->gain) || !(p->gain > 0)) return bad(who, "gain must be finite and > 0");
    if (device) {
        if (misaligned(before, 16) || misaligned(after, 16)) return bad(who, "device pointer to a state not 16-byte aligned");
        if (misaligned(motion, 16)) return bad(who, "device pointer to a motion frame not 16-byte aligned");
        if (misaligned(change, 4)) return bad(who, "device pointer to floats not 4-byte aligned");
    }
    const size_t n = (size_t)W * H;
    const struct { const void* q; size_t bytes; } ins[3] = {{before, 4 * FRAYHIP_ACCUM_CHANNELS * n}, {after, 4 * FRAYHIP_ACCUM_CHANNELS * n},
                                                            {motion, 4 * FRAYHIP_MOTION_CHANNELS * n}};
    for (const auto& in : ins)
        if (overlaps(change, 4 * n, in.q, in.bytes)) return bad(who, "change must not overlap an input");
    return FRAYHIP_OK;
}

// The device path of both entries (device pointers, checked)
int run(int W, int H, const float* before, const float* after, const float* motion, const struct frayhip_change* p, float* change, hipStream_t stream,
        frayhip_stats* st, std::chrono::steady_clock::time_point t0)
{
    ChangeCall T{};
    T.W = W; T.H = H;
    T.before = (const float4*)before; T.after = (const float4*)after; T.motion = (const float4*)motion;
    T.change = change;
    T.radius = p->radius; T.gain = p->gain;
    Events E;
    HIP_TRY(hipEventCreate(&E.a));
    HIP_TRY(hipEventCreate(&E.b));
    struct Drain { hipStream_t s; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(s); } } drain{stream};
    HIP_TRY(hipEventRecord(E.a, stream));
    hipLaunchKernelGGL(k_ch_frame, dim3((unsigned)((W + 15) / 16) * (unsigned)((H + 15) / 16)), dim3(256), 0, stream, T);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(E.b, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    if (st) {
        frayhip_stats o{};
        float ms = 0;
        (void)hipEventElapsedTime(&ms, E.a, E.b);
        o.ms_kernels = ms;
        o.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *st = o;
    }
    return FRAYHIP_OK;
}

}  // namespace

extern "C" {

int frayhip_change_defaults(struct frayhip_change* p)
{
    if (!p) return bad("frayhip_change_defaults", "null parameters");
    p->radius = 3;
    p->gain = 1.0f;
    return FRAYHIP_OK;
}

int frayhip_change_frame_device(int width, int height, const float* d_accum_before, const float* d_accum_after, const float* d_motion,
                                const struct frayhip_change* p, float* d_change, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = check("frayhip_change_frame_device", width, height, d_accum_before, d_accum_after, d_motion, p, d_change, true)) return rc;
    return run(width, height, d_accum_before, d_accum_after, d_motion, p, d_change, (hipStream_t)hip_stream, st, t0);
}

int frayhip_change_frame(int width, int height, const float* accum_before, const float* accum_after, const float* motion, const struct frayhip_change* p,
                         float* change, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_change_frame";
    if (const int rc = check(who, width, height, accum_before, accum_after, motion, p, change, false)) return rc;
    const size_t n = (size_t)width * height;
    const size_t AC = FRAYHIP_ACCUM_CHANNELS, MC = FRAYHIP_MOTION_CHANNELS;
    // one allocation, the 16-byte rows first: both states, motion when given, then change
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_before;
    if (const int rc = B.alloc(d_before, n * (2 * AC + (motion ? MC : 0) + 1))) return rc;
    float* d_after = d_before + AC * n;
    float* d_motion = motion ? d_after + AC * n : nullptr;
    float* d_change = d_after + AC * n + (motion ? MC * n : 0);
    HIP_TRY(hipMemcpy(d_before, accum_before, n * 4 * AC, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_after, accum_after, n * 4 * AC, hipMemcpyHostToDevice));
    if (d_motion) HIP_TRY(hipMemcpy(d_motion, motion, n * 4 * MC, hipMemcpyHostToDevice));
    if (const int rc = run(width, height, d_before, d_after, d_motion, p, d_change, nullptr, st, t0)) return rc;
    HIP_TRY(hipMemcpy(change, d_change, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

}  // extern "C"
