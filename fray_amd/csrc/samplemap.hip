// C ABI, sample maps from a state (include/frayhip.h "sample maps"): frayhip_sample_map_defaults, frayhip_sample_map and its _device entry, and
// frayhip_sample_map_pair / _pair_device for a pair of component states (the two components' mean luminances and noise estimates added).  A
// resumable state and its per-pixel sample counts go in; out comes the `add` plane of frayhip_render_samples_map: how many more samples each pixel
// needs before the standard error of its mean's luminance is `tolerance` times that luminance.  Scene-free, FP32 throughout; the Makefile builds
// this object as it builds denoise.o (-ffp-contract=off, correctly rounded divide), so every product below is rounded where it is written
// (tests/sample_map_ref.py restates it in numpy, and the two agree bit for bit).
//
//   k_sample_map<PAIR>   per pixel: k_acc_mean's mean and noise at the pixel's own N (PAIR: of both states, added), the count at which that noise
//                        would meet the tolerance, the caps (the formula itself: samplemap_formula.hpp, shared with samplemap_budget.hip)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <string>

#include "entry_support.hpp"
#include "samplemap_formula.hpp"
#include "temporal_common.hpp"

struct SampleMapArgs {
    size_t n;
    const float4* accum;        // one row a pixel: {sum.rgb, m2}
    const float4* accum2;       // the indirect state of a pair (accum is then the direct one); null otherwise
    const int32_t* count;
    int32_t* add;
    float tolerance, lumFloor;
    int minCount, maxCount, maxAdd, grow;
    unsigned long long* totals; // [0] pixels with add > 0, [1] the sum of add
};

template <bool PAIR>
static __global__ __launch_bounds__(256) void k_sample_map(SampleMapArgs A)
{
    __shared__ unsigned long long sPix, sSum;
    if (threadIdx.x == 0) { sPix = 0; sSum = 0; }
    __syncthreads();
    unsigned long long tPix = 0, tSum = 0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < A.n; p += (size_t)gridDim.x * blockDim.x) {
        const int N = A.count[p];
        int add = 0;
        if (N < A.maxCount) {
            float noise = 0.0f, ref = 0.0f;
            if (N >= A.minCount) sm_reduce<PAIR>(A.accum, A.accum2, p, N, A.lumFloor, noise, ref);
            add = sm_add(N, noise, ref, A.tolerance, A.minCount, A.maxCount, A.maxAdd, A.grow);
        }
        A.add[p] = add;
        if (add > 0) { tPix++; tSum += (unsigned long long)add; }
    }
    if (tPix) { atomicAdd(&sPix, tPix); atomicAdd(&sSum, tSum); }
    __syncthreads();
    if (threadIdx.x == 0 && sPix) { atomicAdd(&A.totals[0], sPix); atomicAdd(&A.totals[1], sSum); }
}

namespace {

using namespace frayhip_detail;
using namespace frayhip_temporal_detail;
using frayhip_samplemap_detail::check;
using frayhip_samplemap_detail::kMaxCount;

// The device path of both entries (device pointers, checked).  A negative count is read as a pixel below min_count.
int run(int W, int H, const float* accum, const float* accum2, const int32_t* count, struct frayhip_sample_map* p, int32_t* add, hipStream_t stream, frayhip_stats* st,
        std::chrono::steady_clock::time_point t0)
{
    struct Totals {
        unsigned long long* d = nullptr;
        ~Totals() { if (d) (void)hipFree(d); }
    } totals;
    HIP_TRY(hipMalloc((void**)&totals.d, 16));
    SampleMapArgs A{};
    A.n = (size_t)W * H;
    A.accum = (const float4*)accum; A.accum2 = (const float4*)accum2; A.count = count; A.add = add;
    A.tolerance = p->tolerance; A.lumFloor = p->lum_floor;
    A.minCount = p->min_count; A.maxCount = p->max_count; A.maxAdd = p->max_add; A.grow = p->grow;
    A.totals = totals.d;
    Events E;
    HIP_TRY(hipEventCreate(&E.a));
    HIP_TRY(hipEventCreate(&E.b));
    struct Drain { hipStream_t s; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(s); } } drain{stream};
    HIP_TRY(hipMemsetAsync(totals.d, 0, 16, stream));
    HIP_TRY(hipEventRecord(E.a, stream));
    if (accum2) hipLaunchKernelGGL(k_sample_map<true>, dim3(grid_for(A.n)), dim3(256), 0, stream, A);
    else hipLaunchKernelGGL(k_sample_map<false>, dim3(grid_for(A.n)), dim3(256), 0, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(E.b, stream));
    unsigned long long h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h, totals.d, 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    p->pixels = h[0];
    p->samples = h[1];
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

int frayhip_sample_map_defaults(struct frayhip_sample_map* p)
{
    if (!p) return bad("frayhip_sample_map_defaults", "null parameters");
    p->tolerance = 0.05f;
    p->lum_floor = 0.01f;
    p->min_count = 4;
    p->max_count = 0;               // none: the caller sets it
    p->max_add = kMaxCount;         // no cap of its own
    p->grow = 2;
    p->pixels = 0;
    p->samples = 0;
    return FRAYHIP_OK;
}

int frayhip_sample_map_device(int width, int height, const float* d_accum, const int32_t* d_count, struct frayhip_sample_map* p, int32_t* d_add, void* hip_stream,
                              frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = check("frayhip_sample_map_device", width, height, d_accum, nullptr, false, d_count, p, d_add, true)) return rc;
    return run(width, height, d_accum, nullptr, d_count, p, d_add, (hipStream_t)hip_stream, st, t0);
}

int frayhip_sample_map(int width, int height, const float* accum, const int32_t* count, struct frayhip_sample_map* p, int32_t* add, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_sample_map";
    if (const int rc = check(who, width, height, accum, nullptr, false, count, p, add, false)) return rc;
    const size_t n = (size_t)width * height;
    // one allocation, the 16-byte rows first: the state, the counts, then add
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_accum;
    if (const int rc = B.alloc(d_accum, n * 6)) return rc;
    int32_t* d_count = (int32_t*)(d_accum + 4 * n);
    int32_t* d_add = d_count + n;
    HIP_TRY(hipMemcpy(d_accum, accum, n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, count, n * 4, hipMemcpyHostToDevice));
    if (const int rc = run(width, height, d_accum, nullptr, d_count, p, d_add, nullptr, st, t0)) return rc;
    HIP_TRY(hipMemcpy(add, d_add, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

int frayhip_sample_map_pair_device(int width, int height, const float* d_accum_direct, const float* d_accum_indirect, const int32_t* d_count,
                                   struct frayhip_sample_map* p, int32_t* d_add, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = check("frayhip_sample_map_pair_device", width, height, d_accum_direct, d_accum_indirect, true, d_count, p, d_add, true)) return rc;
    return run(width, height, d_accum_direct, d_accum_indirect, d_count, p, d_add, (hipStream_t)hip_stream, st, t0);
}

int frayhip_sample_map_pair(int width, int height, const float* accum_direct, const float* accum_indirect, const int32_t* count, struct frayhip_sample_map* p,
                            int32_t* add, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_sample_map_pair";
    if (const int rc = check(who, width, height, accum_direct, accum_indirect, true, count, p, add, false)) return rc;
    const size_t n = (size_t)width * height;
    // one allocation, the 16-byte rows first: the two states, the counts, then add
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_direct;
    if (const int rc = B.alloc(d_direct, n * 10)) return rc;
    float* d_indirect = d_direct + 4 * n;
    int32_t* d_count = (int32_t*)(d_indirect + 4 * n);
    int32_t* d_add = d_count + n;
    HIP_TRY(hipMemcpy(d_direct, accum_direct, n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_indirect, accum_indirect, n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, count, n * 4, hipMemcpyHostToDevice));
    if (const int rc = run(width, height, d_direct, d_indirect, d_count, p, d_add, nullptr, st, t0)) return rc;
    HIP_TRY(hipMemcpy(add, d_add, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

}  // extern "C"
