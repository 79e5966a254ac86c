// The per-pixel formula of the sample maps (include/frayhip.h "sample maps") and the argument checks of their entries, shared by k_sample_map
// (samplemap.hip) and the budgeted map's kernels (samplemap_budget.hip).  FP32 without contraction: both objects are built as denoise.o is, so
// every product is rounded where it is written (tests/sample_map_ref.py restates it in numpy).
//
// The formula in two halves.  sm_reduce takes a pixel's row (two rows for a pair) to the two numbers the tolerance meets, noise and ref;
// sm_add takes them, the pixel's N and a tolerance to the pixel's add.  MONOTONE IN THE TOLERANCE: for a fixed pixel sm_add does not increase
// when the tolerance does.  t = tolerance * ref with ref > 0 (fmaxf with a positive floor), t * t, noise / (t * t) for a noise >= 0,
// fn * (...) and ceilf are each one correctly rounded operation, and a correctly rounded operation is monotone in each operand; the conversions,
// max(N, .), min(., grow * N), min(., max_count) - N and min(., max_add) are non-decreasing in need.  The rows where that chain is not of
// finite numbers are constant or drop once: a NaN noise or an infinite one gives a need that is NaN or +inf at every tolerance (max_count
// asked for throughout; inf / inf is NaN, which asks for the same); a t * t that underflows to 0 gives need = +inf or NaN (max_count) up to the
// tolerance at which t * t is positive, a finite need from there on; a t * t that overflows gives need 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "entry_support.hpp"
#include "temporal_common.hpp"

// k_acc_mean's mean luminance and noise of one row at N samples
__host__ __device__ __forceinline__ void sm_row(const float4 row, int N, float fn, float& lbar, float& noise)
{
    const float mr = row.x / fn, mg = row.y / fn, mb = row.z / fn;
    lbar = ((mr + mg) + mb) / 3.0f;             // tp_lum
    const float v = fmaxf(0.0f, row.w / fn - lbar * lbar);
    noise = N >= 2 ? v / (float)(N - 1) : lbar * lbar;
}

// noise and ref of pixel p, min_count <= N < max_count
template <bool PAIR>
__host__ __device__ __forceinline__ void sm_reduce(const float4* accum, const float4* accum2, size_t p, int N, float lumFloor, float& noise, float& ref)
{
    const float fn = (float)N;
    float lbar;
    sm_row(accum[p], N, fn, lbar, noise);
    if (PAIR) {          // the components are separate signals to the split filter, and their errors add in the final sum
        float lbarI, noiseI;
        sm_row(accum2[p], N, fn, lbarI, noiseI);
        lbar = lbar + lbarI;
        noise = noise + noiseI;
    }
    ref = fmaxf(lbar, lumFloor);
}

// add of a pixel that holds N samples (noise and ref are read only for min_count <= N < max_count)
__host__ __device__ __forceinline__ int sm_add(int N, float noise, float ref, float tolerance, int minCount, int maxCount, int maxAdd, int grow)
{
    if (N >= maxCount) return 0;
    int target;
    if (N < minCount) target = minCount;
    else {
        const float fn = (float)N;
        const float t = tolerance * ref;
        const float need = ceilf(fn * (noise / (t * t)));
        target = need <= (float)maxCount ? (N > (int)need ? N : (int)need) : maxCount;     // a NaN need asks for max_count: never stops a pixel early
        const int most = grow * N;
        target = target < most ? target : most;
    }
    const int add = (target < maxCount ? target : maxCount) - N;
    return add < maxAdd ? add : maxAdd;
}

namespace frayhip_samplemap_detail {

using frayhip_detail::bad;
using frayhip_detail::misaligned;
using frayhip_temporal_detail::overlaps;

constexpr int kMaxCount = 1 << 24;

// Every check of the map entries, in this order; none touches the device
// (pair: accum is the direct state and accum2 the indirect one)
inline int check(const char* who, int W, int H, const float* accum, const float* accum2, bool pair, const int32_t* count, const struct frayhip_sample_map* p,
                 const int32_t* add, bool device)
{
    if (W < 1 || H < 1) return bad(who, "width and height must be >= 1");
    if ((long long)W * H > (1ll << 30)) return bad(who, "more than 2^30 pixels");
    if (!accum) return bad(who, pair ? "null accum_direct" : "null accum");
    if (pair && !accum2) return bad(who, "null accum_indirect");
    if (!count) return bad(who, "null count");
    if (!p) return bad(who, "null parameters");
    if (!add) return bad(who, "null add");
    if (!std::isfinite(p->tolerance) || !(p->tolerance > 0)) return bad(who, "tolerance must be finite and > 0");
    if (!std::isfinite(p->lum_floor) || !(p->lum_floor > 0)) return bad(who, "lum_floor must be finite and > 0");
    if (p->min_count < 1) return bad(who, "min_count must be >= 1");
    if (p->max_count < p->min_count) return bad(who, "max_count must be >= min_count");
    if (p->max_count > kMaxCount) return bad(who, "max_count must be <= 2^24");
    if (p->max_add < 1) return bad(who, "max_add must be >= 1");
    if (p->grow < 2 || p->grow > 16) return bad(who, "grow must be 2..16");
    if (device) {
        if (misaligned(accum, 16) || (pair && misaligned(accum2, 16))) return bad(who, "device pointer to the state not 16-byte aligned");
        if (misaligned(count, 4) || misaligned(add, 4)) return bad(who, "device pointer to a plane not 4-byte aligned");
    }
    const size_t n = (size_t)W * H;
    if (overlaps(add, 4 * n, accum, 16 * n) || overlaps(add, 4 * n, count, 4 * n)) return bad(who, "add must not overlap an input");
    if (pair) {
        if (overlaps(add, 4 * n, accum2, 16 * n)) return bad(who, "add must not overlap an input");
        if (overlaps(accum2, 16 * n, accum, 16 * n)) return bad(who, "accum_indirect must not overlap accum_direct");
        if (overlaps(count, 4 * n, accum, 16 * n)) return bad(who, "count must not overlap accum_direct");
        if (overlaps(count, 4 * n, accum2, 16 * n)) return bad(who, "count must not overlap accum_indirect");
        return FRAYHIP_OK;
    }
    if (overlaps(count, 4 * n, accum, 16 * n)) return bad(who, "count must not overlap accum");
    return FRAYHIP_OK;
}

}  // namespace frayhip_samplemap_detail
