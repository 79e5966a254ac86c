// C ABI, history maps (include/frayhip.h "history maps"): frayhip_history_map_defaults, frayhip_history_map and its _device entry.  Given the
// history that frayhip_temporal_accumulate_weighted will fetch for this view, how many samples each pixel gets this frame: a pixel whose
// reprojected history already amounts to `target` units gets `base` samples, one that holds less gets the missing whole units on top, at most
// max_units of them, and the target is lowered until the plane fits a frame-wide budget.  Scene-free; the Makefile builds this object as it
// builds temporal.o (-ffp-contract=off, correctly rounded divide and sqrt), and steps 1 and 2 are temporal_common.hpp's tp_surface and tp_fetch,
// the very functions k_tp_accumulate runs, so `held` is that kernel's hu bit for bit.  tests/history_map_ref.py restates the definition.
//
// A call is three launches on the caller's stream, ordered by the stream alone, and one synchronisation, whatever the data:
//   k_hm_held<MOTION, AGGREGATE>  per pixel: the fetch, held (into the call's workspace, and the caller's plane when given), k = floor(min(held,
//                       max_history)) counted into a histogram of max_history + 1 bins.  A block counts in LDS, one atomic a pixel, and flushes
//                       its non-zero bins with integer atomics; <.., true> first lets each wave's first active lane count every lane that holds
//                       the same k with one LDS atomic (one round: the lanes that differ add their own).  Integer sums: the bins depend on
//                       neither grid nor timing.
//   k_hm_select         one block: C(j), the pixels with k <= j, from the bins; S(1) = base * W*H, S(t + 1) = S(t) + base * (C(t - 1) - C(t - max_units))
//                       (the pixels whose units grow by one from t to t + 1 are those with t - max_units < k < t); the largest t <= target with
//                       S(t) <= budget, S(t) and the pixels with more than one unit, C(t - 2), go to the control record
//   k_hm_map            per pixel: units = min(max(t - k, 1), max_units) with the record's t; add = base * units, weight = (float)units
// The entries launch k_hm_held<.., false>: at 1080p the two kernels measured the same within what the order of two calls changes (about
// 4 %), for a settled history (seven pixels in eight in one bin) as for a random one, so the simpler one runs -- 64 LDS atomics to one address
// cost no more than the ballots and the shuffle that would spare them (profiles/history_map/README.md).  FRAYHIP_HISTORY_MAP_AGGREGATE=1
// in the environment selects <.., true>, which is kept so that tools/history_map_rate.py can time the two side by side; the planes and
// the record are the same either way.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "entry_support.hpp"
#include "temporal_common.hpp"

namespace {

// The control record, in 64-bit words; the bins (32-bit: W*H <= 2^30) follow it
enum : int { kTargetUsed = 0, kSamples = 1, kBoosted = 2, kRecordWords = 4 };

struct HistoryMapCall {
    int W, H;
    size_t n;
    const float* feat;
    const float4* motion;       // null: the pixel's own position and normal
    const float* change;        // null: no change frame
    const float4* histIn;       // null: first frame
    const float* unitsIn;
    frayhip_view view;          // read only with histIn
    float maxHistory, filmOffset, planeTolerance, normalMinDot;
    int bins;                   // max_history + 1
    int base, target, maxUnits;
    unsigned long long budget;
    float* heldWs;              // the call's workspace: held per pixel
    float* held;                // the caller's plane, or null
    unsigned long long* record;
    unsigned int* hist;
    int32_t* add;
    float* weight;
};

__device__ __forceinline__ int hm_k(float held, float maxHistory) { return (int)floorf(fminf(held, maxHistory)); }

template <bool MOTION, bool AGGREGATE>
static __global__ __launch_bounds__(256) void k_hm_held(HistoryMapCall A)
{
    extern __shared__ unsigned int sBins[];
    for (int b = (int)threadIdx.x; b < A.bins; b += 256) sBins[b] = 0u;
    __syncthreads();
    const int lane = (int)threadIdx.x & 63;
    // the loop's bounds are the block's, so every wave runs the ballots below together
    for (size_t first = (size_t)blockIdx.x * 256; first < A.n; first += (size_t)gridDim.x * 256) {
        const size_t p = first + threadIdx.x;
        const bool valid = p < A.n;
        int k = 0;
        if (valid) {
            float held = 0.0f;
            if (A.histIn) {
                const TpSurface S = tp_surface<MOTION>(A.feat + p * FRAYHIP_FEAT_CHANNELS, A.motion, p);
                const TpFetch h = tp_fetch<true>(S, A.W, A.H, A.histIn, A.unitsIn, A.view, A.filmOffset, A.planeTolerance, A.normalMinDot);
                if (h.sb > 0.0f) {
                    const float hu = h.hu / h.sb;
                    held = hu;
                    if (A.change) {
                        const float g = A.change[p];
                        if (!(g < 1.0f)) held = 0.0f;
                        else if (g > 0.0f) held = hu * (1.0f - g);
                    }
                }
            }
            if (!(held >= 0.0f)) held = 0.0f;
            A.heldWs[p] = held;
            if (A.held) A.held[p] = held;
            k = hm_k(held, A.maxHistory);
        }
        if constexpr (AGGREGATE) {
            const unsigned long long active = __ballot(valid);
            if (active) {
                const int leader = __ffsll((long long)active) - 1;
                const int kl = __shfl(k, leader, 64);
                const unsigned long long same = __ballot(valid && k == kl);
                if (lane == leader) atomicAdd(&sBins[kl], (unsigned int)__popcll(same));
                else if (valid && k != kl) atomicAdd(&sBins[k], 1u);
            }
        } else {
            if (valid) atomicAdd(&sBins[k], 1u);
        }
    }
    __syncthreads();
    for (int b = (int)threadIdx.x; b < A.bins; b += 256) {
        const unsigned int c = sBins[b];
        if (c) atomicAdd(&A.hist[b], c);
    }
}

#define FRAY_HM_MAX_BINS 4097           // max_history <= 4096 (check_params)

static __global__ __launch_bounds__(256) void k_hm_select(HistoryMapCall A)
{
    __shared__ unsigned int sC[FRAY_HM_MAX_BINS];       // C(j): the pixels with k <= j
    for (int b = (int)threadIdx.x; b < A.bins; b += 256) sC[b] = A.hist[b];
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned int run = 0u;
    for (int b = 0; b < A.bins; b++) { run += sC[b]; sC[b] = run; }
    const int last = A.bins - 1;
    auto C = [&](int j) -> unsigned long long { return j < 0 ? 0ull : (unsigned long long)sC[j < last ? j : last]; };
    const unsigned long long base = (unsigned long long)A.base;
    unsigned long long S = base * (unsigned long long)A.n;          // S(1): one unit everywhere; <= budget by the entry's check
    int t = 1;
    while (t < A.target) {
        const unsigned long long next = S + base * (C(t - 1) - C(t - A.maxUnits));
        if (next > A.budget) break;
        S = next;
        t++;
    }
    A.record[kTargetUsed] = (unsigned long long)t;
    A.record[kSamples] = S;
    A.record[kBoosted] = A.maxUnits >= 2 ? C(t - 2) : 0ull;
}

static __global__ __launch_bounds__(256) void k_hm_map(HistoryMapCall A)
{
    const int t = (int)A.record[kTargetUsed];
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < A.n; p += (size_t)gridDim.x * blockDim.x) {
        const int k = hm_k(A.heldWs[p], A.maxHistory);
        const int units = min(max(t - k, 1), A.maxUnits);
        A.add[p] = A.base * units;
        A.weight[p] = (float)units;
    }
}

using namespace frayhip_detail;
using namespace frayhip_temporal_detail;

// Every check of the two entries, in this order; none touches the device
int check(const char* who, int W, int H, const float* feat, const float* motion, const float* change, const frayhip_view* view, const float* histIn,
          const float* unitsIn, const struct frayhip_temporal* p, const struct frayhip_history_map* m, const int32_t* add, const float* weight, const float* held,
          bool device)
{
    if (W < 1 || H < 1) return bad(who, "width and height must be >= 1");
    if ((long long)W * H > (1ll << 30)) return bad(who, "more than 2^30 pixels");
    if (!feat) return bad(who, "null feat");
    if (!p) return bad(who, "null parameters");
    if (!m) return bad(who, "null map");
    if (!add) return bad(who, "null add");
    if (!weight) return bad(who, "null weight");
    if (!histIn != !view || !histIn != !unitsIn) return bad(who, "hist_in, units_in and prev_view must all be given or all be null");
    if (device) {
        for (const void* q : {(const void*)feat, (const void*)change, (const void*)unitsIn, (const void*)add, (const void*)weight, (const void*)held})
            if (misaligned(q, 4)) return bad(who, "device pointer not 4-byte aligned");
        if (misaligned(histIn, 16)) return bad(who, "device pointer to a history not 16-byte aligned");
        if (misaligned(motion, 16)) return bad(who, "device pointer to a motion frame not 16-byte aligned");
    }
    if (const int rc = check_view(who, W, H, view)) return rc;
    if (const int rc = check_params(who, p)) return rc;
    if (m->base < 1) return bad(who, "base must be >= 1");
    if (m->target < 1 || m->target > p->max_history) return bad(who, "target must be 1..max_history");
    if (m->max_units < 1) return bad(who, "max_units must be >= 1");
    if ((long long)m->base * m->max_units > (1ll << 24)) return bad(who, "base * max_units must be <= 2^24");
    if (m->reserved != 0) return bad(who, "reserved must be 0");
    const size_t n = (size_t)W * H;
    if (m->budget < (uint64_t)m->base * n) return bad(who, "budget is below base * width * height: one unit a pixel is the least a map hands out");
    const struct { const void* q; size_t bytes; } ins[5] = {{feat, 4 * FRAYHIP_FEAT_CHANNELS * n}, {motion, 4 * FRAYHIP_MOTION_CHANNELS * n}, {change, 4 * n},
                                                            {histIn, 4 * FRAYHIP_HISTORY_CHANNELS * n}, {unitsIn, 4 * n}};
    const struct { const void* q; size_t bytes; const char* name; } outs[3] = {{add, 4 * n, "add"}, {weight, 4 * n, "weight"}, {held, 4 * n, "held"}};
    for (int o = 0; o < 3; o++) {
        for (const auto& in : ins)
            if (overlaps(outs[o].q, outs[o].bytes, in.q, in.bytes)) return bad(who, std::string(outs[o].name) + " must not overlap an input");
        for (int k = 0; k < o; k++)
            if (overlaps(outs[o].q, outs[o].bytes, outs[k].q, outs[k].bytes)) return bad(who, std::string(outs[o].name) + " must not overlap " + outs[k].name);
    }
    return FRAYHIP_OK;
}

// The device path of both entries (device pointers, checked)
int run(const char* who, int W, int H, const float* feat, const float* motion, const float* change, const frayhip_view* view, const float* histIn,
        const float* unitsIn, const struct frayhip_temporal* prm, struct frayhip_history_map* m, int32_t* add, float* weight, float* held, hipStream_t stream,
        frayhip_stats* st, std::chrono::steady_clock::time_point t0)
{
    const size_t n = (size_t)W * H;
    HistoryMapCall A{};
    A.W = W; A.H = H; A.n = n;
    A.feat = feat; A.motion = (const float4*)motion; A.change = change;
    A.histIn = (const float4*)histIn; A.unitsIn = unitsIn;
    if (view) A.view = *view;
    A.maxHistory = (float)prm->max_history; A.filmOffset = prm->film_offset;
    A.planeTolerance = prm->plane_tolerance; A.normalMinDot = prm->normal_min_dot;
    A.bins = prm->max_history + 1;
    A.base = m->base; A.target = m->target; A.maxUnits = m->max_units; A.budget = m->budget;
    A.held = held; A.add = add; A.weight = weight;
    // the call's workspace: the record and the bins, then held
    DeviceArrays B(std::string(who) + ": out of device memory");
    unsigned char* ws;
    const size_t headBytes = kRecordWords * 8 + (size_t)A.bins * 4, head = r256(headBytes);
    if (const int rc = B.alloc(ws, head + n * sizeof(float))) return rc;
    A.record = (unsigned long long*)ws;
    A.hist = (unsigned int*)(ws + kRecordWords * 8);
    A.heldWs = (float*)(ws + head);
    const char* agg = std::getenv("FRAYHIP_HISTORY_MAP_AGGREGATE");
    const bool aggregate = agg && agg[0] == '1';
    Events E;
    HIP_TRY(hipEventCreate(&E.a));
    HIP_TRY(hipEventCreate(&E.b));
    struct Drain { hipStream_t s; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(s); } } drain{stream};
    const dim3 grid(grid_for(n)), block(256);
    const size_t lds = (size_t)A.bins * 4;
    HIP_TRY(hipMemsetAsync(ws, 0, headBytes, stream));
    HIP_TRY(hipEventRecord(E.a, stream));
    if (motion && aggregate) hipLaunchKernelGGL((k_hm_held<true, true>), grid, block, lds, stream, A);
    else if (motion) hipLaunchKernelGGL((k_hm_held<true, false>), grid, block, lds, stream, A);
    else if (aggregate) hipLaunchKernelGGL((k_hm_held<false, true>), grid, block, lds, stream, A);
    else hipLaunchKernelGGL((k_hm_held<false, false>), grid, block, lds, stream, A);
    hipLaunchKernelGGL(k_hm_select, dim3(1), block, 0, stream, A);
    hipLaunchKernelGGL(k_hm_map, grid, block, 0, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(E.b, stream));
    unsigned long long h[kRecordWords] = {};
    HIP_TRY(hipMemcpyAsync(h, A.record, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    m->target_used = (int32_t)h[kTargetUsed];
    m->samples = h[kSamples];
    m->boosted = h[kBoosted];
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

int frayhip_history_map_defaults(struct frayhip_history_map* m)
{
    if (!m) return bad("frayhip_history_map_defaults", "null map");
    struct frayhip_history_map zero = {};
    *m = zero;
    m->target = 8;
    m->max_units = 8;
    m->budget = UINT64_MAX;
    return FRAYHIP_OK;
}

int frayhip_history_map_device(int width, int height, const float* d_feat, const float* d_motion, const float* d_change, const frayhip_view* prev_view,
                               const float* d_hist_in, const float* d_units_in, const struct frayhip_temporal* p, struct frayhip_history_map* m, int32_t* d_add,
                               float* d_weight, float* d_held, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_history_map_device";
    if (const int rc = check(who, width, height, d_feat, d_motion, d_change, prev_view, d_hist_in, d_units_in, p, m, d_add, d_weight, d_held, true)) return rc;
    return run(who, width, height, d_feat, d_motion, d_change, prev_view, d_hist_in, d_units_in, p, m, d_add, d_weight, d_held, (hipStream_t)hip_stream, st, t0);
}

int frayhip_history_map(int width, int height, const float* feat, const float* motion, const float* change, const frayhip_view* prev_view, const float* hist_in,
                        const float* units_in, const struct frayhip_temporal* p, struct frayhip_history_map* m, int32_t* add, float* weight, float* held,
                        frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_history_map";
    if (const int rc = check(who, width, height, feat, motion, change, prev_view, hist_in, units_in, p, m, add, weight, held, false)) return rc;
    const size_t n = (size_t)width * height;
    const size_t HC = FRAYHIP_HISTORY_CHANNELS, MC = FRAYHIP_MOTION_CHANNELS;
    // one allocation, the 16-byte rows first: hist_in and motion when given, then feat, add, weight, held, and change and units_in when given
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_all;
    if (const int rc = B.alloc(d_all, n * ((hist_in ? HC + 1 : 0) + (motion ? MC : 0) + FRAYHIP_FEAT_CHANNELS + 3 + (change ? 1 : 0)))) return rc;
    float* q = d_all;
    float* d_hin = nullptr;
    float* d_motion = nullptr;
    float* d_change = nullptr;
    float* d_uin = nullptr;
    if (hist_in) { d_hin = q; q += HC * n; }
    if (motion) { d_motion = q; q += MC * n; }
    float* d_feat = q;
    int32_t* d_add = (int32_t*)(d_feat + FRAYHIP_FEAT_CHANNELS * n);
    float* d_weight = (float*)(d_add + n);
    float* d_held = d_weight + n;
    q = d_held + n;
    if (change) { d_change = q; q += n; }
    if (hist_in) { d_uin = q; q += n; }
    HIP_TRY(hipMemcpy(d_feat, feat, n * 4 * FRAYHIP_FEAT_CHANNELS, hipMemcpyHostToDevice));
    if (d_change) HIP_TRY(hipMemcpy(d_change, change, n * 4, hipMemcpyHostToDevice));
    if (d_motion) HIP_TRY(hipMemcpy(d_motion, motion, n * 4 * MC, hipMemcpyHostToDevice));
    if (d_hin) HIP_TRY(hipMemcpy(d_hin, hist_in, n * 4 * HC, hipMemcpyHostToDevice));
    if (d_uin) HIP_TRY(hipMemcpy(d_uin, units_in, n * 4, hipMemcpyHostToDevice));
    if (const int rc = run(who, width, height, d_feat, d_motion, d_change, prev_view, d_hin, d_uin, p, m, d_add, d_weight, held ? d_held : nullptr, nullptr, st, t0))
        return rc;
    HIP_TRY(hipMemcpy(add, d_add, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(weight, d_weight, n * 4, hipMemcpyDeviceToHost));
    if (held) HIP_TRY(hipMemcpy(held, d_held, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

}  // extern "C"
