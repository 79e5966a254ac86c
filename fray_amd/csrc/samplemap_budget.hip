// C ABI, budgeted sample maps (include/frayhip.h "sample maps"): frayhip_sample_map_budget and its _device entry.  The map of frayhip_sample_map
// (or of frayhip_sample_map_pair, with a second state) made to fit a frame-wide sample budget: the tolerance is raised until the frame can afford
// it (stage 1), and where no tolerance is enough a per-pixel cap is lowered (stage 2).  Scene-free, FP32 throughout; the Makefile builds this
// object as it builds samplemap.o, and the per-pixel formula is the one header both share (samplemap_formula.hpp), so stage 0's plane is
// k_sample_map's bit for bit.  tests/sample_map_budget_ref.py restates the definition with a two-way bisection.
//
// A call is a fixed sequence of launches on the caller's stream, ordered by the stream alone (no host round trip, no grid-wide barrier):
//   k_budget_prepare<PAIR>  per pixel: the row(s) reduced once to the record {noise, ref} in the call's workspace (N stays in the caller's count
//                           plane, which no kernel writes); S(tolerance) and S(FLT_MAX) summed into the control block
//   k_budget_search x 8     launch k re-derives its interval from the control block (budget_search.hpp: the stage from the two sums, then the
//                           narrowing of launches 0 .. k-1 replayed from their totals, by one thread of every block), evaluates 16 candidates
//                           of the searched parameter per pixel while the record is read once, and adds 16 totals to its own row of the
//                           control block.  Stage 0, or an interval already closed: it returns after reading the control block.
//   k_budget_final          replays all eight, writes add at the tolerance and cap found, sums pixels and samples, records the outcome
// The control block is zeroed once per call.  Every total is an exact integer sum (64-bit per thread, wave shuffles, LDS across the block's four
// waves, one 64-bit atomic per block and candidate), so it depends on neither the grid nor the order of arrival.  Why eight launches close any
// interval: budget_search.hpp.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "budget_search.hpp"
#include "entry_support.hpp"
#include "samplemap_formula.hpp"
#include "temporal_common.hpp"

namespace {

using fray_budget::kCandidates;
using fray_budget::kLaunches;

// The control block, in 64-bit words
enum : int {
    kDemand = 0,        // S(tolerance)
    kRest = 1,          // S(FLT_MAX)
    kPixels = 2,        // the final plane's pixels with add > 0
    kSamples = 3,       // and the sum of its add
    kStage = 4,
    kTolBits = 5,
    kCap = 6,           // as int64; -1: none
    kHead = 8,          // what the host reads back
    kSums = 8,          // kLaunches rows of kCandidates totals
    kWords = kSums + kLaunches * kCandidates,
};

struct BudgetArgs {
    size_t n;
    const float4* accum;        // one row a pixel: {sum.rgb, m2}
    const float4* accum2;       // the indirect state of a pair; null otherwise
    const int32_t* count;
    int32_t* add;
    float2* rec;                // per pixel {noise, ref}, meaningful for min_count <= N < max_count
    unsigned long long* ctl;
    unsigned long long budget;
    float tolerance, lumFloor;
    int minCount, maxCount, maxAdd, grow;
};

// The sum of v[j] over the block's 256 threads (four waves of 64), added to dst[j]; M <= 256
template <int M>
__device__ __forceinline__ void block_sum(unsigned long long (&v)[M], unsigned long long* dst)
{
    __shared__ unsigned long long sPart[4][M];
#pragma unroll
    for (int j = 0; j < M; j++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[j] += __shfl_down(v[j], off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < M; j++) sPart[wave][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < M) {
        const unsigned long long s = (sPart[0][threadIdx.x] + sPart[1][threadIdx.x]) + (sPart[2][threadIdx.x] + sPart[3][threadIdx.x]);
        if (s) atomicAdd(&dst[threadIdx.x], s);
    }
}

__device__ __forceinline__ fray_budget::Search search_state(const BudgetArgs& A, int launches)
{
    const fray_budget::Search s = fray_budget::start(A.ctl[kDemand], A.ctl[kRest], A.budget, __float_as_uint(A.tolerance), (uint32_t)A.maxAdd);
    return fray_budget::replay(s, (const uint64_t*)(A.ctl + kSums), launches, A.budget);
}

template <bool PAIR>
static __global__ __launch_bounds__(256) void k_budget_prepare(BudgetArgs A)
{
    unsigned long long t[2] = {0, 0};
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < A.n; p += (size_t)gridDim.x * blockDim.x) {
        const int N = A.count[p];
        float noise = 0.0f, ref = 0.0f;
        if (N >= A.minCount && N < A.maxCount) sm_reduce<PAIR>(A.accum, A.accum2, p, N, A.lumFloor, noise, ref);
        A.rec[p] = make_float2(noise, ref);
        t[0] += (unsigned long long)sm_add(N, noise, ref, A.tolerance, A.minCount, A.maxCount, A.maxAdd, A.grow);
        t[1] += (unsigned long long)sm_add(N, noise, ref, FLT_MAX, A.minCount, A.maxCount, A.maxAdd, A.grow);
    }
    block_sum<2>(t, A.ctl + kDemand);
}

static __global__ __launch_bounds__(256) void k_budget_search(BudgetArgs A, int launch)
{
    __shared__ uint32_t sCand[kCandidates];
    __shared__ int sStage;              // 0: nothing to search (stage 0, or the interval is closed)
    if (threadIdx.x == 0) {
        const fray_budget::Search s = search_state(A, launch);
        sStage = fray_budget::open(s) ? s.stage : 0;
        for (int j = 0; j < kCandidates; j++) sCand[j] = fray_budget::candidate(s, j);
    }
    __syncthreads();
    const int stage = sStage;
    if (stage == 0) return;
    uint32_t cand[kCandidates];
#pragma unroll
    for (int j = 0; j < kCandidates; j++) cand[j] = sCand[j];
    unsigned long long t[kCandidates];
#pragma unroll
    for (int j = 0; j < kCandidates; j++) t[j] = 0;
    if (stage == 1) {
        for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < A.n; p += (size_t)gridDim.x * blockDim.x) {
            const int N = A.count[p];
            if (N >= A.maxCount) continue;
            const float2 r = A.rec[p];
#pragma unroll
            for (int j = 0; j < kCandidates; j++)
                t[j] += (unsigned long long)sm_add(N, r.x, r.y, __uint_as_float(cand[j]), A.minCount, A.maxCount, A.maxAdd, A.grow);
        }
    } else {
        for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < A.n; p += (size_t)gridDim.x * blockDim.x) {
            const int N = A.count[p];
            if (N >= A.maxCount) continue;
            const float2 r = A.rec[p];
            const int rest = sm_add(N, r.x, r.y, FLT_MAX, A.minCount, A.maxCount, A.maxAdd, A.grow);
#pragma unroll
            for (int j = 0; j < kCandidates; j++) t[j] += (unsigned long long)min(rest, (int)cand[j]);
        }
    }
    block_sum<kCandidates>(t, A.ctl + kSums + launch * kCandidates);
}

static __global__ __launch_bounds__(256) void k_budget_final(BudgetArgs A)
{
    __shared__ uint32_t sTol;
    __shared__ int sCap;
    if (threadIdx.x == 0) {
        const fray_budget::Search s = search_state(A, kLaunches);
        const int32_t cap = fray_budget::cap_of(s);
        sTol = fray_budget::tolerance_bits(s);
        sCap = cap < 0 ? A.maxAdd : cap;
        if (blockIdx.x == 0) {
            A.ctl[kStage] = (unsigned long long)s.stage;
            A.ctl[kTolBits] = fray_budget::tolerance_bits(s);
            A.ctl[kCap] = (unsigned long long)(long long)cap;
        }
    }
    __syncthreads();
    const float tol = __uint_as_float(sTol);
    const int cap = sCap;
    unsigned long long t[2] = {0, 0};
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < A.n; p += (size_t)gridDim.x * blockDim.x) {
        const int N = A.count[p];
        const float2 r = A.rec[p];
        const int add = min(sm_add(N, r.x, r.y, tol, A.minCount, A.maxCount, A.maxAdd, A.grow), cap);
        A.add[p] = add;
        if (add > 0) { t[0]++; t[1] += (unsigned long long)add; }
    }
    block_sum<2>(t, A.ctl + kPixels);
}

using namespace frayhip_detail;
using namespace frayhip_temporal_detail;
using frayhip_samplemap_detail::check;

// frayhip_sample_map's checks under this entry's name, then the two of the budget
int check_budget(const char* who, int W, int H, const float* accum, const float* accum2, const int32_t* count, const struct frayhip_sample_map* p,
                 const struct frayhip_sample_budget* b, const int32_t* add, bool device)
{
    if (const int rc = check(who, W, H, accum, accum2, accum2 != nullptr, count, p, add, device)) return rc;
    if (!b) return bad(who, "null budget");
    if (b->reserved != 0) return bad(who, "reserved must be 0");
    return FRAYHIP_OK;
}

// The device path of both entries (device pointers, checked).  One synchronisation, at the end, whatever the data.
int run(const char* who, int W, int H, const float* accum, const float* accum2, const int32_t* count, struct frayhip_sample_map* p, struct frayhip_sample_budget* b,
        int32_t* add, hipStream_t stream, frayhip_stats* st, std::chrono::steady_clock::time_point t0)
{
    const size_t n = (size_t)W * H;
    // the call's workspace: the control block, then the records
    DeviceArrays B(std::string(who) + ": out of device memory");
    unsigned char* ws;
    const size_t head = r256(kWords * 8);
    if (const int rc = B.alloc(ws, head + n * sizeof(float2))) return rc;
    BudgetArgs A{};
    A.n = n;
    A.accum = (const float4*)accum; A.accum2 = (const float4*)accum2; A.count = count; A.add = add;
    A.ctl = (unsigned long long*)ws;
    A.rec = (float2*)(ws + head);
    A.budget = b->budget;
    A.tolerance = p->tolerance; A.lumFloor = p->lum_floor;
    A.minCount = p->min_count; A.maxCount = p->max_count; A.maxAdd = p->max_add; A.grow = p->grow;
    Events E;
    HIP_TRY(hipEventCreate(&E.a));
    HIP_TRY(hipEventCreate(&E.b));
    struct Drain { hipStream_t s; bool armed = true; ~Drain() { if (armed) (void)hipStreamSynchronize(s); } } drain{stream};
    const dim3 grid(grid_for(n)), block(256);
    HIP_TRY(hipMemsetAsync(A.ctl, 0, kWords * 8, stream));
    HIP_TRY(hipEventRecord(E.a, stream));
    if (accum2) hipLaunchKernelGGL(k_budget_prepare<true>, grid, block, 0, stream, A);
    else hipLaunchKernelGGL(k_budget_prepare<false>, grid, block, 0, stream, A);
    for (int k = 0; k < kLaunches; k++) hipLaunchKernelGGL(k_budget_search, grid, block, 0, stream, A, k);
    hipLaunchKernelGGL(k_budget_final, grid, block, 0, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(E.b, stream));
    unsigned long long h[kHead] = {};
    HIP_TRY(hipMemcpyAsync(h, A.ctl, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    drain.armed = false;
    p->pixels = h[kPixels];
    p->samples = h[kSamples];
    b->demand = h[kDemand];
    const uint32_t bits = (uint32_t)h[kTolBits];
    std::memcpy(&b->tolerance_used, &bits, 4);
    b->cap_used = (int32_t)(long long)h[kCap];
    b->stage = (int32_t)h[kStage];
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

int frayhip_sample_map_budget_device(int width, int height, const float* d_accum, const float* d_accum_indirect, const int32_t* d_count, struct frayhip_sample_map* p,
                                     struct frayhip_sample_budget* b, int32_t* d_add, void* hip_stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_sample_map_budget_device";
    if (const int rc = check_budget(who, width, height, d_accum, d_accum_indirect, d_count, p, b, d_add, true)) return rc;
    return run(who, width, height, d_accum, d_accum_indirect, d_count, p, b, d_add, (hipStream_t)hip_stream, st, t0);
}

int frayhip_sample_map_budget(int width, int height, const float* accum, const float* accum_indirect, const int32_t* count, struct frayhip_sample_map* p,
                              struct frayhip_sample_budget* b, int32_t* add, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const char* who = "frayhip_sample_map_budget";
    if (const int rc = check_budget(who, width, height, accum, accum_indirect, count, p, b, add, false)) return rc;
    const size_t n = (size_t)width * height;
    const size_t states = accum_indirect ? 2 : 1;
    // one allocation, the 16-byte rows first: the state(s), the counts, then add
    DeviceArrays B(std::string(who) + ": out of device memory");
    float* d_accum;
    if (const int rc = B.alloc(d_accum, n * (4 * states + 2))) return rc;
    float* d_indirect = accum_indirect ? d_accum + 4 * n : nullptr;
    int32_t* d_count = (int32_t*)(d_accum + 4 * states * n);
    int32_t* d_add = d_count + n;
    HIP_TRY(hipMemcpy(d_accum, accum, n * 16, hipMemcpyHostToDevice));
    if (d_indirect) HIP_TRY(hipMemcpy(d_indirect, accum_indirect, n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_count, count, n * 4, hipMemcpyHostToDevice));
    if (const int rc = run(who, width, height, d_accum, d_indirect, d_count, p, b, d_add, nullptr, st, t0)) return rc;
    HIP_TRY(hipMemcpy(add, d_add, n * 4, hipMemcpyDeviceToHost));
    if (st) st->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FRAYHIP_OK;
}

}  // extern "C"
