// The search of a budgeted sample map (include/frayhip.h "sample maps", frayhip_sample_map_budget): which stage a budget falls into, the candidates
// one launch evaluates and how the launch after it narrows the interval from their sums.  Pure integer code, host and device, no HIP header: the
// kernels of samplemap_budget.hip replay it from a control block in device memory, and tests/native/budget_search_check.cpp runs it on the CPU
// against brute force.
//
// The problem, in both searched stages: an interval (lo, hi] of 32-bit values and a predicate that is false at lo, true at hi and monotone
// (false ... false true ... true); wanted is the smallest x in (lo, hi] at which it is true.
//   stage 1   x is the bit pattern of a positive float tolerance (positive floats are ordered as their bit patterns), (lo, hi] = (bits(tolerance),
//             bits(FLT_MAX)], the predicate is S(x) <= budget; S is non-increasing in x.  The answer is tolerance_used.
//   stage 2   x is a per-pixel cap, (lo, hi] = (0, max_add], the predicate is T(x) > budget with T(c) = sum min(A(FLT_MAX)[p], c), non-decreasing in c;
//             T(0) = 0 <= budget and T(max_add) = S(FLT_MAX) > budget.  The answer is one above cap_used.
//
// One launch evaluates kCandidates = 16 values x_0 <= ... <= x_15 of (lo, hi]:
//   w = hi - lo <= 17:  x_j = min(lo + 1 + j, hi): every value of the interval short of hi, whose predicate is known; the step leaves width 1.
//   w > 17:             x_j = lo + floor((j + 1) w / 17), strictly between lo and hi and strictly increasing.
// With x_-1 = lo and x_16 = hi, the next interval is (x_{j-1}, x_j] for the first j whose predicate is true.
// TERMINATION.  For w > 17, x_j - x_{j-1} = floor((j + 1) w / 17) - floor(j w / 17) <= ceil(w / 17) for j = 0 .. 16 (x_16 = lo + floor(17 w / 17)
// = hi), so a step takes width w to at most ceil(w / 17), and to exactly 1 once w <= 17.  A tolerance's interval has at most 2^31 bit patterns
// (0x7f7fffff - 1): 2^31 -> 126322568 -> 7430740 -> 437103 -> 25712 -> 1513 -> 89 -> 6 -> 1, eight steps; a cap's is (0, max_add], 2^24 wide by default (six
// steps) and below 2^31 for any int32 max_add.  kLaunches = 8 therefore always ends at width 1, where hi is the answer; a step at width 1 changes nothing, so the launches past the
// last useful one return at once and their sums stay zero (replay does not read them).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FRAY_BS_HD __host__ __device__
#else
#define FRAY_BS_HD
#endif

namespace fray_budget {

constexpr int kCandidates = 16;
#ifndef FRAY_BUDGET_LAUNCHES
#define FRAY_BUDGET_LAUNCHES 8      // the host check builds a copy with 7 to see the widest intervals stay open
#endif
constexpr int kLaunches = FRAY_BUDGET_LAUNCHES;
constexpr uint32_t kTolMaxBits = 0x7f7fffffu;     // FLT_MAX

struct Search {
    int stage;              // 0, 1, 2
    uint32_t lo, hi;        // stages 1 and 2: the predicate is false at lo and true at hi
};

// The stage of a budget: demand = S(tolerance), rest = S(FLT_MAX)
FRAY_BS_HD inline Search start(uint64_t demand, uint64_t rest, uint64_t budget, uint32_t tolBits, uint32_t maxAdd)
{
    if (demand <= budget) return Search{0, tolBits, tolBits};
    if (rest <= budget) return Search{1, tolBits, kTolMaxBits};       // tolBits < kTolMaxBits here: equal tolerances have equal sums
    return Search{2, 0u, maxAdd};
}

FRAY_BS_HD inline bool open(const Search& s) { return s.stage != 0 && s.hi - s.lo > 1u; }

FRAY_BS_HD inline uint32_t candidate(const Search& s, int j)
{
    const uint64_t w = (uint64_t)s.hi - s.lo;
    if (w <= (uint64_t)kCandidates + 1) {
        const uint64_t x = (uint64_t)s.lo + 1 + (uint64_t)j;
        return x < s.hi ? (uint32_t)x : s.hi;
    }
    return s.lo + (uint32_t)(((uint64_t)(j + 1) * w) / (uint64_t)(kCandidates + 1));
}

// The interval after a launch whose candidates summed to sums[0 .. kCandidates)
FRAY_BS_HD inline Search narrow(const Search& s, const uint64_t* sums, uint64_t budget)
{
    if (!open(s)) return s;
    Search n = s;
    for (int j = 0; j < kCandidates; j++) {
        const uint32_t x = candidate(s, j);
        const bool pred = s.stage == 1 ? sums[j] <= budget : sums[j] > budget;
        if (pred) { n.hi = x; return n; }
        n.lo = x;
    }
    return n;
}

// The interval that launch number `launches` of the search starts from: sums holds kCandidates totals per earlier launch
FRAY_BS_HD inline Search replay(Search s, const uint64_t* sums, int launches, uint64_t budget)
{
    for (int k = 0; k < launches && open(s); k++) s = narrow(s, sums + (size_t)k * kCandidates, budget);
    return s;
}

// What the final plane is made with
FRAY_BS_HD inline uint32_t tolerance_bits(const Search& s) { return s.stage == 0 ? s.lo : s.stage == 1 ? s.hi : kTolMaxBits; }
FRAY_BS_HD inline int32_t cap_of(const Search& s) { return s.stage == 2 ? (int32_t)(s.hi - 1u) : -1; }

}  // namespace fray_budget
