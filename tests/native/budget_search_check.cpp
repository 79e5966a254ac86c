// fray_amd/csrc/budget_search.hpp on the host: the 16-way search of a budgeted sample map against brute force.
//
// The kernels' protocol is restated here as they run it: a table of kLaunches x kCandidates totals, zeroed; launch k derives its interval by
// replaying launches 0 .. k-1 from the table, returns at once when the interval is closed, and otherwise stores the totals of its candidates in
// row k; the answer is the replay of all kLaunches rows.  The totals come from random monotone step functions:
//   stage 1   S over the bit patterns (lo, hi], non-increasing: wanted is the smallest x with S(x) <= budget
//   stage 2   T(c) = sum min(a_p, c) over random planes a, non-decreasing: wanted is the largest c in [0, max_add] with T(c) <= budget
// over intervals of width 1, 2, K-1, K, K+1, K+2, small random widths (brute force value by value) and up to 2^31 - 1 (brute force over the
// function's steps), with the step at either end, and the two cases that never reach the search (under the budget everywhere: stage 0; never
// under it: stage 2).  Prints the counts and the most launches any case needed; exit status 1 on a contradiction.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <vector>

#include "budget_search.hpp"

using namespace fray_budget;

static long long gCases = 0, gBad = 0;
static int gMostLaunches = 0;

// The kernels' sequence of launches; total(x): the sum at candidate x.  Returns the final state.
static Search run_launches(const Search& first, uint64_t budget, const std::function<uint64_t(uint32_t)>& total)
{
    std::vector<uint64_t> sums((size_t)kLaunches * kCandidates, 0);
    int used = 0;
    for (int k = 0; k < kLaunches; k++) {
        const Search s = replay(first, sums.data(), k, budget);
        if (!open(s)) continue;                                   // the launch returns after reading the control block
        used = k + 1;
        for (int j = 0; j < kCandidates; j++) {
            const uint32_t x = candidate(s, j);
            if (!(x > s.lo && x <= s.hi)) { gBad++; std::printf("candidate %u outside (%u, %u]\n", x, s.lo, s.hi); }
            sums[(size_t)k * kCandidates + j] = total(x);
        }
    }
    gMostLaunches = std::max(gMostLaunches, used);
    return replay(first, sums.data(), kLaunches, budget);
}

static void expect(bool ok, const char* what, const Search& s, uint64_t want)
{
    gCases++;
    if (ok) return;
    gBad++;
    if (gBad < 20) std::printf("CONTRADICTION %s: stage %d (%u, %u], wanted %llu\n", what, s.stage, s.lo, s.hi, (unsigned long long)want);
}

// A non-increasing step function on [lo, hi]: value v[i] from the i-th step on; steps sorted, in (lo, hi]
struct Steps {
    std::vector<uint32_t> at;
    std::vector<uint64_t> v;         // v[0] on [lo, at[0]), v[i + 1] from at[i] on; strictly decreasing
    uint64_t operator()(uint32_t x) const { return v[(size_t)(std::upper_bound(at.begin(), at.end(), x) - at.begin())]; }
};

static void check_stage1(uint32_t lo, uint32_t hi, const Steps& S, uint64_t budget)
{
    // stage 1's precondition: S(lo) > budget >= S(hi)
    if (!(S(lo) > budget && S(hi) <= budget)) return;
    uint64_t want = hi;
    for (size_t i = 0; i < S.at.size(); i++)
        if (S.v[i + 1] <= budget) { want = S.at[i]; break; }
    if ((uint64_t)hi - lo <= 4096) {            // value by value
        uint64_t brute = hi;
        for (uint64_t x = (uint64_t)lo + 1; x <= hi; x++)
            if (S((uint32_t)x) <= budget) { brute = x; break; }
        if (brute != want) { gBad++; std::printf("the harness disagrees with itself\n"); }
    }
    const Search end = run_launches(Search{1, lo, hi}, budget, [&](uint32_t x) { return S(x); });
    expect(!open(end) && end.hi - end.lo == 1 && tolerance_bits(end) == want, "stage 1", end, want);
}

static Steps random_steps(std::mt19937_64& rng, uint32_t lo, uint32_t hi, int mode)
{
    Steps S;
    const uint64_t w = (uint64_t)hi - lo;
    const int n = 1 + (int)(rng() % 6);
    for (int i = 0; i < n; i++) S.at.push_back((uint32_t)(lo + 1 + rng() % w));
    if (mode == 1) S.at.push_back(lo + 1);      // a step at the low end
    if (mode == 2) S.at.push_back(hi);          // and at the high end
    if (mode == 3) { S.at.clear(); S.at.push_back(lo + 1); }
    if (mode == 4) { S.at.clear(); S.at.push_back(hi); }
    std::sort(S.at.begin(), S.at.end());
    S.at.erase(std::unique(S.at.begin(), S.at.end()), S.at.end());
    uint64_t v = (1ull << 40) + rng() % (1ull << 36);       // sums past 2^32
    S.v.push_back(v);
    for (size_t i = 0; i < S.at.size(); i++) { v -= 1 + rng() % (v / (S.at.size() - i + 1) + 1); S.v.push_back(v); }
    return S;
}

static uint64_t capped_sum(const std::vector<uint32_t>& a, uint64_t c)
{
    uint64_t t = 0;
    for (uint32_t x : a) t += std::min<uint64_t>(x, c);
    return t;
}

static void check_stage2(const std::vector<uint32_t>& a, uint32_t maxAdd, uint64_t budget)
{
    // the plane is already capped at max_add (A(FLT_MAX) <= max_add); stage 2's precondition: T(max_add) > budget
    if (!(capped_sum(a, maxAdd) > budget)) return;
    uint64_t want;
    if (maxAdd <= 4096) {
        want = 0;
        for (uint64_t c = 0; c <= maxAdd; c++)
            if (capped_sum(a, c) <= budget) want = c;
    } else {                                     // T rises by (number of a_p > c) per unit: walk the sorted plane
        std::vector<uint32_t> s(a);
        std::sort(s.begin(), s.end());
        uint64_t c = 0, t = 0;
        for (size_t i = 0; i < s.size(); i++) {
            const uint64_t left = s.size() - i, rise = (uint64_t)s[i] - c;
            if (t + rise * left <= budget) { t += rise * left; c = s[i]; continue; }
            c += (budget - t) / left;
            break;
        }
        want = c;
    }
    const Search end = run_launches(Search{2, 0u, maxAdd}, budget, [&](uint32_t c) { return capped_sum(a, c); });
    expect(!open(end) && end.hi - end.lo == 1 && cap_of(end) == (int32_t)want && tolerance_bits(end) == kTolMaxBits, "stage 2", end, want);
}

int main(int argc, char** argv)
{
    const long long rounds = argc > 1 ? std::atoll(argv[1]) : 20000;
    std::mt19937_64 rng(20240607);
    const uint32_t K = kCandidates;
    const uint64_t widths[] = {1, 2, K - 1, K, K + 1, K + 2, 17 * 17, 17 * 17 + 1, 4096, 1u << 24, (1ull << 31) - 1};
    long long stage1 = 0, stage2 = 0;
    for (long long r = 0; r < rounds; r++) {
        for (uint64_t w : widths) {
            // stage 1: the interval anywhere in the positive floats' bit patterns, or the widest one of all
            const uint32_t lo = w == (1ull << 31) - 1 ? 0u : (uint32_t)(rng() % (0x7f7fffffull - w + 1));
            const uint32_t hi = (uint32_t)(lo + w);
            for (int mode = 0; mode < 5; mode++) {
                const Steps S = random_steps(rng, lo, hi, mode);
                // a budget at a step's value, one under it (the step is then not enough), or between two values
                const size_t i = 1 + rng() % (S.v.size() - 1);
                for (uint64_t budget : {S.v[i], S.v[i] - 1, S.v[i] + (S.v[i - 1] - S.v[i]) / 2, S.v.back(), S.v[0] - 1}) {
                    const long long before = gCases;
                    check_stage1(lo, hi, S, budget);
                    stage1 += gCases - before;
                }
            }
        }
        // stage 2: planes of 1 .. 40 pixels under max_add of every width above
        for (uint64_t w : widths) {
            const uint32_t maxAdd = (uint32_t)w;
            std::vector<uint32_t> a(1 + rng() % 40);
            for (uint32_t& x : a) x = (uint32_t)(rng() % ((uint64_t)maxAdd + 1));
            if (r % 3 == 0) a[0] = maxAdd;
            const uint64_t top = capped_sum(a, maxAdd);
            if (top == 0) continue;
            for (uint64_t budget : {(uint64_t)0, (uint64_t)1, top - 1, top / 2, top / 3, (uint64_t)a.size(), (uint64_t)a.size() - 1, rng() % top}) {
                const long long before = gCases;
                check_stage2(a, maxAdd, budget);
                stage2 += gCases - before;
            }
        }
    }
    // the stage of a budget: under it everywhere, under it only at the far end, never under it
    long long staged = 0;
    for (int r = 0; r < 1000; r++) {
        const uint64_t rest = rng() % 1000, demand = rest + rng() % 1000;
        const uint32_t tol = 1 + (uint32_t)(rng() % 0x7f7ffffeu), maxAdd = 1 + (uint32_t)(rng() % (1u << 24));
        for (uint64_t budget : {demand, demand + 1, demand - 1, rest, rest - 1, rest + 1, (uint64_t)0, ~(uint64_t)0}) {
            if (demand == 0 && budget == demand - 1) continue;
            if (rest == 0 && budget == rest - 1) continue;
            const Search s = start(demand, rest, budget, tol, maxAdd);
            const int want = demand <= budget ? 0 : rest <= budget ? 1 : 2;
            bool ok = s.stage == want;
            if (want == 0) ok = ok && !open(s) && tolerance_bits(s) == tol && cap_of(s) == -1;
            if (want == 1) ok = ok && s.lo == tol && s.hi == kTolMaxBits && cap_of(s) == -1;
            if (want == 2) ok = ok && s.lo == 0 && s.hi == maxAdd;
            expect(ok, "start", s, (uint64_t)want);
            staged++;
        }
    }
    std::printf("cases %lld (stage 1: %lld, stage 2: %lld, start: %lld), contradictions %lld, most launches %d of %d\n", gCases, stage1, stage2, staged, gBad,
                gMostLaunches, kLaunches);
    return gBad == 0 && gMostLaunches <= kLaunches && stage1 > 0 && stage2 > 0 ? 0 : 1;
}
