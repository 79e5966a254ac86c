// The radiance query (frayhip_shade_rays, include/frayhip.h) for one kernel flag word: the Makefile compiles this file eight times, -DFRAY_ST=0..5,
// 8, 9, into shade<ST>.o.  trace(ray, rnd) of the reference (main.cpp:286-293) for caller-supplied rays: raytrace() for Whitted scenes, pathtrace()
// with `gi on`.  Objects of their own: the frame kernels of render_variant.hip and the ray queries of query_variant.hip are compiled exactly as
// they were without them (kernels.hpp is not touched, only instantiated here once more).
//
//   k_seed_keyed        k_seed for a batch of (ray, sample) slots: x[397] of the seeding recurrence started at sample_seed(seed, key, sample)
//   k_whitted_rays<ST>  raytrace() per (ray, sample): k_whitted's persistent waves with per-lane refill and its step machine (dev_whitted.hpp),
//                       started from the caller's ray at depth 0 instead of a camera sample; the sample's colour goes to its slot
//   k_pt_init_rays<ST>  k_pt_init for caller-supplied rays: generators seeded from the key, rng_skip words of `rnd` discarded, the dense path queue
//   then the frame's own exact path-tracing kernels: k_meta_dense, k_pt_bounce<ST, false> / k_scan / k_pt_shadow<ST> per bounce, k_pt_fold
//   k_shade_resolve     per ray: the samples' colours added in sample order, the running FP32 sum kept across batches, / spp at the last one
//   k_shade_black       maxTraceDepth < 0: every ray is black
#include "shade.hpp"
#include "render_impl.hpp"

#ifndef FRAY_ST
#error "compile with -DFRAY_ST=0..5, 8 or 9"
#endif

namespace {

// One batch: rays r0 .. r0 + nr - 1 of the call, samples s0 .. s0 + cn - 1 of each; slot = s * nr + i (sample-major, as the frame's batches are).
struct ShadeRays {
    const double* org;
    const double* dir;
    const uint32_t* keys;         // null: key = ray index
    uint32_t seed;
    int r0, nr, s0, cn, skip;
};

FD bool finite3(V3 v) { return fabs(v.x) <= __DBL_MAX__ && fabs(v.y) <= __DBL_MAX__ && fabs(v.z) <= __DBL_MAX__; }
// frayhip_trace_rays' rule: a non-finite component, or a direction whose squared length is 0 or overflows, is not traced
FD bool load_ray(const ShadeRays& R, int g, V3& o, V3& d)
{
    const double* po = R.org + 3 * (size_t)g;
    const double* pd = R.dir + 3 * (size_t)g;
    o = v3(po[0], po[1], po[2]);
    d = v3(pd[0], pd[1], pd[2]);
    const double dd = d.x * d.x + d.y * d.y + d.z * d.z;
    return finite3(o) && dd > 0.0 && dd <= __DBL_MAX__;
}
FD uint32_t ray_key(const ShadeRays& R, int g) { return R.keys ? R.keys[g] : (uint32_t)g; }

// x397[slot] for the batch's slots (k_seed's recurrence, FRAY_SEED_CHAINS independent chains per lane)
static __global__ __launch_bounds__(256) void k_seed_keyed(ShadeRays R, uint32_t* __restrict__ x397)
{
    constexpr int NC = FRAY_SEED_CHAINS;
    const uint32_t total = (uint32_t)R.nr * (uint32_t)R.cn;
    const uint32_t groups = (total + NC - 1u) / NC;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
        uint32_t b[NC], slot[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) {
            slot[k] = q + (uint32_t)k * groups;
            b[k] = 0;
            if (slot[k] < total) {
                const int i = (int)(slot[k] % (uint32_t)R.nr), s = (int)(slot[k] / (uint32_t)R.nr);
                b[k] = sample_seed(R.seed, ray_key(R, R.r0 + i), (uint32_t)(R.s0 + s));
            }
        }
#pragma unroll 1
        for (uint32_t i = 1; i <= 397; i++) {
#pragma unroll
            for (int k = 0; k < NC; k++) b[k] = mt_lcg(b[k], i);
        }
#pragma unroll
        for (int k = 0; k < NC; k++) if (slot[k] < total) x397[slot[k]] = b[k];
    }
}

// Every sample counts in `samples`, with or without the counting variant (the frame's counters are zero without it; a query reports what it traced)
template <int ST>
FD void flush_query(DStats* st, const Cnt& c)
{
    if (ST & 1) flush_stats(st, c);
    else if (c.samples) atomicAdd(&st->samples, c.samples);
}

// raytrace() per (ray, sample) slot.  The driver of k_whitted<ST, 0> (kernels.hpp) without what a camera sample adds to it -- pixel items, jitter,
// lens, stereo eyes, the speculative fans -- so the per-lane sequence of steps, random draws and FP32 operations is k_whitted's, and the
// reference's.  The generator is the contract's getRandomGen() of the slot's (key, sample), from word 0: raytrace() draws nothing from the sample's
// own `rnd`, so rng_skip changes nothing here.
struct WhittedRaysArgs { DScene S; ShadeRays R; float* rad; uint32_t* mtWork; const uint32_t* x397; DStats* st; DCursors* cur; };
template <int ST>
static __global__ __launch_bounds__(256, whitted_waves(ST)) void k_whitted_rays(WhittedRaysArgs A)
{
    Cnt c = zero_cnt();
    MtLong tab;
    tab.stride = gridDim.x * blockDim.x;
    tab.st = A.mtWork + (blockIdx.x * blockDim.x + threadIdx.x);
    const int nr = A.R.nr;
    const int nTot = A.R.nr * A.R.cn;
    DCursors* const cur = A.cur;
    DStats* const st = A.st;
    const uint32_t lane = threadIdx.x & 63u;
    const SpecBuf SP{};                           // MODE 0 of the step machine: no fans
    WhittedLane L;
    L.mode = WM_NEXT_PIXEL; L.sp = 0;
    SpecLane SL;
    SL.state = 2; SL.sp = 0; SL.base = 0; SL.looked = 0; SL.missed = 0;
    int slot = 0;
    bool ovf = false;
    int poolNext = 0, poolEnd = 0, claimR = 0;
    for (;;) {
        const FRAY_RO WhittedRaysArgs* AP = kernel_args<WhittedRaysArgs>();
        const DScene& S = KARG(WhittedRaysArgs, AP, S);
        const ShadeRays& R = KARG(WhittedRaysArgs, AP, R);
        // ---- cheap steps, until every lane stands at a search, a direct-light loop, or has nothing left (k_whitted's rounds)
        for (;;) {
            const unsigned long long need = __ballot(L.mode == WM_NEXT_PIXEL);
            const unsigned long long busy = __ballot(L.mode != WM_NEXT_PIXEL && L.mode != WM_EXHAUSTED);
            const bool refill = need && ((int)__popcll(need) >= FRAY_WHITTED_REFILL || !busy);
            if (__any(L.mode < WM_NEXT_SAMPLE && tab.idx < 0 && tab.r.j >= FRAY_MT_EARLY)) {
                if (L.mode < WM_NEXT_SAMPLE && tab.idx < 0) tab.materialise();
            }
            const bool cheap = L.mode == WM_NEXT_PIXEL ? refill : (L.mode == WM_ROOT_RET || L.mode == WM_NEXT_SAMPLE || (L.mode < WM_ROOT_RET && wl_cheap(S, L)));
            if (!__any(cheap)) break;
            if (refill) {
                if (poolNext == poolEnd && claimR < 8) {
                    const int tile = claim_tile(cur, (nTot + 63) >> 6, claimR);
                    if (tile >= 0) { poolNext = tile * 64; poolEnd = poolNext + 64 < nTot ? poolNext + 64 : nTot; }
                }
                const int have = poolEnd - poolNext;
                const int rank = (int)__popcll(need & ((1ull << lane) - 1ull));
                if (L.mode == WM_NEXT_PIXEL) {
                    if (rank < have) { slot = poolNext + rank; L.mode = WM_NEXT_SAMPLE; }
                    else if (have == 0 && claimR >= 8) L.mode = WM_EXHAUSTED;
                }
                const int want = (int)__popcll(need);
                poolNext += want < have ? want : have;
            }
            if (L.mode == WM_NEXT_SAMPLE) {
                const int k = slot / nr, g = R.r0 + (slot - k * nr);
                V3 o, d;
                if (load_ray(R, g, o, d)) {
                    tab.reseed_with(sample_seed(R.seed, ray_key(R, g), (uint32_t)(R.s0 + k)), KARG(WhittedRaysArgs, AP, x397)[slot]);
                    c.samples++;
                    wl_start(L, o, d);
                } else {                                                  // degenerate: black, not traced, not counted
                    float* const rad = KARG(WhittedRaysArgs, AP, rad) + 3 * (size_t)slot;
                    rad[0] = 0; rad[1] = 0; rad[2] = 0;
                    L.mode = WM_NEXT_PIXEL;
                }
            } else if (L.mode == WM_ROOT_RET) {                              // the ray's raytrace() returned: the sample's colour
                float* const rad = KARG(WhittedRaysArgs, AP, rad) + 3 * (size_t)slot;
                rad[0] = L.ret.r; rad[1] = L.ret.g; rad[2] = L.ret.b;
                L.mode = WM_NEXT_PIXEL;
            } else if (L.mode < WM_ROOT_RET && wl_cheap(S, L)) {
                wl_cheap_step<ST, MtLong, 0>(S, L, tab, c, ovf, SP, SL);
            }
        }
        if (!__any(L.mode != WM_EXHAUSTED)) break;
        if (L.mode == WM_TRACE) wl_trace_step<ST>(S, L, c);
        if (L.mode == WM_SHADE && S.shaders[L.shader].kind <= 2) wl_direct_step<ST, MtLong>(S, L, tab, c);
    }
    if (ovf) atomicAdd(&st->rngOverflow, 1ull);
    flush_query<ST>(st, c);
    if ((ST & 2) && c.envelope) atomicAdd(&st->rngOverflow, 1ull);
}

// k_pt_init for caller-supplied rays: both generators of the contract seeded from (key, sample); `rnd` (the sample's own, which the frame's jitter
// draws from) advanced by rng_skip words, `tab` (getRandomGen(), which a thin lens would draw from) at word 0.  Degenerate rays get no path.
template <int ST>
static __global__ __launch_bounds__(256) void k_pt_init_rays(ShadeRays R, PathQueue Q, unsigned short* __restrict__ termCount, const uint32_t* __restrict__ x397, DStats* st)
{
    Cnt c = zero_cnt();
    const uint32_t total = (uint32_t)R.nr * (uint32_t)R.cn;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < total; slot += gridDim.x * blockDim.x) {
        const int k = (int)(slot / (uint32_t)R.nr), g = R.r0 + (int)(slot - (uint32_t)k * (uint32_t)R.nr);
        PathState ps;
        if (load_ray(R, g, ps.o, ps.d)) {
            ps.rnd = mt_seed_with(sample_seed(R.seed, ray_key(R, g), (uint32_t)(R.s0 + k)), x397[slot]);
            ps.tab = ps.rnd;
            mt_skip(ps.rnd, R.skip);
            ps.pm = c3(1, 1, 1);
            ps.slot = slot;
            ps.depth = 0;
            ps.flags = 0;
            c.samples++;
            path_store<FRAY_SORT && sort_variant(ST)>(Q, slot, ps, ray_sort_class<ST>(ps.d, 0u));
        } else {                                                            // k_pt_init's mark of a slot without a path
            PathRec* r = Q.rec + slot;
            r->d[0] = 0; r->d[1] = 0; r->d[2] = 0;
            r->depthFlags = FRAY_DEAD;
            if constexpr (FRAY_SORT && sort_variant(ST)) Q.cls[slot] = 15;
        }
        termCount[slot] = 0;
    }
    flush_query<ST>(st, c);
}

// rgb[i] = (sum over the ray's samples in sample order) / spp: k_pt_resolve's arithmetic per ray.  `s` is the batch's first sample counted from the
// call's first; `sum` carries the running FP32 sum between batches; rgb points at the batch's first ray.
static __global__ __launch_bounds__(256) void k_shade_resolve(int nr, int s, int cn, int spp, const float* __restrict__ rad, float* __restrict__ sum, float* __restrict__ rgb)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nr; i += gridDim.x * blockDim.x) {
        const size_t si = (size_t)i * 3;
        C3 a = s == 0 ? c3(0, 0, 0) : c3(sum[si], sum[si + 1], sum[si + 2]);
        for (int k = 0; k < cn; k++) {
            const size_t q = ((size_t)k * nr + i) * 3;
            a = a + c3(rad[q], rad[q + 1], rad[q + 2]);
        }
        if (s + cn >= spp) {
            a = a / (float)spp;
            rgb[si] = a.r; rgb[si + 1] = a.g; rgb[si + 2] = a.b;
        } else {
            sum[si] = a.r; sum[si + 1] = a.g; sum[si + 2] = a.b;
        }
    }
}

// maxTraceDepth < 0: raytrace() / pathtrace() return black before they look at the scene; every traceable ray's samples are counted, as k_black counts the frame's
static __global__ __launch_bounds__(256) void k_shade_black(ShadeRays R, float* __restrict__ rgb, DStats* st)
{
    unsigned long long n = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < R.nr; i += gridDim.x * blockDim.x) {
        V3 o, d;
        if (load_ray(R, i, o, d)) n += (unsigned long long)R.cn;
        rgb[3 * (size_t)i] = 0; rgb[3 * (size_t)i + 1] = 0; rgb[3 * (size_t)i + 2] = 0;
    }
    if (n) atomicAdd(&st->samples, n);
}

}  // namespace

namespace frayhip_detail {

// One call on ONE stream (the caller's): batches of (rays x samples) that fit the scene's work budget, rays outer, samples inner and in order.  Not the
// frame's batch lanes: kernels that keep spilled registers in scratch must not share the chip with other streams' kernels (render_impl, round 5), and
// a query has nothing to gain from the risk.
template <int ST>
int shade_impl(frayhip_scene* sc, const ShadeCall& q, hipStream_t stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const frayhip_settings& set = sc->settings;
    const DScene S = frame_scene(sc);
    const int n = q.n, spp = q.spp;
    ShadeRays R0{q.org, q.dir, q.keys, q.seed, 0, n, q.sampleFirst, spp, q.rngSkip};

    // Long generators (render_impl's longRng): k_pt_bounce<ST, true> derives a path's seed from its frame pixel (LongRng), which a keyed sample does not have
    if (const int rc = refuse_long_generators("frayhip_shade_rays", sc, "radiance queries")) return rc;
    HIP_TRY(hipMemsetAsync(sc->d_stats, 0, kStatsBytes, stream));
    DCursors* cursors = (DCursors*)((unsigned char*)sc->d_stats + kCursorOffset);
    HIP_TRY(hipEventRecord(sc->evA, stream));
    size_t nTraceEvents = 0, nShadowEvents = 0;

    if (set.maxTraceDepth < 0) {
        hipLaunchKernelGGL(k_shade_black, dim3(grid_for((size_t)n)), dim3(256), 0, stream, R0, q.rgb, sc->d_stats);
    } else if (!set.gi) {
        // workspace: k_whitted's per-thread generator columns, the rays' running sums, per slot of a batch the sample's colour and x[397] of its seed
        const int grid = persistent_grid((size_t)n * spp, whitted_waves(ST));
        const size_t colBytes = r256((size_t)grid * 256 * 624 * sizeof(uint32_t));
        int nr = 0, cn = 0;
        for (;;) {          // planned again with half the budget when the allocation fails
            const size_t wb = work_budget(sc);
            const size_t budget = wb > colBytes + (64u << 20) ? wb - colBytes : (64u << 20);
            const size_t slots = std::min<size_t>(std::max<size_t>(budget / 28, 64), (size_t)1 << 30);     // 16 bytes per slot, 12 per ray
            nr = (int)std::min<size_t>((size_t)n, slots);
            cn = (int)std::min<size_t>((size_t)spp, std::max<size_t>(1, slots / (size_t)nr));
            const size_t m = (size_t)nr * cn;
            const int rc = ensure_work_or_shrink(sc, colBytes + r256((size_t)nr * 12) + r256(m * 12) + r256(m * 4), m > 64);
            if (rc == FRAYHIP_RETRY_SMALLER) continue;
            if (rc) return rc;
            break;
        }
        Carve work{(unsigned char*)sc->d_work};
        uint32_t* mtWork = (uint32_t*)work.take(colBytes);
        float* sum = (float*)work.take((size_t)nr * 12);
        float* rad = (float*)work.take((size_t)nr * cn * 12);
        uint32_t* x397 = (uint32_t*)work.take((size_t)nr * cn * 4);
        bool first = true;
        for (int r0 = 0; r0 < n; r0 += nr) {
            const int mr = std::min(nr, n - r0);
            for (int s = 0; s < spp; s += cn) {
                const int c = std::min(cn, spp - s);
                const ShadeRays R{q.org, q.dir, q.keys, q.seed, r0, mr, q.sampleFirst + s, c, q.rngSkip};
                const size_t m = (size_t)mr * c;
                if (!first) HIP_TRY(hipMemsetAsync(cursors, 0, sizeof(DCursors), stream));     // the previous batch's tile cursors
                first = false;
                hipLaunchKernelGGL(k_seed_keyed, dim3(seed_grid((m + FRAY_SEED_CHAINS - 1) / FRAY_SEED_CHAINS)), dim3(256), 0, stream, R, x397);
                hipEvent_t a = pool_event(sc->evPool, nTraceEvents), b = pool_event(sc->evPool, nTraceEvents + 1);
                if (!a || !b) return FRAYHIP_E_NOMEM;
                HIP_TRY(hipEventRecord(a, stream));
                hipLaunchKernelGGL(k_whitted_rays<ST>, dim3(persistent_grid(m, whitted_waves(ST))), dim3(256), 0, stream,
                                   WhittedRaysArgs{S, R, rad, mtWork, x397, sc->d_stats, cursors});
                HIP_TRY(hipEventRecord(b, stream));
                nTraceEvents += 2;
                hipLaunchKernelGGL(k_shade_resolve, dim3(grid_for((size_t)mr)), dim3(256), 0, stream, mr, s, c, spp, (const float*)rad, sum, q.rgb + 3 * (size_t)r0);
            }
        }
    } else {
        const bool alone = (ST & 2) != 0;
        const int nBounce = set.maxTraceDepth + 2;
        const size_t termBytes = (size_t)nBounce * 12 + 2;
        int nr = 0, cn = 0;
        size_t nQueue = 0;
        for (;;) {          // planned again with half the budget when the allocation fails
            const size_t slots = std::min<size_t>(std::max<size_t>(work_budget(sc) / (240 + termBytes), 64), (size_t)1 << 30);
            nr = (int)std::min<size_t>((size_t)n, slots);
            cn = (int)std::min<size_t>((size_t)spp, std::max<size_t>(1, slots / (size_t)nr));
            const size_t m = (size_t)nr * cn;
            nQueue = m + (size_t)bounce_grid(m, alone) * 4 * 128;          // per-wave segments round their share up to a multiple of 64
            const size_t bytes = r256((size_t)nr * 12) + 2 * queue_bytes(nQueue) + shadow_bytes(nQueue) + r256(m * 12) + r256(m * 4) +
                                 r256(m * (size_t)nBounce * 12) + r256(m * 2);
            const int rc = ensure_work_or_shrink(sc, bytes, m > 64);
            if (rc == FRAYHIP_RETRY_SMALLER) continue;
            if (rc) return rc;
            break;
        }
        const size_t nPaths = (size_t)nr * cn;
        unsigned char* p = (unsigned char*)sc->d_work;
        float* sum = (float*)p; p += r256((size_t)nr * 12);
        PathQueue Q[2];
        ShadowQueue SQ;
        p = carve_queue(p, nQueue, Q[0]);
        p = carve_queue(p, nQueue, Q[1]);
        p = carve_shadow(p, nQueue, SQ);
        float* rad = (float*)p; p += r256(nPaths * 12);
        uint32_t* x397 = (uint32_t*)p; p += r256(nPaths * 4);
        float* terms = (float*)p; p += r256(nPaths * (size_t)nBounce * 12);
        unsigned short* termCount = (unsigned short*)p;
        QMeta* meta = sc->d_qmeta;
        for (int r0 = 0; r0 < n; r0 += nr) {
            const int mr = std::min(nr, n - r0);
            for (int s = 0; s < spp; s += cn) {
                const int c = std::min(cn, spp - s);
                const ShadeRays R{q.org, q.dir, q.keys, q.seed, r0, mr, q.sampleFirst + s, c, q.rngSkip};
                const size_t m = (size_t)mr * c;
                hipLaunchKernelGGL(k_seed_keyed, dim3(seed_grid((m + FRAY_SEED_CHAINS - 1) / FRAY_SEED_CHAINS)), dim3(256), 0, stream, R, x397);
                hipLaunchKernelGGL(k_meta_dense, dim3(1), dim3(64), 0, stream, meta, (uint32_t)m);
                hipLaunchKernelGGL(k_pt_init_rays<ST>, dim3(grid_for(m)), dim3(256), 0, stream, R, Q[0], termCount, (const uint32_t*)x397, sc->d_stats);
                if (const int rc = pt_bounces<ST>(sc, S, Q, SQ, TermBuf{terms, termCount, (uint32_t)nPaths, 0}, nBounce, bounce_grid(m, alone), stream, nTraceEvents, nShadowEvents))
                    return rc;
                // a sample's radiance from its terms, innermost first (k_pt_resolve_terms' order), then the per-ray sum in sample order
                hipLaunchKernelGGL(k_pt_fold, dim3(grid_for(m)), dim3(256), 0, stream, TermBuf{terms, termCount, (uint32_t)nPaths, 0}, (uint32_t)m, rad);
                hipLaunchKernelGGL(k_shade_resolve, dim3(grid_for((size_t)mr)), dim3(256), 0, stream, mr, s, c, spp, (const float*)rad, sum, q.rgb + 3 * (size_t)r0);
            }
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc->evB, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    DStats dsv[2];
    HIP_TRY(hipMemcpy(dsv, sc->d_stats, sizeof dsv, hipMemcpyDeviceToHost));
    if (dsv[0].rngOverflow || dsv[1].rngOverflow) {
        set_error("frayhip_shade_rays: a sample left the supported envelope (Whitted: shade() nesting deeper than 40; path tracing: a generator past 227 words; "
                  "a CsgOp operand with more intersections than the device path holds)");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if (st) *st = finish_stats(sc, dsv, 2, nTraceEvents, nShadowEvents, t0);
    return FRAYHIP_OK;
}

template int shade_impl<FRAY_ST>(frayhip_scene*, const ShadeCall&, hipStream_t, frayhip_stats*);

}  // namespace frayhip_detail
