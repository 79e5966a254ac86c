// Adaptive frames (frayhip_render_adaptive, include/frayhip.h) for one kernel flag word: the Makefile compiles this file eight times, -DFRAY_ST=0..5,
// 8, 9, into adaptive<ST>.o.  A path-traced mono frame whose pixels climb a ladder of sample counts and stop where their noise estimate is small
// enough.  Objects of their own: the frame kernels of render_variant.hip are compiled exactly as they were without them (kernels.hpp is not
// touched, only instantiated here once more).
//
// Per rung, for the rung's active pixel list (ascending work items, so a wave holds neighbouring pixels of one 8x8 tile):
//   k_seed_list          x[397] of the seeding recurrence for (active pixel, sample) slots, key y * W + x (k_seed's recurrence)
//   k_pt_init_list<ST>   k_pt_init's mono branch for the listed pixels: jitter, camera / thin-lens ray, the dense path queue
//   then the frame's own exact path-tracing kernels: k_meta_dense, k_pt_bounce<ST, false> / k_scan / k_pt_shadow<ST> per bounce
//   k_adaptive_resolve   per active pixel: the batch's samples added to the running FP32 sum in sample order (terms innermost first); at the
//                        rung's last batch the mean, the error against the previous rung's mean, the outputs of a pixel that stops, its flag
//   k_compact_count / k_compact_scan / k_compact_write   the next rung's list: the flagged entries, in their order, and their count
// k_list_init starts the list (every work item of the call's buckets whose pixel lies inside the frame); k_adaptive_black answers maxTraceDepth < 0.
// The list and compaction kernels are dev_compact.hpp's, shared with sample maps.
#include "adaptive.hpp"
#include "dev_compact.hpp"
#include "render_impl.hpp"

#ifndef FRAY_ST
#error "compile with -DFRAY_ST=0..5, 8 or 9"
#endif

namespace {

// One batch: entries p0 .. p0 + np - 1 of the rung's list (work items of the frame's buckets), samples s0 .. s0 + cn - 1 of each;
// slot = s * np + i (sample-major, as the frame's batches are)
struct ListBatch {
    const int* list;
    int p0, np, s0, cn;
};

// x397[slot] for the batch's slots: k_seed's recurrence (FRAY_SEED_CHAINS independent chains per lane), keyed by the listed pixel
static __global__ __launch_bounds__(256) void k_seed_list(DFrame F, ListBatch B, uint32_t* __restrict__ x397)
{
    constexpr int NC = FRAY_SEED_CHAINS;
    const uint32_t total = (uint32_t)B.np * (uint32_t)B.cn;
    const uint32_t groups = (total + NC - 1u) / NC;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
        uint32_t b[NC], slot[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) {
            slot[k] = q + (uint32_t)k * groups;
            b[k] = 0;
            if (slot[k] < total) {
                const int i = (int)(slot[k] % (uint32_t)B.np), s = (int)(slot[k] / (uint32_t)B.np);
                int x, y;
                item_pixel(F, B.list[B.p0 + i], x, y);
                b[k] = sample_seed(F.seed, (uint32_t)y * (uint32_t)F.W + (uint32_t)x, (uint32_t)(B.s0 + s));
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

// k_pt_init's mono branch (kernels.hpp) with the pixel taken from the list: both generators seeded from (pixel, sample), two jitter floats from
// `rnd`, the camera ray through the jittered film position -- or, with DOF, the thin-lens ray drawn from `tab`.  Every listed pixel lies inside
// the frame, so every slot holds a path.  Every sample counts in `samples`, with or without the counting variant (the call reports what it traced).
template <int ST>
static __global__ __launch_bounds__(256) void k_pt_init_list(DCamera C, DFrame F, ListBatch B, PathQueue Q, unsigned short* __restrict__ termCount,
                                                             const uint32_t* __restrict__ x397, DStats* st)
{
    Cnt c = zero_cnt();
    const uint32_t total = (uint32_t)B.np * (uint32_t)B.cn;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < total; slot += gridDim.x * blockDim.x) {
        const int i = (int)(slot % (uint32_t)B.np), s = (int)(slot / (uint32_t)B.np);
        int x, y;
        item_pixel(F, B.list[B.p0 + i], x, y);
        PathState ps;
        const uint32_t p = (uint32_t)y * (uint32_t)F.W + (uint32_t)x;
        ps.rnd = mt_seed_with(sample_seed(F.seed, p, (uint32_t)(B.s0 + s)), x397[slot]);
        ps.tab = ps.rnd;
        float ox = rng_float(ps.rnd), oy = rng_float(ps.rnd);           // gi: always jittered (main.cpp:351-353)
        double fx = (double)((float)x + ox), fy = (double)((float)y + oy);
        if (C.dof) dof_ray(C, fx, fy, ps.tab, ps.o, ps.d); else screen_ray(C, fx, fy, ps.o, ps.d);
        ps.pm = c3(1, 1, 1);
        ps.slot = slot;
        ps.depth = 0;
        ps.flags = 0;
        c.samples++;
        path_store<FRAY_SORT && sort_variant(ST)>(Q, slot, ps, ray_sort_class<ST>(ps.d, 0u));
        termCount[slot] = 0;
    }
    if (ST & 1) flush_stats(st, c);
    else if (c.samples) atomicAdd(&st->samples, c.samples);
}

// Per-pixel state of a call, indexed by work item: the running FP32 sum of the samples so far and the mean at the previous rung.  Per entry of
// the rung's list: the pixel's continue flag.
struct PixelState {
    float* sum;
    float* prev;
    unsigned char* flag;
};

// Outputs (device, frame-sized; spp / err may be null) and the rung: its sample count r, whether it is rung 0 (no error yet), the frame's spp and
// the stop rule
struct ResolveArgs {
    DFrame F;
    ListBatch B;
    int sBefore;                  // samples of each listed pixel before this batch (0: the sum starts here)
    bool last;                    // the rung's last batch
    bool first;                   // rung 0
    int r, spp;
    double threshold, errFloor;
    TermBuf TB;
    PixelState P;
    float* rgb;
    int32_t* sppOut;
    float* errOut;
};

// The pixel's error at a rung (include/frayhip.h): in double, each FP32 operand widened first, in this order (no contraction: -ffp-contract=off)
FD double adaptive_err(C3 m, C3 h, double errFloor)
{
    const double num = (fabs((double)m.r - (double)h.r) + fabs((double)m.g - (double)h.g)) + fabs((double)m.b - (double)h.b);
    const double den = errFloor + (((double)m.r + (double)m.g) + (double)m.b);
    return num / den;
}

// k_pt_resolve_terms' arithmetic per listed pixel (each sample's terms innermost first, the samples in sample order, / (float)r), the running sum
// carried between batches and rungs.  At the rung's last batch: rung 0 keeps the mean for the error of rung 1; a later rung computes the error, and a
// pixel that stops (err <= threshold, or r == spp; a NaN error does not stop it) gets its outputs.
static __global__ __launch_bounds__(256) void k_adaptive_resolve(ResolveArgs A)
{
    const ListBatch& B = A.B;
    const TermBuf& TB = A.TB;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B.np; i += gridDim.x * blockDim.x) {
        const int item = B.list[B.p0 + i];
        const size_t si = (size_t)item * 3;
        C3 a = A.sBefore == 0 ? c3(0, 0, 0) : c3(A.P.sum[si], A.P.sum[si + 1], A.P.sum[si + 2]);
        for (int s = 0; s < B.cn; s++) {
            const uint32_t slot = (uint32_t)s * (uint32_t)B.np + (uint32_t)i;
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
            a = a + result;
        }
        A.P.sum[si] = a.r; A.P.sum[si + 1] = a.g; A.P.sum[si + 2] = a.b;
        if (!A.last) continue;
        const C3 m = a / (float)A.r;
        bool stop = false;
        if (!A.first) {
            const C3 h = c3(A.P.prev[si], A.P.prev[si + 1], A.P.prev[si + 2]);
            const double err = adaptive_err(m, h, A.errFloor);
            stop = err <= A.threshold || A.r == A.spp;
            if (stop) {
                int x, y;
                item_pixel(A.F, item, x, y);
                const size_t p = (size_t)y * A.F.W + x;
                A.rgb[3 * p] = m.r; A.rgb[3 * p + 1] = m.g; A.rgb[3 * p + 2] = m.b;
                if (A.sppOut) A.sppOut[p] = A.r;
                if (A.errOut) A.errOut[p] = (float)err;
            }
        }
        A.P.prev[si] = m.r; A.P.prev[si + 1] = m.g; A.P.prev[si + 2] = m.b;
        A.P.flag[B.p0 + i] = stop ? 0 : 1;
    }
}

// maxTraceDepth < 0: pathtrace() returns black before it looks at the scene; every pixel stops at min_spp with error 0, its samples counted
static __global__ __launch_bounds__(256) void k_adaptive_black(DFrame F, int nItems, int minSpp, float* __restrict__ rgb, int32_t* __restrict__ sppOut,
                                                               float* __restrict__ errOut, DStats* st)
{
    unsigned long long n = 0;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nItems; item += gridDim.x * blockDim.x) {
        int x, y;
        if (!item_pixel(F, item, x, y)) continue;
        const size_t p = (size_t)y * F.W + x;
        rgb[3 * p] = 0; rgb[3 * p + 1] = 0; rgb[3 * p + 2] = 0;
        if (sppOut) sppOut[p] = minSpp;
        if (errOut) errOut[p] = 0;
        n += (unsigned long long)minSpp;
    }
    if (n) atomicAdd(&st->samples, n);
}

}  // namespace

namespace frayhip_detail {

// One call on ONE stream (the caller's), as shade_impl: kernels that keep spilled registers in scratch must not share the chip with other streams'
// kernels (render_impl, round 5).  Per rung, batches of (listed pixels x samples) that fit the scene's work budget, pixel ranges outer, samples
// inner and in order; the host reads the next rung's list length once per rung.
template <int ST>
int adaptive_impl(frayhip_scene* sc, AdaptiveCall& q, hipStream_t stream, frayhip_stats* st)
{
    const auto t0 = std::chrono::steady_clock::now();
    const frayhip_settings& set = sc->settings;
    const DFrame F = frame_record(sc, q.bucketFirst, q.bucketStride, q.seed);          // spp: q.spp, the frame's; jitter on (gi)
    const int nItems = F.nBuckets * 2304;
    const DScene S = frame_scene(sc);
    const DCamera C = camera_begin_frame(sc->camera, F.W, F.H);
    const std::vector<int> ladder = adaptive_ladder(q.minSpp, q.spp);

    // an adaptive frame is a frame: the last frame's figures are its own (it runs no contracted kernel and no speculative fan)
    sc->lastContracted = 0;
    for (int k = 0; k < 4; k++) sc->lastFans[k] = 0;
    q.rungs = 0;
    q.samples = 0;
    HIP_TRY(hipMemsetAsync(sc->d_stats, 0, kStatsBytes, stream));
    HIP_TRY(hipEventRecord(sc->evA, stream));
    size_t nTraceEvents = 0, nShadowEvents = 0;

    if (nItems > 0 && set.maxTraceDepth < 0) {
        hipLaunchKernelGGL(k_adaptive_black, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, q.minSpp, q.rgb, q.sppOut, q.errOut, sc->d_stats);
        q.rungs = 2;
    } else if (nItems > 0) {
        const bool alone = (ST & 2) != 0;
        const int nBounce = set.maxTraceDepth + 2;
        const size_t termBytes = (size_t)nBounce * 12 + 2;
        const int nTiles = (nItems + kTile - 1) / kTile;
        // per work item: sum and previous mean (24 B), two lists (8 B), a flag; per tile: count and offset
        const size_t stateBytes = 2 * r256((size_t)nItems * 12) + 2 * r256((size_t)nItems * 4) + r256((size_t)nItems) + 2 * r256((size_t)nTiles * 4) + 256;
        int maxRung = ladder[0];
        for (size_t j = 1; j < ladder.size(); j++) maxRung = std::max(maxRung, ladder[j] - ladder[j - 1]);
        if (q.sppChunk > 0) maxRung = std::min(maxRung, q.sppChunk);
        size_t slots = 0, nQueue = 0;
        for (;;) {          // planned again with half the budget when the allocation fails
            const size_t wb = work_budget(sc);
            const size_t budget = wb > stateBytes + (64u << 20) ? wb - stateBytes : (64u << 20);
            slots = std::min<size_t>(std::max<size_t>(budget / (240 + termBytes), 64), (size_t)1 << 30);
            slots = std::min<size_t>(slots, (size_t)nItems * (size_t)maxRung);
            nQueue = slots + (size_t)bounce_grid(slots, alone) * 4 * 128;          // per-wave segments round their share up to a multiple of 64
            const size_t bytes = stateBytes + 2 * queue_bytes(nQueue) + shadow_bytes(nQueue) + r256(slots * 4) + r256(slots * (size_t)nBounce * 12) + r256(slots * 2);
            const int rc = ensure_work_or_shrink(sc, bytes, q.sppChunk <= 0 && slots > 64);
            if (rc == FRAYHIP_RETRY_SMALLER) continue;
            if (rc) return rc;
            break;
        }
        Carve work{(unsigned char*)sc->d_work};
        PixelState P;
        P.sum = (float*)work.take((size_t)nItems * 12);
        P.prev = (float*)work.take((size_t)nItems * 12);
        int* list[2] = {(int*)work.take((size_t)nItems * 4), (int*)work.take((size_t)nItems * 4)};
        P.flag = work.take((size_t)nItems);
        int* tileCount = (int*)work.take((size_t)nTiles * 4);
        int* tileOffset = (int*)work.take((size_t)nTiles * 4);
        int* dCount = (int*)work.take(256);
        PathQueue Q[2];
        ShadowQueue SQ;
        work.p = carve_queue(work.p, nQueue, Q[0]);
        work.p = carve_queue(work.p, nQueue, Q[1]);
        work.p = carve_shadow(work.p, nQueue, SQ);
        uint32_t* x397 = (uint32_t*)work.take(slots * 4);
        float* terms = (float*)work.take(slots * (size_t)nBounce * 12);
        unsigned short* termCount = (unsigned short*)work.take(slots * 2);
        QMeta* meta = sc->d_qmeta;

        // the list's new length, read back once per compaction
        int cur = 0;
        auto compact = [&](int n, int& out) -> int {
            const int tiles = (n + kTile - 1) / kTile;
            hipLaunchKernelGGL(k_compact_count, dim3(tiles), dim3(256), 0, stream, (const unsigned char*)P.flag, n, tileCount);
            hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, stream, (const int*)tileCount, tiles, tileOffset, dCount);
            hipLaunchKernelGGL(k_compact_write, dim3(tiles), dim3(256), 0, stream, (const int*)list[cur], (const unsigned char*)P.flag, n, (const int*)tileOffset, list[cur ^ 1]);
            HIP_TRY(hipMemcpyAsync(&out, dCount, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            cur ^= 1;
            return FRAYHIP_OK;
        };
        int nActive = 0;
        hipLaunchKernelGGL(k_list_init, dim3(grid_for((size_t)nItems)), dim3(256), 0, stream, F, nItems, list[0], P.flag);
        if (const int rc = compact(nItems, nActive)) return rc;

        for (size_t j = 0; j < ladder.size() && nActive > 0; j++) {
            const int sLo = j == 0 ? 0 : ladder[j - 1], r = ladder[j], rs = r - sLo;
            const int np = (int)std::min<size_t>((size_t)nActive, slots);
            int cn = (int)std::min<size_t>((size_t)rs, std::max<size_t>(1, slots / (size_t)np));
            if (q.sppChunk > 0) cn = std::min(cn, q.sppChunk);
            q.rungs++;
            q.samples += (uint64_t)nActive * (uint64_t)rs;
            for (int p0 = 0; p0 < nActive; p0 += np) {
                const int mp = std::min(np, nActive - p0);
                for (int s = 0; s < rs; s += cn) {
                    const int c = std::min(cn, rs - s);
                    const ListBatch B{list[cur], p0, mp, sLo + s, c};
                    const size_t m = (size_t)mp * c;
                    hipLaunchKernelGGL(k_seed_list, dim3(seed_grid((m + FRAY_SEED_CHAINS - 1) / FRAY_SEED_CHAINS)), dim3(256), 0, stream, F, B, x397);
                    hipLaunchKernelGGL(k_meta_dense, dim3(1), dim3(64), 0, stream, meta, (uint32_t)m);
                    hipLaunchKernelGGL(k_pt_init_list<ST>, dim3(grid_for(m)), dim3(256), 0, stream, C, F, B, Q[0], termCount, (const uint32_t*)x397, sc->d_stats);
                    if (const int rc = pt_bounces<ST>(sc, S, Q, SQ, TermBuf{terms, termCount, (uint32_t)slots, 0}, nBounce, bounce_grid(m, alone), stream, nTraceEvents, nShadowEvents))
                        return rc;
                    const ResolveArgs RA{F, B, sLo + s, s + c >= rs, j == 0, r, q.spp, q.threshold, q.errFloor, TermBuf{terms, termCount, (uint32_t)slots, 0}, P,
                                         q.rgb, q.sppOut, q.errOut};
                    hipLaunchKernelGGL(k_adaptive_resolve, dim3(grid_for((size_t)mp)), dim3(256), 0, stream, RA);
                }
            }
            // rung 0 stops no pixel; the last rung stops every one
            if (j > 0 && j + 1 < ladder.size())
                if (const int rc = compact(nActive, nActive)) return rc;
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sc->evB, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    DStats dsv[2];
    HIP_TRY(hipMemcpy(dsv, sc->d_stats, sizeof dsv, hipMemcpyDeviceToHost));
    if (set.maxTraceDepth < 0) q.samples = dsv[0].samples;          // min_spp per pixel of the call's buckets
    if (dsv[0].rngOverflow || dsv[1].rngOverflow) {
        set_error("frayhip_render_adaptive: a camera sample left the supported envelope (a generator past 227 words; a CsgOp operand with more "
                  "intersections than the device path holds)");
        return FRAYHIP_E_UNSUPPORTED;
    }
    if (st) *st = finish_stats(sc, dsv, 2, nTraceEvents, nShadowEvents, t0);
    return FRAYHIP_OK;
}

template int adaptive_impl<FRAY_ST>(frayhip_scene*, AdaptiveCall&, hipStream_t, frayhip_stats*);

}  // namespace frayhip_detail
