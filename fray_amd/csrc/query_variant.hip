// The ray query kernels for one kernel flag word (the Makefile compiles this file eight times, -DFRAY_ST=0..5, 8, 9, into query<ST>.o).  They live
// in objects of their own: the frame kernels of render_variant.hip are compiled exactly as they were without them.
//
//   k_query_closest<ST, REC>   closest_hit for caller-supplied rays (frayhip_trace_rays), the k_primary loop with rows for camera rays; REC: the
//                              winner's IntersectionInfo (finalize_hit, or the light's light_record) as well
//   k_query_visible<ST>        visible(a, b) for caller-supplied segments (frayhip_visible)
#include "query.hpp"
#include "kernels.hpp"

#ifndef FRAY_ST
#error "compile with -DFRAY_ST=0..5, 8 or 9"
#endif

using frayhip_detail::QueryArgs;

// Waves per SIMD: k_primary's and the any-hit kernels' (primary_waves, anyhit_waves), except in the timed KD variant, where at their 4 waves the
// query kernels spilled VGPRs (10 for ids + dist, 39 with the record, 6 for visible; k_primary<4> itself spills 2): at 3 they spill none.
#ifndef FRAY_QUERY_WAVES_KD
#define FRAY_QUERY_WAVES_KD 3
#endif
constexpr int query_closest_waves(int st) { return st == 4 ? FRAY_QUERY_WAVES_KD : primary_waves(st); }
constexpr int query_visible_waves(int st) { return st == 4 ? FRAY_QUERY_WAVES_KD : anyhit_waves(st); }

FD bool finite3(V3 v) { return fabs(v.x) <= __DBL_MAX__ && fabs(v.y) <= __DBL_MAX__ && fabs(v.z) <= __DBL_MAX__; }

// Persistent waves claim 64-item tiles as k_primary's do; the last tile's lanes past n idle.
template <int ST, bool REC>
static __global__ __launch_bounds__(256, query_closest_waves(ST)) void k_query_closest(QueryArgs A)
{
    Cnt c = zero_cnt();
    const int n = A.n, nItems = (n + 63) & ~63;
    DCursors* const cur = A.cur;
    for (int r = 0, i = claim_items(cur, nItems, r); i < nItems; i = claim_items(cur, nItems, r)) {
        if (i >= n) continue;
        const FRAY_RO QueryArgs* AP = kernel_args<QueryArgs>();
        const DScene& S = KARG(QueryArgs, AP, S);
        const double* const po = KARG(QueryArgs, AP, a) + 3 * (size_t)i;
        const double* const pd = KARG(QueryArgs, AP, b) + 3 * (size_t)i;
        const V3 o = v3(po[0], po[1], po[2]), d = v3(pd[0], pd[1], pd[2]);
        // a non-finite component or a direction that cannot be normalised (squared length 0 or overflowing) is a miss, not traced
        const double dd = d.x * d.x + d.y * d.y + d.z * d.z;
        HitT<ST> h;
        h.node = -1;
        h.dist = 1e99;
        if (finite3(o) && dd > 0.0 && dd <= __DBL_MAX__) closest_hit<ST>(S, o, d, h, c);
        int32_t* const hitId = KARG(QueryArgs, AP, hitId);
        double* const hitDist = KARG(QueryArgs, AP, hitDist);
        if (hitId) hitId[i] = h.node;
        if (hitDist) hitDist[i] = h.dist;
        if constexpr (REC) {
            V3 ip = v3(0, 0, 0), norm = v3(0, 0, 0);
            double u = 0, v = 0;
            if (h.node >= 0) {
                HitInfo info;
                finalize_hit<ST, false, true>(S, h, o, d, true, info);
                ip = info.ip; norm = info.norm; u = info.u; v = info.v;
            } else if (h.node <= -2) {
                light_record(S.lights[-2 - h.node], o, d, ip, norm);
            }
            double* const rec = KARG(QueryArgs, AP, hitRec) + 9 * (size_t)i;
            rec[0] = h.dist;
            rec[1] = ip.x; rec[2] = ip.y; rec[3] = ip.z;
            rec[4] = norm.x; rec[5] = norm.y; rec[6] = norm.z;
            rec[7] = u; rec[8] = v;
        }
    }
    if (ST & 1) flush_stats(A.st, c);
    if ((ST & 2) && c.envelope) atomicAdd(&A.st->rngOverflow, 1ull);
}

template <int ST>
static __global__ __launch_bounds__(256, query_visible_waves(ST)) void k_query_visible(QueryArgs A)
{
    Cnt c = zero_cnt();
    const int n = A.n, nItems = (n + 63) & ~63;
    DCursors* const cur = A.cur;
    for (int r = 0, i = claim_items(cur, nItems, r); i < nItems; i = claim_items(cur, nItems, r)) {
        if (i >= n) continue;
        const FRAY_RO QueryArgs* AP = kernel_args<QueryArgs>();
        const DScene& S = KARG(QueryArgs, AP, S);
        const double* const pa = KARG(QueryArgs, AP, a) + 3 * (size_t)i;
        const double* const pb = KARG(QueryArgs, AP, b) + 3 * (size_t)i;
        const V3 a = v3(pa[0], pa[1], pa[2]), b = v3(pb[0], pb[1], pb[2]);
        // a non-finite endpoint or a segment of length 0 (a == b) or of an overflowing length is visible, not traced
        const V3 e = b - a;
        const double ll = e.x * e.x + e.y * e.y + e.z * e.z;
        bool vis = true;
        if (finite3(a) && finite3(b) && ll > 0.0 && ll <= __DBL_MAX__) vis = visible<ST>(S, a, b, c);
        KARG(QueryArgs, AP, vis)[i] = vis ? 1 : 0;
    }
    if (ST & 1) flush_stats(A.st, c);
    if ((ST & 2) && c.envelope) atomicAdd(&A.st->rngOverflow, 1ull);
}

namespace frayhip_detail {
template <int ST> void launch_query_closest(hipStream_t stream, const QueryArgs& A)
{
    const int grid = persistent_grid((size_t)A.n, query_closest_waves(ST));
    if (A.hitRec) hipLaunchKernelGGL((k_query_closest<ST, true>), dim3(grid), dim3(256), 0, stream, A);
    else hipLaunchKernelGGL((k_query_closest<ST, false>), dim3(grid), dim3(256), 0, stream, A);
}
template <int ST> void launch_query_visible(hipStream_t stream, const QueryArgs& A)
{
    hipLaunchKernelGGL(k_query_visible<ST>, dim3(persistent_grid((size_t)A.n, query_visible_waves(ST))), dim3(256), 0, stream, A);
}
template void launch_query_closest<FRAY_ST>(hipStream_t, const QueryArgs&);
template void launch_query_visible<FRAY_ST>(hipStream_t, const QueryArgs&);
}  // namespace frayhip_detail
