// The ray queries (include/frayhip.h: frayhip_trace_rays, frayhip_visible): what the C entry points (capi_query.hip) hand to the kernels of
// query_variant.hip, which the Makefile compiles once per kernel flag word as it does render_variant.hip.
#pragma once
#include "render_state.hpp"

namespace frayhip_detail {

// One launch: n rays (origin a, direction b) or segments (a -> b), rows of three doubles.  Outputs may be null (hitRec null: no record).
struct QueryArgs {
    DScene S;
    int n;
    const double* a;
    const double* b;
    int32_t* hitId;
    double* hitDist;
    double* hitRec;          // [n][9]: dist, ip, norm, u, v
    uint8_t* vis;
    DStats* st;
    DCursors* cur;           // zeroed work cursors (claim_items)
};

template <int ST> void launch_query_closest(hipStream_t stream, const QueryArgs& A);
template <int ST> void launch_query_visible(hipStream_t stream, const QueryArgs& A);
#define FRAY_QUERY_EXTERN(st) extern template void launch_query_closest<st>(hipStream_t, const QueryArgs&); \
                              extern template void launch_query_visible<st>(hipStream_t, const QueryArgs&);
FRAY_QUERY_EXTERN(0) FRAY_QUERY_EXTERN(1) FRAY_QUERY_EXTERN(2) FRAY_QUERY_EXTERN(3)
FRAY_QUERY_EXTERN(4) FRAY_QUERY_EXTERN(5) FRAY_QUERY_EXTERN(8) FRAY_QUERY_EXTERN(9)
#undef FRAY_QUERY_EXTERN

}  // namespace frayhip_detail
