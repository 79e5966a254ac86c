// The ray queries (include/frayhip.h: frayhip_trace_rays, frayhip_visible): what the C entry points (capi_query.hip) hand to the kernels of
// query_variant.hip, which the Makefile compiles once per kernel flag word as it does render_variant.hip.
#pragma once
#include "entry_support.hpp"

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
FRAY_EXTERN_ST(void launch_query_closest, (hipStream_t, const QueryArgs&))
FRAY_EXTERN_ST(void launch_query_visible, (hipStream_t, const QueryArgs&))

}  // namespace frayhip_detail
