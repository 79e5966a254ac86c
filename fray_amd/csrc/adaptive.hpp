// Adaptive frames (include/frayhip.h: frayhip_render_adaptive): what the C entry points (capi_adaptive.hip) hand to adaptive_impl<ST> of
// adaptive_variant.hip, which the Makefile compiles once per kernel flag word as it does shade_variant.hip.
#pragma once
#include <algorithm>
#include <vector>

#include "entry_support.hpp"

namespace frayhip_detail {

// One call, already checked (gi on, mono, register generators): the frame's buckets, its sample count `spp`, the ladder of sample counts and
// the stop rule; outputs in device memory (spp / err may be null).  rungs and samples are filled in by adaptive_impl.
struct AdaptiveCall {
    int bucketFirst, bucketStride;
    uint32_t seed;
    int sppChunk;                 // > 0: the most samples per pixel in one batch
    bool stats;
    int spp, minSpp;
    double threshold, errFloor;
    float* rgb;
    int32_t* sppOut;
    float* errOut;
    int rungs = 0;
    uint64_t samples = 0;
};

// r_0 = floor(min_spp / 2), r_1 = min_spp, r_{j+1} = min(2 r_j, spp), ending at the first rung equal to spp
inline std::vector<int> adaptive_ladder(int minSpp, int spp)
{
    std::vector<int> r{minSpp / 2, minSpp};
    while (r.back() < spp) r.push_back((int)std::min<long long>(2ll * r.back(), spp));
    return r;
}

template <int ST> int adaptive_impl(frayhip_scene* sc, AdaptiveCall& q, hipStream_t stream, frayhip_stats* st);
FRAY_EXTERN_ST(int adaptive_impl, (frayhip_scene*, AdaptiveCall&, hipStream_t, frayhip_stats*))

}  // namespace frayhip_detail
