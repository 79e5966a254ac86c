// The radiance queries (include/frayhip.h: frayhip_shade_rays): what the C entry points (capi_shade.hip) hand to shade_impl<ST> of
// shade_variant.hip, which the Makefile compiles once per kernel flag word as it does render_variant.hip and query_variant.hip.
#pragma once
#include "entry_support.hpp"

namespace frayhip_detail {

// One call, already checked: n rays (origin, direction: rows of three doubles, device memory), samples sample_first .. sample_first + spp - 1 of
// each, generator key keys[i] (device memory) or i, colour rgb[n][3] (device memory).
struct ShadeCall {
    int n;
    const double* org;
    const double* dir;
    const uint32_t* keys;
    uint32_t seed;
    int spp, sampleFirst, rngSkip;
    bool stats;
    float* rgb;
};

template <int ST> int shade_impl(frayhip_scene* sc, const ShadeCall& q, hipStream_t stream, frayhip_stats* st);
FRAY_EXTERN_ST(int shade_impl, (frayhip_scene*, const ShadeCall&, hipStream_t, frayhip_stats*))

}  // namespace frayhip_detail
