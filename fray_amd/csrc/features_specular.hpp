// Specular feature frames (include/frayhip.h: frayhip_render_features_specular): what the C entry points (capi_features.hip) hand to
// the kernel of features_specular_variant.hip, which the Makefile compiles once per kernel flag word as it does features_variant.hip.
#pragma once
#include "features.hpp"

namespace frayhip_detail {

// One launch over the frame's work items, as FeatureArgs; every camera sample followed through at most maxBounces Refl / Refr nodes
struct SpecularFeatureArgs {
    DScene S;
    DCamera C;
    DFrame F;
    int nItems;
    int n;
    int maxBounces;          // 1 .. FRAYHIP_SPECULAR_MAX_BOUNCES
    float* feat;             // [H][W][FRAYHIP_FEAT_CHANNELS], device
    float* bounces;          // [H][W], device, or null
    DStats* st;
    DCursors* cur;           // zeroed work cursors (claim_items)
};

template <int ST> void launch_features_specular(hipStream_t stream, const SpecularFeatureArgs& A);
FRAY_EXTERN_ST(void launch_features_specular, (hipStream_t, const SpecularFeatureArgs&))

}  // namespace frayhip_detail
