// Feature frames (include/frayhip.h: frayhip_render_features): what the C entry points (capi_features.hip) hand to the kernel of
// features_variant.hip, which the Makefile compiles once per kernel flag word as it does query_variant.hip.
#pragma once
#include "entry_support.hpp"

namespace frayhip_detail {

// One launch over the frame's work items (8x8 tiles of its buckets); n samples per pixel, averaged in sample order
struct FeatureArgs {
    DScene S;
    DCamera C;
    DFrame F;
    int nItems;
    int n;
    float* feat;             // [H][W][FRAYHIP_FEAT_CHANNELS], device
    DStats* st;
    DCursors* cur;           // zeroed work cursors (claim_items)
};

template <int ST> void launch_features(hipStream_t stream, const FeatureArgs& A);
FRAY_EXTERN_ST(void launch_features, (hipStream_t, const FeatureArgs&))

}  // namespace frayhip_detail
