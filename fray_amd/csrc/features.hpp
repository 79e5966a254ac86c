// Feature frames (include/frayhip.h: frayhip_render_features, frayhip_render_features_motion): what the C entry points (capi_features.hip) hand to
// the kernel of features_variant.hip, which the Makefile compiles once per kernel flag word as it does query_variant.hip.
#pragma once
#include "entry_support.hpp"

namespace frayhip_detail {

// What a node's transform was when the previous frame was rendered, as the motion frame carries a point back: {offset, m} of frayhip_transform
struct DPrevXform { double off[3]; double m[9]; };    // 96 B

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
    // the motion frame (k_features<ST, true> only; null otherwise)
    float* motion;                 // [H][W][FRAYHIP_MOTION_CHANNELS], device
    const DPrevXform* prev;        // [S.nNodes], read by the lanes whose hit node is moved
    const unsigned char* moved;    // [S.nNodes], 1: the node's transform differs from prev by bit pattern
};

// MOTION: the launch writes A.motion beside A.feat
template <int ST> void launch_features(hipStream_t stream, const FeatureArgs& A, bool motion);
FRAY_EXTERN_ST(void launch_features, (hipStream_t, const FeatureArgs&, bool))

}  // namespace frayhip_detail
