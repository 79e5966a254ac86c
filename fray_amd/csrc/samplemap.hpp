// Sample maps (include/frayhip.h: frayhip_render_samples_map): what the C entry points (capi_samplemap.hip) hand to samplemap_impl<ST> of
// samplemap_variant.hip, which the Makefile compiles once per kernel flag word as it does adaptive_variant.hip.
#pragma once
#include "entry_support.hpp"

namespace frayhip_detail {

constexpr int kMapMaxSamples = 1 << 24;          // (float)N is exact up to here (frayhip_render_samples' bound)

// One call, already checked but for the planes' values (gi on, mono, register generators): the frame's buckets and the five buffers in device
// memory (rgb / noise may be null).  samplemap_impl fills in the rest; badPlanes: its first kernel met a value the entry refuses, nothing was written.
// A component call (frayhip_render_components_map) has a second state: accum / rgb / noise are then the direct state's and the *Indirect ones the
// indirect state's (accumIndirect set, the two outputs optional); all three null is the single-state call, launch for launch.
struct SampleMapCall {
    int bucketFirst, bucketStride;
    uint32_t seed;
    int sppChunk;                 // > 0: the most samples per pixel in one batch
    bool stats;
    float* accum;
    int32_t* count;
    const int32_t* add;
    float* rgb;
    float* noise;
    float* accumIndirect = nullptr;
    float* rgbIndirect = nullptr;
    float* noiseIndirect = nullptr;
    uint64_t samples = 0;
    int countMin = 0, countMax = 0;
    bool badPlanes = false;
};

template <int ST> int samplemap_impl(frayhip_scene* sc, SampleMapCall& q, hipStream_t stream, frayhip_stats* st);
FRAY_EXTERN_ST(int samplemap_impl, (frayhip_scene*, SampleMapCall&, hipStream_t, frayhip_stats*))

}  // namespace frayhip_detail
