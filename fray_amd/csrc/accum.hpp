// Resumable frames (include/frayhip.h "resumable frames": frayhip_render_samples): what the C entry points of accum.hip hand to render_impl<ST>,
// and the launch wrappers of accum.hip's kernels, which render_impl<ST> calls in place of the frame's own resolves.  The kernels themselves are
// compiled once, in accum.o (-ffp-contract=off); nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_scene.hpp"
#include "dev_queues.hpp"

namespace frayhip_detail {

// The accumulation request of a call: render samples first .. first + count - 1 of the call's pixels into the caller's state.
//   accum   device, W*H rows of FRAYHIP_ACCUM_CHANNELS floats (sum.r, sum.g, sum.b, m2), 16-byte aligned; read only when first > 0
//   noise   device, W*H floats or nullptr (rgb is render_impl's d_rgb, which may be nullptr too)
//   done    out: the samples per pixel the state holds when the call returns (first + count, or fewer after a cancel)
// A component call (include/frayhip.h "component frames": frayhip_render_components) carries a second state: `accum` then takes the samples' direct
// light and `accum2` their indirect light, rgb1 / noise take the first state's outputs (render_impl's d_rgb is nullptr: no previews) and rgb2 /
// noise2 the second's.  accum2 == nullptr is an ordinary resumable call.
struct AccumCall {
    int first = 0, count = 1;
    float* accum = nullptr;
    float* noise = nullptr;
    int done = 0;
    float* accum2 = nullptr;
    float *rgb1 = nullptr, *rgb2 = nullptr, *noise2 = nullptr;
    const char* who = "frayhip_render_samples";
};

// The mono path tracer's resolve into the state: batch (s0, chunk), each sample's terms folded innermost first, the samples in sample order
void launch_acc_resolve_terms(int grid, hipStream_t stream, const DFrame& F, int nItems, int s0, int chunk, const TermBuf& TB, float* accum);
// The same into two states: a sample's term 0 into `direct`, the fold of its terms 1 .. n-1 into `indirect`
void launch_acc_resolve_terms_split(int grid, hipStream_t stream, const DFrame& F, int nItems, int s0, int chunk, const TermBuf& TB, float* direct, float* indirect);
// The same over per-sample colours (stereo: sampleRadR given, blended as k_pt_resolve blends)
void launch_acc_resolve(int grid, hipStream_t stream, const DFrame& F, const DCamera& C, float saturation, int nItems, int s0, int chunk,
                        const float* sampleRad, const float* sampleRadR, float* accum);
// maxTraceDepth < 0: `chunk` samples of +0 per pixel, and their count (times `eyes`) to st->samples
void launch_acc_black(int grid, hipStream_t stream, const DFrame& F, int nItems, int s0, int chunk, int eyes, float* accum, DStats* st);
// rgb (W*H*3) and noise (W*H) of the call's pixels from the state after n samples; either may be nullptr
void launch_acc_mean(int grid, hipStream_t stream, const DFrame& F, int nItems, int n, const float* accum, float* rgb, float* noise);

}  // namespace frayhip_detail
