// Host-side state behind a frayhip_scene handle and the workspace / grid helpers shared by the translation
// units of the library (defined in capi.hip).  What sits between a C entry point and its kernels -- the kernel
// flag word and its dispatch, the frame's records, the counters -- is entry_support.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <vector>

#include "capi_common.h"
#include "dev_scene.hpp"
#include "dev_queues.hpp"

// A failing HIP call: the runtime's own text goes to frayhip_last_error(); the code tells allocation
// failures (FRAYHIP_E_NOMEM) and a missing device (FRAYHIP_E_NODEVICE) from everything else (FRAYHIP_E_HIP).
namespace frayhip_detail {
inline int hip_error_code(hipError_t e)
{
    switch (e) {
        case hipErrorOutOfMemory: return FRAYHIP_E_NOMEM;
        case hipErrorNoDevice: case hipErrorInvalidDevice: case hipErrorInsufficientDriver: case hipErrorNotInitialized: return FRAYHIP_E_NODEVICE;
        default: return FRAYHIP_E_HIP;
    }
}
}  // namespace frayhip_detail
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            frayhip_detail::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));         \
            return frayhip_detail::hip_error_code(e_);                                            \
        }                                                                                         \
    } while (0)

#ifndef FRAY_PT_BUDGET_MIB
#define FRAY_PT_BUDGET_MIB 24576   // default workspace budget of a path-traced / wavefront-Whitted frame (frayhip_scene_set_option "pt_budget_mib"): the headline frame then runs 8 batches of 8 spp on 4 lanes (338 B per path in flight)
#endif
#ifndef FRAY_SEED_TABLE_MIB
#define FRAY_SEED_TABLE_MIB 4096   // default cap of the seed table (frayhip_scene_set_option "seed_table_mib"): holds 1080p x 256 spp (2070 MiB: planes are whole 48 x 48 buckets)
#endif
#ifndef FRAY_PT_LANES
#define FRAY_PT_LANES 4   // headline frame / smallpt 64 spp, ms: 1 lane 150.0 / 136.3, 2 -> 136.9 / 126.5, 3 -> 135.8 / 125.1, 4 -> 135.8 / 123.8, 6 -> 135.2 / 123.9
#endif

// The x[397] seed table of a scene handle ("The seed table"): k_seed's words of every camera sample of a frame, kept across frames.
// Plane-major and unpadded, d[(size_t)s * nItems + item] for the absolute sample index s, so a batch (s0, cn) is the slice at d + (size_t)s0 * nItems
// in the layout the kernels index.  The key is what item_pixel and sample_seed read of DFrame; a plane is valid once its k_seed launch was enqueued.
struct SeedTable {
    uint32_t* d = nullptr;
    size_t bytes = 0;                 // allocated
    bool keyed = false;
    int32_t key[7] = {};              // W, H, BW, BH, bucketFirst, bucketStride, nBuckets
    uint32_t seed = 0;
    int nItems = 0;
    std::vector<unsigned char> valid; // per plane the allocation has room for under this key
    bool noGrow = false;              // an allocation for this key failed, or the workspace needed the memory: no further attempt until the key changes
    bool serving = false;             // the frame being rendered takes its seeds from the table
};

struct SceneEdit;                     // capi.hip: what frayhip_scene_update needs of the arena as built, and the fixed tables of the description to compare with

struct frayhip_scene {
    void* d_arena = nullptr;
    size_t arena_bytes = 0;
    SceneEdit* edit = nullptr;
    long long sceneUpdates = 0, sceneUpdateBytes = 0;   // frayhip_scene_update calls since creation and the bytes the last one uploaded (get_option "scene_updates", "scene_update_bytes")
    DScene S{};
    frayhip_camera camera{};
    frayhip_settings settings{};
    bool whittedNeedsRecursion = false;
    int specFanMax = 0;               // > 0: the largest numSamples of a glossy Refl shader, in a scene whose lights draw no random numbers (speculative glossy fans, dev_whitted.hpp)
    bool speculateFans = true;        // option "speculate_fans"
    bool lightDraws = false;          // some light draws random numbers when sampled (RectLight::getNthSample, lights.cpp:62-63)
    int lastWhittedPath = 0;          // the last Whitted frame: 0 = k_whitted (recursive shaders), 1 = shade / visible / gather launches, 2 = the fused k_wh_shade (get_option "whitted_path")
    int fusedWhittedMax = 4;          // scenes whose lights take at most this many samples per hit render Whitted frames with the one-kernel path (k_whitted) instead of shade / visible / gather launches (FRAYHIP_FUSED_WHITTED_MAX)
    int csgLanes = 1;                 // batches in flight for the Cube / CSG kernel variants (FRAYHIP_CSG_LANES; their scratch arenas are made one stream at a time, render_impl)
    unsigned warmMask = 0;            // kernel sets whose scratch arenas the lanes' streams already hold (render_impl: empty launches, one stream after the other)
    bool fpContract = false;          // option "fp_contract": path tracing past a sample's first closest hit on the kernels built with fused multiply-adds (render_contract.hip)
    long long lastContracted = 0;     // the last frame's launches of contracted kernels (frayhip_scene_get_option "contracted_launches")
    bool skipNullSegments = true;     // option "skip_null_segments": the timed path-tracing kernels queue no next-event segment whose contribution is +0 in every channel (dev_shade.hpp nee_prepare)
    bool segmentPlanes = true;        // option "segment_planes": k_pt_shadow skips, per wave, the eligible nodes whose triangles' planes no live segment crosses (dev_segcert.hpp)
    bool certifiedSegments = true;    // option "certified_segments": path_shade stores the term of a next-event segment proven unoccluded itself instead of queueing it (dev_trace.hpp segment_certified; needs segmentPlanes and DScene::segCertAll)
    bool tightGates = true;           // frayhip_scene_tight_gates: the producers test an eligible mesh's gate by its own triangles' box and a guard (dev_gatecert.hpp) instead of its reference box
    bool cameraSkip = true;           // frayhip_scene_camera_skip: a first-bounce wave leaves out the meshes all its camera rays provably miss (dev_trace.hpp camera_skip_nodes, dev_scene.hpp DCamSkip)
    bool shadeShortcuts = true;       // frayhip_scene_shade_shortcuts: the path tracer's timed kernels shade the hits of an all-untransformed flat-mesh scene without the transform and a stored normal, and axis-scaled lights by their diagonals (dev_shade.hpp finalize_hit, light_nth_sample; dev_trace.hpp light_intersect)
    bool cameraTiles = true;          // frayhip_scene_camera_tiles: the first bounce reads its tile's pixel origin and skipped nodes from a per-frame table (dev_camtile.hpp, kernels.hpp k_cam_tiles)
    long long lastCameraSkipped = 0, lastCameraWaves = 0;   // the last frame's (wave, node) pairs skipped that way, and the first-bounce wave iterations that evaluated the records (frayhip_scene_camera_skip)
    long long lastShadowCertified = 0;   // the last frame's next-event segments decided that way (frayhip_scene_get_option "shadow_segments_certified"); they are part of lastShadowSegments
    long long lastShadowNodesSkipped = 0;   // the last frame's sum over k_pt_shadow's wave iterations of the nodes skipped that way (frayhip_scene_get_option "shadow_nodes_skipped")
    long long lastShadowSegments = 0; // the last frame's next-event segments the timed kernels decided, shadow-queue entries over all its launches plus the certified ones (frayhip_scene_get_option "shadow_segments"; render_impl frames)
    long long lastFans[4] = {0, 0, 0, 0};   // the last frame's fans filed, children traced ahead, children looked up, fans given up part of the way (frayhip_scene_get_option)
    int lightSampleCount = 0;         // sum over lights of Light::getNumSamples(): segments a Lambert / Phong hit queues (wavefront Whitted)
    bool extGeometry = false;         // Cube / CSG nodes present
    bool textured = false;            // textures or a loaded environment map present: selects the <ST | 8> variants when neither bit 1 nor bit 2 is set
    bool kdMeshes = false;            // some mesh has a KD-tree: selects the <ST | 4> kernel variants (the others are compiled without the KD walk)
    // per-frame workspace, grown on demand and kept between frames
    void* d_work = nullptr;
    size_t work_bytes = 0;
    DStats* d_stats = nullptr;
    // frayhip_render_features_motion: the call's table of previous transforms and moved bytes, kept between calls and grown with the node count
    void* d_motionTab = nullptr;
    size_t motionTabBytes = 0;
    std::vector<unsigned char> motionTabHost;     // what the upload reads: lives as long as the stream may read it
    QMeta* d_qmeta = nullptr;         // [3] segment tables: ping-pong path queues + shadow queue
    hipEvent_t evA = nullptr, evB = nullptr;
    std::vector<hipEvent_t> evPool, evPoolShadow;
    // path tracing: batches of a frame run on FRAY_PT_LANES streams at once (lane 0 = the caller's stream)
    hipStream_t laneStream[FRAY_PT_LANES] = {};
    hipEvent_t evLaneStart = nullptr, evResolved[FRAY_PT_LANES] = {};
    // tunables (frayhip_scene_set_option; defaults from FRAYHIP_PT_LANES / FRAYHIP_PT_BUDGET_MIB in the environment)
    int ptLanes = FRAY_PT_LANES;
    size_t ptBudgetBytes = (size_t)FRAY_PT_BUDGET_MIB << 20;
    // what a frame plans with: ptBudgetBytes clamped to the device's free memory ONCE (scene creation, a change of the option) and halved when an
    // allocation fails all the same -- never re-derived per frame (other processes' allocations would move the batch size, and every growth of the
    // workspace is a hipFree + hipMalloc in the middle of a run).  0 = not computed yet.
    size_t ptBudgetEff = 0;
    // option "seed_table_mib": the cap of the seed table, 0 = off (every batch seeds into its own scratch words, as before the table)
    size_t seedTableCapBytes = (size_t)FRAY_SEED_TABLE_MIB << 20;
    SeedTable seedTab;
    int lastBatchLanes = 0;           // the last frame's batch lanes: the streams its batches ran on, as planned (get_option "batch_lanes"; 1 unless path-traced)
    long long lastSeedLaunches = 0, lastSeedReused = 0;   // the last frame's k_seed launches and planes taken from the table (get_option "seed_launches", "seed_planes_reused")
    bool rendering = false;           // a frame of this scene is being rendered: set by every render entry, so that a progress callback cannot render or change it
};

namespace frayhip_detail {

// d_stats: two DStats blocks, then (256-byte aligned) the work cursors; one memset clears all of it per frame
// ... and, in the gap before the cursors, one running total of shadow-queue entries per batch lane (k_scan adds each launch's total to its lane's word:
// the launches of a lane are ordered by its stream, so no atomic is needed); and after those, per batch lane, the nodes k_pt_shadow's waves skipped by the
// segment-plane certificate (one atomic per wave at the kernel's end); and after those, per batch lane, the next-event segments k_pt_bounce's waves certified
// instead of queueing (the same pattern); and after those, per batch lane, two words: the (wave, node) pairs the first bounce skipped by its miss records and the
// wave iterations that evaluated them (the same pattern)
constexpr size_t kSegTotalsOffset = 2 * sizeof(DStats);
constexpr size_t kSegSkippedOffset = kSegTotalsOffset + FRAY_PT_LANES * sizeof(unsigned long long);
constexpr size_t kSegCertifiedOffset = kSegSkippedOffset + FRAY_PT_LANES * sizeof(unsigned long long);
constexpr size_t kCamSkippedOffset = kSegCertifiedOffset + FRAY_PT_LANES * sizeof(unsigned long long);
constexpr size_t kCursorOffset = (kCamSkippedOffset + 2 * FRAY_PT_LANES * sizeof(unsigned long long) + 255) / 256 * 256;
constexpr size_t kStatsBytes = kCursorOffset + 3 * sizeof(DCursors);     // sets of tile cursors: a batch's closest-hit and any-hit kernels; the three passes of speculative Whitted

DCamera camera_begin_frame(const frayhip_camera& c, int W, int H);
int persistent_grid(size_t n, int wavesPerSimd);
size_t work_budget(frayhip_scene* sc);
enum { FRAYHIP_RETRY_SMALLER = 1 };      // internal: ensure_work_or_shrink halved the budget, plan the frame again
int ensure_work_or_shrink(frayhip_scene* sc, size_t bytes, bool canRetry);
int bounce_grid(size_t n, bool alone);
int grid_for(size_t n);
int seed_grid(size_t n);
int ensure_work(frayhip_scene* sc, size_t bytes);
// The seed table at the head of a frame of `spp` sample planes of `nItems` words: compares the key (a change invalidates every plane), grows the
// allocation, and sets seedTab.serving; a frame the table cannot serve (option off, over the cap, allocation failed) renders as without it.
void seed_table_begin(frayhip_scene* sc, const DFrame& F, int nItems, int spp);
void seed_table_invalidate(frayhip_scene* sc);
void seed_table_free(frayhip_scene* sc);

// A progressive frame's request (frayhip_render_progressive / frayhip_render_device_progressive): the caller's callback and preview interval;
// h_rgb is the host frame the host entry copies every preview (and the final frame) to before it calls back, nullptr for the device entry.
struct Progress {
    const frayhip_progressive* req;
    float* h_rgb;
};
// i-th event of a pool, created on first use; nullptr (and the error text set) when hipEventCreate fails
hipEvent_t pool_event(std::vector<hipEvent_t>& pool, size_t i);

}  // namespace frayhip_detail
