// C ABI, device side: scene upload, frame set-up (Camera::beginFrame), kernel launches, timing.
// Stands behind render() of the reference (src/main.cpp:373-405).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <functional>
#include <cstdlib>


#include "entry_support.hpp"
#include "dev_rng.hpp"
#include "dev_pack.hpp"
#include "scene_arena.hpp"

namespace {

using frayhip_detail::set_error;

void put3(double* o, const double* p) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
}  // namespace

namespace frayhip_detail {

// Camera::beginFrame, camera.cpp:34-57 (host, FP64; sin/cos/tan from the host libm like the reference).
void matmul3(const double* a, const double* b, double* c)
{
    for (int i = 0; i < 9; i++) c[i] = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++) c[i * 3 + j] += a[i * 3 + k] * b[k * 3 + j];
}
void rowmul(const double* v, const double* m, double* o)
{
    for (int j = 0; j < 3; j++) o[j] = v[0] * m[j] + v[1] * m[3 + j] + v[2] * m[6 + j];
}
DCamera camera_begin_frame(const frayhip_camera& c, int W, int H)
{
    const double PI = 3.141592653589793238;
    auto rad = [&](double a) { return a / 180.0 * PI; };
    DCamera f{};
    const double aspect = c.aspectRatio;
    const double bc[3] = {-aspect - 0.0, 1.0 - 0.0, 1.0 - 1.0};
    const double lenBC = sqrt(bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2]);
    const double m = tan(rad(c.fov / 2)) / lenBC;
    const double tl[3] = {-aspect * m, +m, 1}, tr[3] = {+aspect * m, +m, 1}, bl[3] = {-aspect * m, -m, 1};
    // rotationAroundZ / X / Y (matrix.cpp:29-62) take `sin(angle)` and `cos(angle)`; the reference's build (g++ -O2) merges the pair into ONE call of
    // glibc's sincos(), whose sine is not sin()'s in the last place for one angle in 700 (-7.93, -7.84, -19.99 degrees ...).  This file is compiled by
    // clang, which keeps two calls: ask for sincos() by name, so that the camera is the reference's whatever compiles it.
    double S, C;
    sincos(rad(c.roll), &S, &C);
    const double rz[9] = {C, -S, 0, S, C, 0, 0, 0, 1};
    sincos(rad(c.pitch), &S, &C);
    const double rx[9] = {1, 0, 0, 0, C, -S, 0, S, C};
    sincos(rad(c.yaw), &S, &C);
    const double ry[9] = {C, 0, S, 0, 1, 0, -S, 0, C};
    double t[9], rot[9];
    matmul3(rz, rx, t);
    matmul3(t, ry, rot);
    rowmul(tl, rot, f.topLeft);
    rowmul(tr, rot, f.topRight);
    rowmul(bl, rot, f.bottomLeft);
    const double ez[3] = {0, 0, 1}, ey[3] = {0, 1, 0}, ex[3] = {1, 0, 0};
    rowmul(ez, rot, f.frontDir);
    rowmul(ey, rot, f.upDir);
    rowmul(ex, rot, f.rightDir);
    put3(f.pos, c.pos);
    f.w = W; f.h = H;
    f.apertureSize = 1.0 / c.fNumber;
    f.focalPlaneDist = c.focalPlaneDist;
    f.stereoSeparation = c.stereoSeparation;
    memcpy(f.leftMask, c.leftMask, sizeof f.leftMask);
    memcpy(f.rightMask, c.rightMask, sizeof f.rightMask);
    f.dof = c.dof;
    return f;
}

// Grid of a persistent kernel (k_primary, k_whitted: waves claim tiles from DCursors): exactly the
// blocks that are resident at once -- a 256-thread block is one wave per SIMD, so `wavesPerSimd`
// blocks per compute unit.
int persistent_grid(size_t n, int wavesPerSimd)
{
    static int cus = 0;
    if (!cus) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
        else cus = 256;
    }
    size_t blocks = (n + 255) / 256, cap = (size_t)cus * wavesPerSimd;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

#ifndef FRAY_BOUNCE_BLOCKS
#define FRAY_BOUNCE_BLOCKS 2048
#endif
#ifndef FRAY_BOUNCE_PATHS_PER_BLOCK
#define FRAY_BOUNCE_PATHS_PER_BLOCK 8192
#endif
#ifndef FRAY_BOUNCE_BLOCKS_ALONE
#define FRAY_BOUNCE_BLOCKS_ALONE 8192
#endif
static_assert(FRAY_BOUNCE_BLOCKS * 4 <= FRAY_MAXSEG && FRAY_BOUNCE_BLOCKS_ALONE * 4 <= FRAY_MAXSEG, "every wave of the bounce / shadow grid owns one segment of the queue tables (QMeta)");
// Every wave of the bounce / shadow grid gets an equal share of the queue.  With four batches in flight the frame is fastest at 2 048 blocks (smaller shares add
// instructions, and the other lanes' blocks fill a launch's tail anyway: profiles/r04_experiments/README.md K).  The Cube / CSG variants run their batches one at a time
// (`alone`), where the tail is the chip standing empty: 8 192 blocks, csg_nested path traced 79.8 -> 67.4 ms.
// Beside other batches a block should get at least 8 192 paths (2 048 per wave): one rank's share of an 8-rank frame (5.7 M paths per batch) is fastest at 768-1 024 blocks
// (12.6-12.7 ms against 13.3 at 2 048, 15.9 at 4 096), a quarter frame at 1 024-1 536, the whole frame (16.6 M) at 2 048.
int bounce_grid(size_t n, bool alone)
{
    size_t blocks = (n + 255) / 256;
    const size_t cap = alone ? (size_t)FRAY_BOUNCE_BLOCKS_ALONE : std::min<size_t>(FRAY_BOUNCE_BLOCKS, std::max<size_t>(256, n / FRAY_BOUNCE_PATHS_PER_BLOCK));
    if (blocks > cap) blocks = cap;
    return (int)(blocks < 1 ? 1 : blocks);
}

int seed_grid(size_t n)          // k_seed: many short threads
{
    // forest DOF 256: 155.2 ms at 2 048 blocks, 153.6 at 32 768 (a thread runs few chains and the last waves leave together).  FRAYHIP_SEED_BLOCKS is a
    // development knob, read once per process and validated like the others: 1..65535, anything else keeps the default
    static const long cap = [] { const char* e = getenv("FRAYHIP_SEED_BLOCKS"); const long v = e ? atol(e) : 0; return v >= 1 && v <= 65535 ? v : 32768L; }();
    size_t blocks = (n + 255) / 256;
    if (blocks > (size_t)cap) blocks = (size_t)cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

int grid_for(size_t n)
{
    size_t blocks = (n + 255) / 256;
    const size_t cap = 256 * 8;   // 256 CUs x 8 blocks of 256 threads: the chip's full wave capacity
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

int ensure_work(frayhip_scene* sc, size_t bytes)
{
    if (sc->work_bytes >= bytes) return FRAYHIP_OK;
    if (sc->d_work) (void)hipFree(sc->d_work);
    sc->d_work = nullptr;
    sc->work_bytes = 0;
    if (hipMalloc(&sc->d_work, bytes) != hipSuccess) { set_error("frayhip_render: out of device memory for the work queues (" + std::to_string(bytes >> 20) + " MiB)"); return FRAYHIP_E_NOMEM; }
    sc->work_bytes = bytes;
    return FRAYHIP_OK;
}

// The queue budget a frame may plan with: the tunable (pt_budget_mib), but never more than four fifths of what the device could give when the
// clamp was taken (free memory plus the workspace this scene already holds) -- on a smaller or busy GPU, or with several ranks sharing one for a
// rehearsal, the frame is then cut into smaller batches instead of failing with E_NOMEM.  The clamp is taken ONCE (first use after scene creation
// or after a change of the option): asking hipMemGetInfo every frame made the batch size follow other processes' allocations, and every growth of
// the workspace is a hipFree + hipMalloc in the middle of a run.  Ranks that share a GPU all see the same free memory at the same moment and may
// each plan with four fifths of it: an allocation that fails all the same halves the budget and the frame is planned again (ensure_work_or_shrink).
size_t work_budget(frayhip_scene* sc)
{
    if (!sc->ptBudgetEff) {
        size_t freeB = 0, totalB = 0;
        size_t b = sc->ptBudgetBytes;
        // (the seed table's memory counts as free: the workspace takes it back when it has to, ensure_work_or_shrink)
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) b = std::min(b, (freeB + sc->work_bytes + sc->seedTab.bytes) / 5 * 4);
        sc->ptBudgetEff = std::max<size_t>(b, (size_t)64 << 20);
    }
    return sc->ptBudgetEff;
}

// ensure_work for a plan made under work_budget(): FRAYHIP_OK, an error, or FRAYHIP_RETRY_SMALLER after halving the budget (the caller plans again).
// `canRetry`: the caller will plan again with the smaller budget (it is not pinned by frayhip_frame.spp_chunk and is not already at one sample per
// batch); only then is the halved budget kept -- a failure the caller can do nothing about must not shrink every later frame's batches (it is
// reported as FRAYHIP_E_NOMEM and the budget stays; option "pt_budget_effective_mib" reads what frames currently plan with).
int ensure_work_or_shrink(frayhip_scene* sc, size_t bytes, bool canRetry)
{
    int rc = ensure_work(sc, bytes);
    if (rc != FRAYHIP_E_NOMEM) return rc;
    (void)hipGetLastError();
    // The seed table must never make a frame fail or shrink its batches: the workspace takes its memory back first.  A frame planned without
    // its per-batch seed words sees seedTab.serving cleared and plans again (render_impl).
    if (sc->seedTab.d) {
        seed_table_free(sc);
        sc->seedTab.noGrow = true;
        rc = ensure_work(sc, bytes);
        if (rc != FRAYHIP_E_NOMEM) return rc;
        (void)hipGetLastError();
    }
    if (!canRetry || work_budget(sc) <= ((size_t)64 << 20)) return rc;          // nothing to plan again, or already at the floor: give up with the allocation's message
    sc->ptBudgetEff = std::max<size_t>(sc->ptBudgetEff / 2, (size_t)64 << 20);
    return FRAYHIP_RETRY_SMALLER;
}

void seed_table_invalidate(frayhip_scene* sc)
{
    std::fill(sc->seedTab.valid.begin(), sc->seedTab.valid.end(), (unsigned char)0);
}

void seed_table_free(frayhip_scene* sc)
{
    SeedTable& T = sc->seedTab;
    if (T.d) (void)hipFree(T.d);
    T.d = nullptr;
    T.bytes = 0;
    T.valid.clear();
    T.serving = false;
}

// (render_impl has cleared seedTab.serving and the last frame's figures at its head.)
// Called at the head of a frame, when no earlier frame of this scene is in flight: every frame ends with its lanes joined into the caller's
// stream and that stream synchronised (or, on an error, the device), so the copy and the hipFree of a growth race with nothing.
void seed_table_begin(frayhip_scene* sc, const DFrame& F, int nItems, int spp)
{
    SeedTable& T = sc->seedTab;
    if (!sc->seedTableCapBytes) { seed_table_free(sc); T.keyed = false; return; }        // option off: nothing is held
    if (nItems <= 0 || spp <= 0) return;
    const int32_t key[7] = {F.W, F.H, F.BW, F.BH, F.bucketFirst, F.bucketStride, F.nBuckets};
    const size_t planeBytes = (size_t)nItems * sizeof(uint32_t);
    if (!T.keyed || memcmp(key, T.key, sizeof key) != 0 || F.seed != T.seed || nItems != T.nItems) {
        memcpy(T.key, key, sizeof key);
        T.seed = F.seed; T.nItems = nItems; T.keyed = true; T.noGrow = false;
        T.valid.assign(T.bytes / planeBytes, 0);          // the allocation is kept and cut into planes of the new size
    }
    const size_t need = (size_t)spp * planeBytes;
    if (need > sc->seedTableCapBytes) return;
    if (T.valid.size() < (size_t)spp) {
        if (T.noGrow) return;
        uint32_t* d = nullptr;
        if (hipMalloc((void**)&d, need) != hipSuccess) {
            // no room for the old and the new allocation at once: the frame renders from workspace words, and the old table, which frames of this
            // key can no longer use whole, is given back instead of being held for nothing
            (void)hipGetLastError();
            seed_table_free(sc);
            T.noGrow = true;
            return;
        }
        size_t held = 0;                                  // the planes up to the last valid one move to the new allocation
        for (size_t s = 0; s < T.valid.size(); s++) if (T.valid[s]) held = s + 1;
        if (held && hipMemcpy(d, T.d, held * planeBytes, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipGetLastError(); std::fill(T.valid.begin(), T.valid.end(), (unsigned char)0); }
        if (T.d) (void)hipFree(T.d);          // a device-to-device hipMemcpy may return before it is done: this hipFree synchronises the device, so the copy has completed before any stream reads the new table
        T.d = d;
        T.bytes = need;
        T.valid.resize((size_t)spp, 0);
    }
    T.serving = true;
}

hipEvent_t pool_event(std::vector<hipEvent_t>& pool, size_t i)
{
    while (pool.size() <= i) {
        hipEvent_t e = nullptr;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) { set_error(std::string("hipEventCreate: ") + hipGetErrorString(rc)); return nullptr; }
        pool.push_back(e);
    }
    return pool[i];
}

int bad(const char* who, const std::string& why)
{
    set_error(std::string(who) + ": " + why);
    return FRAYHIP_E_ARG;
}
int unsupported(const char* who, const std::string& why)
{
    set_error(std::string(who) + ": " + why);
    return FRAYHIP_E_UNSUPPORTED;
}

int frame_spp(const frayhip_scene* s)
{
    int spp = s->settings.wantAA ? 5 : 1;
    if (s->camera.dof) spp = std::max(spp, s->camera.numDOFSamples);
    if (s->settings.gi) spp = std::max(spp, s->settings.numPaths);
    return spp;
}

DScene frame_scene(const frayhip_scene* s)
{
    const frayhip_settings& set = s->settings;
    DScene S = s->S;
    S.ambient[0] = set.ambientLight[0]; S.ambient[1] = set.ambientLight[1]; S.ambient[2] = set.ambientLight[2];
    S.maxTraceDepth = set.maxTraceDepth;
    S.gi = set.gi;
    S.saturation = set.saturation;
    S.skipNullSegments = s->skipNullSegments ? 1 : 0;
    S.segmentPlanes = s->segmentPlanes ? 1 : 0;
    S.certifiedSegments = (s->certifiedSegments && s->segmentPlanes && S.segCertAll) ? 1 : 0;      // (no effect while "segment_planes" is 0)
    if (!s->cameraSkip) S.nCamSkip = 0;          // frayhip_scene_camera_skip switched off: no record, the first bounce asks every node
    if (!s->shadeShortcuts) S.shadeIdentity = S.lightsDiagonal = S.subdShift = 0;      // frayhip_scene_shade_shortcuts switched off: the kernels take the general forms
    return S;
}

DFrame frame_record(const frayhip_scene* s, int bucketFirst, int bucketStride, uint32_t seed)
{
    DFrame F = frame_grid(s->settings.frameWidth, s->settings.frameHeight);
    F.bucketStride = bucketStride > 0 ? bucketStride : 1;
    F.bucketFirst = bucketFirst;
    F.nBuckets = frayhip_bucket_count(F.W, F.H, F.bucketFirst, F.bucketStride);
    F.spp = frame_spp(s);
    F.seed = seed;
    F.jitter = (s->camera.dof || s->settings.gi) ? 1 : 0;
    return F;
}

int check_bucket_range(const char* who, int nBuckets) { return nBuckets < 0 ? bad(who, "bad bucket_first / bucket_stride") : FRAYHIP_OK; }
int check_pixel_cap(const char* who, int nBuckets)
{
    if ((long long)nBuckets * 2304 > (1ll << 30)) return unsupported(who, "more than 2^30 pixels in one call (shard the frame with bucket_first / bucket_stride)");
    return FRAYHIP_OK;
}
int refuse_stereo(const char* who, const frayhip_scene* s) { return s->camera.stereoSeparation > 0 ? unsupported(who, "stereo frames are not supported") : FRAYHIP_OK; }
int refuse_long_generators(const char* who, const frayhip_scene* s, const char* by)
{
    if (s->settings.gi && s->settings.maxTraceDepth >= 0 && long_generators(s->settings.maxTraceDepth))
        return unsupported(who, std::string("path tracing with maxTraceDepth >= 20 (generators past 227 words) is not supported by ") + by);
    return FRAYHIP_OK;
}

frayhip_stats finish_stats(frayhip_scene* sc, const DStats* blocks, int nBlocks, size_t nTraceEvents, size_t nShadowEvents, std::chrono::steady_clock::time_point t0)
{
    frayhip_stats o{};
    for (int k = 0; k < nBlocks; k++) {
        const DStats& d = blocks[k];
        o.closest_rays += d.closest; o.shadow_rays += d.shadow; o.node_tests += d.node; o.kd_inner_visits += d.kdInner; o.leaf_refs += d.leafRefs;
        o.tri_tests += d.tri; o.prim_tests += d.prim; o.smooth_hits += d.smooth; o.samples += d.samples; o.texture_fetches += d.tex;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, sc->evA, sc->evB);
    o.ms_kernels = ms;
    auto sumEvents = [](const std::vector<hipEvent_t>& pool, size_t n) {
        double t = 0;
        for (size_t i = 0; i + 1 < n; i += 2) {
            float m2 = 0;
            (void)hipEventElapsedTime(&m2, pool[i], pool[i + 1]);
            t += m2;
        }
        return t;
    };
    o.ms_trace = sumEvents(sc->evPool, nTraceEvents);
    o.trace_launches = nTraceEvents / 2;
    o.ms_shadow = sumEvents(sc->evPoolShadow, nShadowEvents);
    o.shadow_launches = nShadowEvents / 2;
    o.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return o;
}

}  // namespace frayhip_detail

// What frayhip_scene_update needs of a scene after its description is gone (include/frayhip.h "scene edits").  Of the arena as built: the table
// list, the facts, and a host copy of the tables arena_update writes or reads -- the editable tables, the DMesh table and the triangle records of the
// meshes whose triangles the segment-plane tables and the tight gate records are made from (detail::arena_keeps_tris: tree-less, a few dozen triangles at most) -- packed back
// to back: nothing whose size grows with a large mesh or with the texel pool.  Of the description: its fixed part, to compare an update's with.
struct SceneEdit {
    frayhip_arena::ArenaFacts F;
    std::vector<frayhip_arena::ArenaTable> tables;
    std::vector<frayhip_arena::ArenaMeshTables> meshTables;
    std::vector<int64_t> texelOffset;
    std::vector<unsigned char> host;
    std::vector<int64_t> hostOff;             // per table: where it starts in `host`, -1 for a table that is not kept
    int32_t counts[11];
    int64_t nTexels;
    std::vector<frayhip_geom_ref> geoms;
    std::vector<frayhip_csg> csgs;
    std::vector<frayhip_mesh> meshes;         // header scalars; the array pointers are never read
    std::vector<frayhip_texture> textures;    // kind, width, height, texel_offset
    frayhip_environment environment;
};

namespace frayhip_detail {
const DNode* host_nodes(const frayhip_scene* s) { return (const DNode*)(s->edit->host.data() + s->edit->hostOff[s->edit->F.tNodes]); }
const DShader* host_shaders(const frayhip_scene* s) { return (const DShader*)(s->edit->host.data() + s->edit->hostOff[s->edit->F.tShaders]); }
}  // namespace frayhip_detail

namespace {

using frayhip_detail::kStatsBytes;
using frayhip_detail::grid_for;

bool create_lanes(frayhip_scene* sc)
{
    if (hipEventCreateWithFlags(&sc->evLaneStart, hipEventDisableTiming) != hipSuccess) return false;
    for (int k = 0; k < FRAY_PT_LANES; k++) {
        if (k > 0 && hipStreamCreateWithFlags(&sc->laneStream[k], hipStreamNonBlocking) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&sc->evResolved[k], hipEventDisableTiming) != hipSuccess) return false;
    }
    return true;
}

// The range checks of the EDITABLE part of a description (include/frayhip.h, frayhip_scene_update): layers, shaders, nodes and lights against the
// element counts.  One copy, for frayhip_scene_create (inside validate_desc) and for frayhip_scene_update.
std::string validate_editable(const frayhip_scene_desc& d, const char* who)
{
    auto bad = [](const char* who, const char* what, long long i) { return std::string(who) + ": " + what + " (element " + std::to_string(i) + ")"; };
    for (int i = 0; i < d.n_layers; i++) {
        const frayhip_layer& L = d.layers[i];
        if (L.shader < 0 || L.shader >= d.n_shaders || L.texture < -1 || L.texture >= d.n_textures) return bad(who, "layer reference out of range", i);
    }
    for (int i = 0; i < d.n_shaders; i++) {
        const frayhip_shader& sh = d.shaders[i];
        if (sh.kind < 0 || sh.kind > 5) return bad(who, "unknown shader kind", i);
        if (sh.texture < -1 || sh.texture >= d.n_textures) return bad(who, "shader texture out of range", i);
        if (sh.kind == FRAYHIP_SHADER_LAYERED && (sh.layer_begin < 0 || sh.layer_count < 0 || (int64_t)sh.layer_begin + sh.layer_count > d.n_layers)) return bad(who, "layer range out of bounds", i);
        if (sh.kind == FRAYHIP_SHADER_REFL && sh.numSamples < 0) return bad(who, "negative numSamples", i);
    }
    for (int i = 0; i < d.n_nodes; i++) {
        const frayhip_node& n = d.nodes[i];
        if (n.geom < 0 || n.geom >= d.n_geoms || n.shader < 0 || n.shader >= d.n_shaders || n.bump_tex < -1 || n.bump_tex >= d.n_textures) return bad(who, "node reference out of range", i);
    }
    for (int i = 0; i < d.n_lights; i++) {
        const frayhip_light& L = d.lights[i];
        if (L.kind < 0 || L.kind > 1) return bad(who, "unknown light kind", i);
        if (L.kind == FRAYHIP_LIGHT_RECT && (L.xSubd <= 0 || L.ySubd <= 0 || (int64_t)L.xSubd * L.ySubd > (1 << 20))) return bad(who, "bad RectLight subdivision", i);
    }
    return std::string();
}

// A description can come from any host, not only from frayhip_scene_parse: every
// index the kernels will follow is range-checked here, because an out-of-range one would be a wild
// device read.  Returns an empty string when the description is sound.
std::string validate_desc(const frayhip_scene_desc& d)
{
    auto bad = [](const char* what, long long i) { return std::string("frayhip_scene_create: ") + what + " (element " + std::to_string(i) + ")"; };
    const int32_t counts[] = {d.n_nodes, d.n_geoms, d.n_planes, d.n_spheres, d.n_cubes, d.n_csgs, d.n_meshes, d.n_shaders, d.n_layers, d.n_textures, d.n_lights};
    for (int32_t c : counts) if (c < 0) return "frayhip_scene_create: negative element count";
    if (d.n_texels < 0) return "frayhip_scene_create: negative texel count";
    const void* arrays[] = {d.nodes, d.geoms, d.planes, d.spheres, d.cubes, d.csgs, d.meshes, d.shaders, d.layers, d.textures, d.lights};
    for (int k = 0; k < 11; k++) if (counts[k] > 0 && !arrays[k]) return "frayhip_scene_create: null array with a non-zero count";
    if (d.n_texels > 0 && !d.texels) return "frayhip_scene_create: null texel pool";
    const int32_t perKind[5] = {d.n_planes, d.n_spheres, d.n_cubes, d.n_meshes, d.n_csgs};
    for (int i = 0; i < d.n_geoms; i++) {
        const frayhip_geom_ref& g = d.geoms[i];
        if (g.kind < 0 || g.kind > 4 || g.index < 0 || g.index >= perKind[g.kind]) return bad("geometry reference out of range", i);
    }
    for (int i = 0; i < d.n_csgs; i++) {
        const frayhip_csg& c = d.csgs[i];
        if (c.op < 0 || c.op > 2 || c.left < 0 || c.left >= d.n_geoms || c.right < 0 || c.right >= d.n_geoms) return bad("CSG operand out of range", i);
    }
    auto texel_range_ok = [&](int64_t off, int32_t w, int32_t h) {
        if (w < 0 || h < 0 || off < 0) return false;
        return off + (int64_t)w * h * 3 <= d.n_texels;
    };
    for (int i = 0; i < d.n_textures; i++) {
        const frayhip_texture& t = d.textures[i];
        if (t.kind < 0 || t.kind > 3) return bad("unknown texture kind", i);
        if ((t.kind == FRAYHIP_TEX_BITMAP || t.kind == FRAYHIP_TEX_BUMP) && (t.width <= 0 || t.height <= 0)) return bad("bitmap texture without texels", i);   // the lookup wraps modulo width / height
        if ((t.kind == FRAYHIP_TEX_BITMAP || t.kind == FRAYHIP_TEX_BUMP) && !texel_range_ok(t.texel_offset, t.width, t.height)) return bad("texture texels outside the pool", i);
    }
    {
        const std::string why = validate_editable(d, "frayhip_scene_create");
        if (!why.empty()) return why;
    }
    if (d.environment.present && d.environment.loaded)
        for (int f = 0; f < 6; f++)
            if (d.environment.width[f] <= 0 || d.environment.height[f] <= 0 || !texel_range_ok(d.environment.texel_offset[f], d.environment.width[f], d.environment.height[f]))
                return bad("environment face outside the texel pool", f);
    for (int i = 0; i < d.n_meshes; i++) {
        const frayhip_mesh& m = d.meshes[i];
        if (m.n_vertices < 0 || m.n_normals < 0 || m.n_uvs < 0 || m.n_triangles < 0 || m.n_kdnodes < 0 || m.n_trirefs < 0) return bad("negative mesh count", i);
        if ((m.n_vertices && !m.vertices) || (m.n_normals && !m.normals) || (m.n_uvs && !m.uvs) || (m.n_triangles && !m.triangles) ||
            (m.n_kdnodes && !m.kdnodes) || (m.n_trirefs && !m.trirefs)) return bad("null mesh array with a non-zero count", i);
        for (int t = 0; t < m.n_triangles; t++) {
            const frayhip_triangle& T = m.triangles[t];
            for (int k = 0; k < 3; k++) {
                if (T.v[k] < 0 || T.v[k] >= m.n_vertices) return bad("triangle vertex index out of range in mesh", i);
                if (m.n_normals > 0 && (T.n[k] < 0 || T.n[k] >= m.n_normals)) return bad("triangle normal index out of range in mesh", i);
                if (m.n_uvs > 0 && (T.t[k] < 0 || T.t[k] >= m.n_uvs)) return bad("triangle uv index out of range in mesh", i);
            }
        }
        if (m.has_kd) {
            if (m.n_kdnodes <= 0) return bad("has_kd without nodes in mesh", i);
            std::vector<int> depth((size_t)m.n_kdnodes, 0);
            for (int k = 0; k < m.n_kdnodes; k++) {
                const frayhip_kdnode& n = m.kdnodes[k];
                if (n.parent < -1 || n.parent >= k || (k == 0) != (n.parent == -1)) return bad("KD parent link is not a tree in mesh", i);
                // the walk's stack of pending children holds one entry per level (dev_trace.hpp); the reference's builder stops at 65 (constants.h:39)
                if (k > 0 && (depth[k] = depth[n.parent] + 1) >= FRAY_KD_MAX_DEPTH) return bad(("KD tree deeper than the walk's stack (" + std::to_string(FRAY_KD_MAX_DEPTH) + " levels) in mesh").c_str(), i);
                if (n.axis == 3) {
                    if (n.tri_begin < 0 || n.tri_count < 0 || (int64_t)n.tri_begin + n.tri_count > m.n_trirefs) return bad("KD leaf range out of bounds in mesh", i);
                } else if (n.axis >= 0 && n.axis <= 2) {
                    // children lie after their parent (pre-order) and point back to it: the stackless walk climbs through these links
                    if (n.child0 <= k || (int64_t)n.child0 + 1 >= m.n_kdnodes || m.kdnodes[n.child0].parent != k || m.kdnodes[n.child0 + 1].parent != k)
                        return bad("KD child link is not a tree in mesh", i);
                } else return bad("bad KD axis in mesh", i);
            }
            for (int r = 0; r < m.n_trirefs; r++) if (m.trirefs[r] < 0 || m.trirefs[r] >= m.n_triangles) return bad("KD triangle reference out of range in mesh", i);
        }
    }
    if (d.settings.frameWidth <= 0 || d.settings.frameHeight <= 0) return "frayhip_scene_create: bad frame size";
    return std::string();
}

void desc_counts(const frayhip_scene_desc& d, int32_t out[11])
{
    const int32_t counts[11] = {d.n_nodes, d.n_geoms, d.n_planes, d.n_spheres, d.n_cubes, d.n_csgs, d.n_meshes, d.n_shaders, d.n_layers, d.n_textures, d.n_lights};
    memcpy(out, counts, sizeof counts);
}

// frayhip_scene_create: keeps what an update needs.  B is the arena as uploaded (placed).
SceneEdit* make_scene_edit(const frayhip_scene_desc& d, const frayhip_arena::ArenaBuilt& B)
{
    SceneEdit* E = new SceneEdit();
    E->F = B.F; E->tables = B.tables; E->meshTables = B.meshTables; E->texelOffset = B.texelOffset;
    E->hostOff.assign(B.tables.size(), -1);
    std::vector<int32_t> keep = frayhip_arena::arena_editable_tables(B.F);
    keep.push_back(B.F.tMeshes);
    const DMesh* const meshes = (const DMesh*)(B.host.data() + B.tables[B.F.tMeshes].off);
    for (int mi = 0; mi < B.F.nMeshes; mi++)
        if (frayhip_arena::detail::arena_keeps_tris(meshes[mi])) keep.push_back(B.meshTables[mi].tris);
    size_t bytes = 0;
    for (int32_t t : keep) { E->hostOff[t] = (int64_t)bytes; bytes += (B.tables[t].bytes + 15) / 16 * 16; }
    E->host.resize(bytes);
    for (int32_t t : keep) if (B.tables[t].bytes) memcpy(E->host.data() + E->hostOff[t], B.host.data() + B.tables[t].off, B.tables[t].bytes);
    desc_counts(d, E->counts);
    E->nTexels = d.n_texels;
    E->geoms.assign(d.geoms, d.geoms + d.n_geoms);
    E->csgs.assign(d.csgs, d.csgs + d.n_csgs);
    E->meshes.assign(d.meshes, d.meshes + d.n_meshes);
    E->textures.assign(d.textures, d.textures + d.n_textures);
    E->environment = d.environment;
    return E;
}

// The fixed part of an update's description against the one the scene was created from; the name of the first table that differs, or nullptr.
const char* fixed_part_differs(const SceneEdit& E, const frayhip_scene_desc& d)
{
    int32_t counts[11];
    desc_counts(d, counts);
    if (memcmp(counts, E.counts, sizeof counts) != 0 || d.n_texels != E.nTexels) return "an element count";
    const void* arrays[] = {d.nodes, d.geoms, d.planes, d.spheres, d.cubes, d.csgs, d.meshes, d.shaders, d.layers, d.textures, d.lights};
    for (int k = 0; k < 11; k++) if (counts[k] > 0 && !arrays[k]) return "a null array with a non-zero count";
    for (int i = 0; i < d.n_geoms; i++) if (d.geoms[i].kind != E.geoms[i].kind || d.geoms[i].index != E.geoms[i].index) return "geoms[]";
    for (int i = 0; i < d.n_csgs; i++) if (d.csgs[i].op != E.csgs[i].op || d.csgs[i].left != E.csgs[i].left || d.csgs[i].right != E.csgs[i].right) return "csgs[]";
    for (int i = 0; i < d.n_meshes; i++) {
        const frayhip_mesh &a = d.meshes[i], &b = E.meshes[i];
        if (a.n_vertices != b.n_vertices || a.n_normals != b.n_normals || a.n_uvs != b.n_uvs || a.n_triangles != b.n_triangles || a.n_kdnodes != b.n_kdnodes ||
            a.n_trirefs != b.n_trirefs || a.faceted != b.faceted || a.backfaceCulling != b.backfaceCulling || a.has_kd != b.has_kd ||
            a.kd_max_depth != b.kd_max_depth || a.kd_depth_sum != b.kd_depth_sum ||
            memcmp(a.bbox_min, b.bbox_min, sizeof a.bbox_min) != 0 || memcmp(a.bbox_max, b.bbox_max, sizeof a.bbox_max) != 0) return "meshes[] (a mesh header)";
    }
    for (int i = 0; i < d.n_textures; i++) {
        const frayhip_texture &a = d.textures[i], &b = E.textures[i];
        if (a.kind != b.kind || a.width != b.width || a.height != b.height || a.texel_offset != b.texel_offset) return "textures[] (kind, width, height or texel_offset)";
    }
    const frayhip_environment &a = d.environment, &b = E.environment;
    if (a.present != b.present || a.loaded != b.loaded || memcmp(a.width, b.width, sizeof a.width) != 0 || memcmp(a.height, b.height, sizeof a.height) != 0 ||
        memcmp(a.texel_offset, b.texel_offset, sizeof a.texel_offset) != 0) return "environment";
    return nullptr;
}

// every field frayhip_scene_create and frayhip_scene_update take from the arena's facts
void commit_facts(frayhip_scene* sc, const frayhip_arena::ArenaFacts& F)
{
    sc->extGeometry = F.extGeometry != 0;
    sc->kdMeshes = F.kdMeshes != 0;
    sc->textured = F.textured != 0;
    sc->whittedNeedsRecursion = F.whittedNeedsRecursion != 0;
    sc->lightDraws = F.lightDraws != 0;
    sc->lightSampleCount = F.lightSampleCount;
    sc->specFanMax = F.specFanMax;
}

}  // namespace

extern "C" {

int frayhip_init(int device_id)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { set_error("frayhip_init: no HIP device available"); return FRAYHIP_E_NODEVICE; }
    if (device_id < 0 || device_id >= n) { set_error("frayhip_init: bad device id"); return FRAYHIP_E_ARG; }
    HIP_TRY(hipSetDevice(device_id));
    return FRAYHIP_OK;
}

int frayhip_scene_create(const frayhip_scene_desc* desc, frayhip_scene** out)
{
    if (!desc || !out) { set_error("frayhip_scene_create: null argument"); return FRAYHIP_E_ARG; }
    if (desc->abi_version != FRAYHIP_ABI_VERSION) { set_error("frayhip_scene_create: ABI version mismatch"); return FRAYHIP_E_ARG; }
    const frayhip_scene_desc& d = *desc;
    {
        const std::string why = validate_desc(d);
        if (!why.empty()) { set_error(why); return FRAYHIP_E_ARG; }
    }
    // ---- what the device path implements ----
    {   // CsgOp trees: the device unrolls the Geometry::intersect recursion FRAY_CSG_DEPTH levels deep
        std::vector<int> levels(d.n_csgs, 0);      // 0 = not computed yet
        std::function<int(int, int)> depth = [&](int i, int guard) -> int {
            if (guard > d.n_csgs) return 1 << 20;   // a cycle cannot come out of the parser, but a hand-made description could hold one
            if (levels[i]) return levels[i];
            int m = 1;
            for (int side = 0; side < 2; side++) {
                const frayhip_geom_ref& g = d.geoms[side == 0 ? d.csgs[i].left : d.csgs[i].right];
                if (g.kind == FRAYHIP_GEOM_CSG) m = std::max(m, 1 + depth(g.index, guard + 1));
            }
            return levels[i] = m;
        };
        for (int i = 0; i < d.n_csgs; i++)
            if (depth(i, 0) > FRAY_CSG_DEPTH) {
                set_error("frayhip_scene_create: CSG operands nested more than " + std::to_string(FRAY_CSG_DEPTH) + " levels deep are not implemented on the device path");
                return FRAYHIP_E_UNSUPPORTED;
            }
    }
    // the arena and the scene facts (scene_arena.hpp): built without a device, then placed at the device allocation's addresses and uploaded
    frayhip_arena::ArenaBuilt B;
    frayhip_arena::arena_build(d, B);
    frayhip_scene* sc = new frayhip_scene();
    commit_facts(sc, B.F);
    if (hipMalloc(&sc->d_arena, B.host.size() ? B.host.size() : 256) != hipSuccess) {
        set_error("frayhip_scene_create: hipMalloc failed (no device?)");
        delete sc;
        return FRAYHIP_E_NODEVICE;
    }
    {
        unsigned char* const base = (unsigned char*)sc->d_arena;
        std::vector<unsigned char*> stage(B.tables.size());
        std::vector<const unsigned char*> addr(B.tables.size());
        for (size_t t = 0; t < B.tables.size(); t++) { stage[t] = B.host.data() + B.tables[t].off; addr[t] = base + B.tables[t].off; }
        frayhip_arena::arena_place(B.F, B.meshTables.data(), B.texelOffset.data(), stage.data(), addr.data(), sc->S);
    }
    hipError_t e = hipMemcpy(sc->d_arena, B.host.data(), B.host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error(std::string("frayhip_scene_create: upload failed: ") + hipGetErrorString(e)); (void)hipFree(sc->d_arena); delete sc; return FRAYHIP_E_NODEVICE; }
    sc->arena_bytes = B.host.size();
    sc->edit = make_scene_edit(d, B);
    sc->camera = d.camera;
    sc->settings = d.settings;
    // [0] everything but k_pt_shadow, [1] k_pt_shadow
    if (hipMalloc((void**)&sc->d_stats, kStatsBytes) != hipSuccess || hipMalloc((void**)&sc->d_qmeta, 3 * FRAY_PT_LANES * sizeof(QMeta)) != hipSuccess ||
        hipEventCreate(&sc->evA) != hipSuccess || hipEventCreate(&sc->evB) != hipSuccess || !create_lanes(sc)) {
        set_error("frayhip_scene_create: could not allocate the per-scene device state");
        frayhip_scene_destroy(sc);
        return FRAYHIP_E_NOMEM;
    }
    // profiling aids: the same knobs as frayhip_scene_set_option, preset from the environment
    if (const char* e = getenv("FRAYHIP_PT_LANES")) { long v = atol(e); if (v >= 1 && v <= FRAY_PT_LANES) sc->ptLanes = (int)v; }
    if (const char* e = getenv("FRAYHIP_SPECULATE_FANS")) sc->speculateFans = atol(e) != 0;
    if (const char* e = getenv("FRAYHIP_FP_CONTRACT")) sc->fpContract = atol(e) == 1;
    if (const char* e = getenv("FRAYHIP_SKIP_NULL_SEGMENTS")) sc->skipNullSegments = atol(e) != 0;
    if (const char* e = getenv("FRAYHIP_SEGMENT_PLANES")) sc->segmentPlanes = atol(e) != 0;
    if (const char* e = getenv("FRAYHIP_CERTIFIED_SEGMENTS")) sc->certifiedSegments = atol(e) != 0;
    if (const char* e = getenv("FRAYHIP_TIGHT_GATES")) sc->tightGates = atol(e) != 0;
    if (const char* e = getenv("FRAYHIP_CAMERA_SKIP")) sc->cameraSkip = atol(e) != 0;
    if (const char* e = getenv("FRAYHIP_CAMERA_TILES")) sc->cameraTiles = atol(e) != 0;
    if (const char* e = getenv("FRAYHIP_SHADE_SHORTCUTS")) sc->shadeShortcuts = atol(e) != 0;
    if (const char* e = getenv("FRAYHIP_FUSED_WHITTED_MAX")) { long v = atol(e); if (v >= 0 && v <= 1024) sc->fusedWhittedMax = (int)v; }
    if (const char* e = getenv("FRAYHIP_CSG_LANES")) { long v = atol(e); if (v >= 1 && v <= FRAY_PT_LANES) sc->csgLanes = (int)v; }
    if (const char* e = getenv("FRAYHIP_SEED_TABLE_MIB")) { long v = atol(e); if (v >= 0 && v <= (1 << 20)) sc->seedTableCapBytes = (size_t)v << 20; }
    if (const char* e = getenv("FRAYHIP_PT_BUDGET_MIB")) { long v = atol(e); if (v >= 1 && v <= (1 << 20)) { sc->ptBudgetBytes = (size_t)v << 20; sc->ptBudgetEff = 0; } }
    *out = sc;
    return FRAYHIP_OK;
}

int frayhip_scene_get_option(frayhip_scene* s, const char* name, int64_t* value)
{
    if (!s || !name || !value) { set_error("frayhip_scene_get_option: null argument"); return FRAYHIP_E_ARG; }
    const std::string n(name);
    if (n == "pt_lanes") *value = s->ptLanes;
    else if (n == "pt_budget_mib") *value = (int64_t)(s->ptBudgetBytes >> 20);
    else if (n == "speculate_fans") *value = s->speculateFans ? 1 : 0;
    else if (n == "fp_contract") *value = s->fpContract ? 1 : 0;
    else if (n == "contracted_launches") *value = s->lastContracted;
    else if (n == "skip_null_segments") *value = s->skipNullSegments ? 1 : 0;
    else if (n == "shadow_segments") *value = s->lastShadowSegments;
    else if (n == "segment_planes") *value = s->segmentPlanes ? 1 : 0;
    else if (n == "segment_plane_nodes") *value = s->S.nSegNodes;
    else if (n == "certified_segments") *value = s->certifiedSegments ? 1 : 0;
    else if (n == "certified_segments_eligible") *value = s->S.segCertAll;
    else if (n == "shadow_segments_certified") *value = s->lastShadowCertified;
    else if (n == "shadow_nodes_skipped") *value = s->lastShadowNodesSkipped;
    else if (n == "seed_table_mib") *value = (int64_t)(s->seedTableCapBytes >> 20);
    else if (n == "seed_table_bytes") *value = (int64_t)s->seedTab.bytes;
    else if (n == "seed_launches") *value = s->lastSeedLaunches;
    else if (n == "seed_planes_reused") *value = s->lastSeedReused;
    else if (n == "batch_lanes") *value = s->lastBatchLanes;
    else if (n == "whitted_path") *value = s->lastWhittedPath;
    else if (n == "fused_whitted_max") *value = s->fusedWhittedMax;
    else if (n == "pt_budget_effective_mib") *value = (int64_t)(frayhip_detail::work_budget(s) >> 20);
    else if (n == "scene_updates") *value = s->sceneUpdates;
    else if (n == "scene_update_bytes") *value = s->sceneUpdateBytes;
    else if (n == "arena_bytes") *value = (int64_t)s->arena_bytes;
    else if (n == "fans_filed") *value = s->lastFans[0];
    else if (n == "fan_children") *value = s->lastFans[1];
    else if (n == "fan_children_looked_up") *value = s->lastFans[2];
    else if (n == "fans_given_up") *value = s->lastFans[3];
    else { set_error("frayhip_scene_get_option: unknown option " + n); return FRAYHIP_E_ARG; }
    return FRAYHIP_OK;
}

int frayhip_scene_set_option(frayhip_scene* s, const char* name, int64_t value)
{
    if (!s || !name) { set_error("frayhip_scene_set_option: null argument"); return FRAYHIP_E_ARG; }
    if (s->rendering) { set_error("frayhip_scene_set_option: the scene is rendering a frame"); return FRAYHIP_E_ARG; }
    const std::string n(name);
    if (n == "pt_lanes") {
        if (value < 1 || value > FRAY_PT_LANES) { set_error("frayhip_scene_set_option: pt_lanes must be 1.." + std::to_string(FRAY_PT_LANES)); return FRAYHIP_E_ARG; }
        s->ptLanes = (int)value;
    } else if (n == "pt_budget_mib") {
        if (value < 1 || value > (1 << 20)) { set_error("frayhip_scene_set_option: pt_budget_mib must be 1..1048576"); return FRAYHIP_E_ARG; }
        s->ptBudgetBytes = (size_t)value << 20;
        s->ptBudgetEff = 0;                 // clamp again at the next frame
    } else if (n == "speculate_fans") {
        if (value != 0 && value != 1) { set_error("frayhip_scene_set_option: speculate_fans must be 0 or 1"); return FRAYHIP_E_ARG; }
        s->speculateFans = value != 0;
    } else if (n == "fused_whitted_max") {
        if (value < 0 || value > 1024) { set_error("frayhip_scene_set_option: fused_whitted_max must be 0..1024"); return FRAYHIP_E_ARG; }
        s->fusedWhittedMax = (int)value;
    } else if (n == "fp_contract") {
        if (value != 0 && value != 1) { set_error("frayhip_scene_set_option: fp_contract must be 0 or 1"); return FRAYHIP_E_ARG; }
        s->fpContract = value != 0;
    } else if (n == "seed_table_mib") {
        if (value < 0 || value > (1 << 20)) { set_error("frayhip_scene_set_option: seed_table_mib must be 0..1048576"); return FRAYHIP_E_ARG; }
        s->seedTableCapBytes = (size_t)value << 20;
        if (s->seedTab.bytes > s->seedTableCapBytes) { frayhip_detail::seed_table_free(s); s->seedTab.keyed = false; }      // a table over the new cap is given back now
    } else if (n == "skip_null_segments") {
        if (value != 0 && value != 1) { set_error("frayhip_scene_set_option: skip_null_segments must be 0 or 1"); return FRAYHIP_E_ARG; }
        s->skipNullSegments = value != 0;
    } else if (n == "segment_planes") {
        if (value != 0 && value != 1) { set_error("frayhip_scene_set_option: segment_planes must be 0 or 1"); return FRAYHIP_E_ARG; }
        s->segmentPlanes = value != 0;
    } else if (n == "certified_segments") {
        if (value != 0 && value != 1) { set_error("frayhip_scene_set_option: certified_segments must be 0 or 1"); return FRAYHIP_E_ARG; }
        s->certifiedSegments = value != 0;
    } else {
        set_error("frayhip_scene_set_option: unknown option " + n);
        return FRAYHIP_E_ARG;
    }
    return FRAYHIP_OK;
}

int frayhip_scene_tight_gates(frayhip_scene* s, int enable, int64_t* enabled, int64_t* eligible)
{
    if (!s) { set_error("frayhip_scene_tight_gates: null scene"); return FRAYHIP_E_ARG; }
    if (enable < -1 || enable > 1) { set_error("frayhip_scene_tight_gates: enable must be -1, 0 or 1"); return FRAYHIP_E_ARG; }
    if (enable >= 0 && s->rendering) { set_error("frayhip_scene_tight_gates: the scene is rendering a frame"); return FRAYHIP_E_ARG; }
    if (enable >= 0) s->tightGates = enable != 0;
    if (enabled) *enabled = s->tightGates ? 1 : 0;
    if (eligible) *eligible = s->edit->F.nTightGates;
    return FRAYHIP_OK;
}

int frayhip_scene_camera_skip(frayhip_scene* s, int enable, int64_t* enabled, int64_t* eligible, int64_t* skipped, int64_t* waves)
{
    if (!s) { set_error("frayhip_scene_camera_skip: null scene"); return FRAYHIP_E_ARG; }
    if (enable < -1 || enable > 1) { set_error("frayhip_scene_camera_skip: enable must be -1, 0 or 1"); return FRAYHIP_E_ARG; }
    if (enable >= 0 && s->rendering) { set_error("frayhip_scene_camera_skip: the scene is rendering a frame"); return FRAYHIP_E_ARG; }
    if (enable >= 0) s->cameraSkip = enable != 0;
    if (enabled) *enabled = s->cameraSkip ? 1 : 0;
    if (eligible) *eligible = s->edit->F.nCamSkip;
    if (skipped) *skipped = s->lastCameraSkipped;
    if (waves) *waves = s->lastCameraWaves;
    return FRAYHIP_OK;
}

int frayhip_scene_camera_tiles(frayhip_scene* s, int enable, int64_t* enabled)
{
    if (!s) { set_error("frayhip_scene_camera_tiles: null scene"); return FRAYHIP_E_ARG; }
    if (enable < -1 || enable > 1) { set_error("frayhip_scene_camera_tiles: enable must be -1, 0 or 1"); return FRAYHIP_E_ARG; }
    if (enable >= 0 && s->rendering) { set_error("frayhip_scene_camera_tiles: the scene is rendering a frame"); return FRAYHIP_E_ARG; }
    if (enable >= 0) s->cameraTiles = enable != 0;
    if (enabled) *enabled = s->cameraTiles ? 1 : 0;
    return FRAYHIP_OK;
}

int frayhip_scene_shade_shortcuts(frayhip_scene* s, int enable, int64_t* enabled, int64_t* eligible)
{
    if (!s) { set_error("frayhip_scene_shade_shortcuts: null scene"); return FRAYHIP_E_ARG; }
    if (enable < -1 || enable > 1) { set_error("frayhip_scene_shade_shortcuts: enable must be -1, 0 or 1"); return FRAYHIP_E_ARG; }
    if (enable >= 0 && s->rendering) { set_error("frayhip_scene_shade_shortcuts: the scene is rendering a frame"); return FRAYHIP_E_ARG; }
    if (enable >= 0) s->shadeShortcuts = enable != 0;
    if (enabled) *enabled = s->shadeShortcuts ? 1 : 0;
    if (eligible) *eligible = (s->edit->F.shadeIdentity ? 1 : 0) | (s->edit->F.lightsDiagonal ? 2 : 0);
    return FRAYHIP_OK;
}

int frayhip_scene_set_view(frayhip_scene* s, const frayhip_camera* camera, const frayhip_settings* settings)
{
    if (!s) { set_error("frayhip_scene_set_view: null scene"); return FRAYHIP_E_ARG; }
    if (s->rendering) { set_error("frayhip_scene_set_view: the scene is rendering a frame"); return FRAYHIP_E_ARG; }
    if (settings && (settings->frameWidth <= 0 || settings->frameHeight <= 0)) { set_error("frayhip_scene_set_view: bad frame size"); return FRAYHIP_E_ARG; }
    if (camera) s->camera = *camera;
    if (settings) s->settings = *settings;
    return FRAYHIP_OK;
}

int frayhip_scene_update(frayhip_scene* s, const frayhip_scene_desc* desc)
{
    if (!s || !desc) { set_error("frayhip_scene_update: null argument"); return FRAYHIP_E_ARG; }
    if (s->rendering) { set_error("frayhip_scene_update: the scene is rendering a frame"); return FRAYHIP_E_ARG; }
    if (desc->abi_version != FRAYHIP_ABI_VERSION) { set_error("frayhip_scene_update: ABI version mismatch"); return FRAYHIP_E_ARG; }
    const frayhip_scene_desc& d = *desc;
    SceneEdit& E = *s->edit;
    if (const char* what = fixed_part_differs(E, d)) {
        set_error(std::string("frayhip_scene_update: ") + what + " differs from the description the scene was created from (only nodes, primitives, shaders, layers, lights and texture parameters can be edited)");
        return FRAYHIP_E_ARG;
    }
    {
        const std::string why = validate_editable(d, "frayhip_scene_update");
        if (!why.empty()) { set_error(why); return FRAYHIP_E_ARG; }
    }
    // the new tables, built beside the kept ones: nothing of the handle changes before the upload
    std::vector<unsigned char> next(E.host);
    frayhip_arena::ArenaFacts F = E.F;
    std::vector<unsigned char*> tab(E.tables.size());
    std::vector<const unsigned char*> addr(E.tables.size());
    for (size_t t = 0; t < E.tables.size(); t++) {
        tab[t] = E.hostOff[t] >= 0 ? next.data() + E.hostOff[t] : nullptr;
        addr[t] = (const unsigned char*)s->d_arena + E.tables[t].off;
    }
    frayhip_arena::arena_update(d, E.meshTables.data(), F, tab.data());
    DScene S = s->S;
    frayhip_arena::arena_place(F, E.meshTables.data(), E.texelOffset.data(), tab.data(), addr.data(), S);
    long long bytes = 0;
    for (int32_t t : frayhip_arena::arena_editable_tables(F)) {
        if (!E.tables[t].bytes) continue;
        HIP_TRY(hipMemcpy((unsigned char*)s->d_arena + E.tables[t].off, tab[t], E.tables[t].bytes, hipMemcpyHostToDevice));
        bytes += (long long)E.tables[t].bytes;
    }
    E.host.swap(next);
    E.F = F;
    commit_facts(s, F);
    s->S = S;
    s->sceneUpdates++;
    s->sceneUpdateBytes = bytes;
    return FRAYHIP_OK;
}

void frayhip_scene_destroy(frayhip_scene* s)
{
    if (!s) return;
    delete s->edit;
    if (s->d_arena) (void)hipFree(s->d_arena);
    if (s->d_work) (void)hipFree(s->d_work);
    frayhip_detail::seed_table_free(s);
    if (s->d_stats) (void)hipFree(s->d_stats);
    if (s->d_motionTab) (void)hipFree(s->d_motionTab);
    if (s->d_qmeta) (void)hipFree(s->d_qmeta);
    if (s->evA) (void)hipEventDestroy(s->evA);
    if (s->evB) (void)hipEventDestroy(s->evB);
    if (s->evLaneStart) (void)hipEventDestroy(s->evLaneStart);
    for (int k = 0; k < FRAY_PT_LANES; k++) {
        if (s->evResolved[k]) (void)hipEventDestroy(s->evResolved[k]);
        if (s->laneStream[k]) (void)hipStreamDestroy(s->laneStream[k]);
    }
    for (auto e : s->evPool) (void)hipEventDestroy(e);
    for (auto e : s->evPoolShadow) (void)hipEventDestroy(e);
    delete s;
}


namespace {
// Every render entry: the kernel flag word the scene needs, and the per-scene `rendering` flag that turns a render, a change or a destruction of the
// scene from inside a progress callback into FRAYHIP_E_ARG.
int render_dispatch(frayhip_scene* s, const frayhip_frame* f, float* d_rgb, int32_t* d_hit_id, double* d_hit_dist, hipStream_t stream, frayhip_stats* st,
                    const frayhip_detail::Progress* prog)
{
    if (s->rendering) { set_error("frayhip_render: the scene is already rendering a frame (a render call from inside a progress callback?)"); return FRAYHIP_E_ARG; }
    frayhip_detail::Busy busy(s, stream, false);          // render_impl drains its lanes itself on an early return
    return frayhip_detail::for_flag_word(frayhip_detail::flag_word(s, (f->flags & FRAYHIP_FRAME_STATS) != 0), [&](auto w) {
        return frayhip_detail::render_impl<decltype(w)::value>(s, f, d_rgb, d_hit_id, d_hit_dist, stream, st, prog, nullptr);
    });
}

int check_progressive(const frayhip_progressive* p, const char* who)
{
    if (!p) { set_error(std::string(who) + ": null progress request"); return FRAYHIP_E_ARG; }
    if (std::isnan(p->preview_ms)) { set_error(std::string(who) + ": preview_ms is NaN"); return FRAYHIP_E_ARG; }
    return FRAYHIP_OK;
}

// The host entries: device buffers for the call, the caller's frame uploaded first when the call renders a subset of the buckets, the results
// copied back.  A progressive frame's rgb is already on the host (render_impl copies it before the final callback), also when it was cancelled.
int render_host(frayhip_scene* s, const frayhip_frame* f, const frayhip_progressive* p, float* rgb, int32_t* hit_id, double* hit_dist, frayhip_stats* st)
{
    const size_t n = (size_t)s->settings.frameWidth * s->settings.frameHeight;
    frayhip_detail::DeviceArrays B("frayhip_render: hipMalloc failed");
    float* d_rgb; int32_t* d_id; double* d_dist;
    if (int rc = B.alloc(d_rgb, 3 * n, rgb != nullptr)) return rc;
    if (int rc = B.alloc(d_id, n, hit_id != nullptr)) return rc;
    if (int rc = B.alloc(d_dist, n, hit_dist != nullptr)) return rc;
    // pixels outside this call's buckets keep what the caller had in the buffers: only a call that renders a SUBSET of the
    // buckets needs the caller's frame on the device first; a whole-frame call overwrites every pixel
    hipError_t ce = hipSuccess;
    const bool subset = f->bucket_stride > 1 || f->bucket_first != 0;
    if (subset) {
        if (d_rgb && ce == hipSuccess) ce = hipMemcpy(d_rgb, rgb, n * 12, hipMemcpyHostToDevice);
        if (d_id && ce == hipSuccess) ce = hipMemcpy(d_id, hit_id, n * 4, hipMemcpyHostToDevice);
        if (d_dist && ce == hipSuccess) ce = hipMemcpy(d_dist, hit_dist, n * 8, hipMemcpyHostToDevice);
    }
    if (ce != hipSuccess) { set_error(std::string("frayhip_render: host-to-device copy failed: ") + hipGetErrorString(ce)); return frayhip_detail::hip_error_code(ce); }
    const frayhip_detail::Progress prog{p, rgb};
    int rc = render_dispatch(s, f, d_rgb, d_id, d_dist, nullptr, st, p ? &prog : nullptr);
    if (!rc || rc == FRAYHIP_E_CANCELLED) {
        if (d_rgb && !p && ce == hipSuccess) ce = hipMemcpy(rgb, d_rgb, n * 12, hipMemcpyDeviceToHost);
        if (d_id && ce == hipSuccess) ce = hipMemcpy(hit_id, d_id, n * 4, hipMemcpyDeviceToHost);
        if (d_dist && ce == hipSuccess) ce = hipMemcpy(hit_dist, d_dist, n * 8, hipMemcpyDeviceToHost);
        if (ce != hipSuccess) { set_error(std::string("frayhip_render: device-to-host copy failed: ") + hipGetErrorString(ce)); rc = frayhip_detail::hip_error_code(ce); }
    }
    return rc;
}
}  // namespace

int frayhip_render_device(frayhip_scene* s, const frayhip_frame* f, float* d_rgb, int32_t* d_hit_id, double* d_hit_dist, void* hip_stream,
                          frayhip_stats* st)
{
    if (!s || !f) { set_error("frayhip_render_device: null argument"); return FRAYHIP_E_ARG; }
    return render_dispatch(s, f, d_rgb, d_hit_id, d_hit_dist, (hipStream_t)hip_stream, st, nullptr);
}

int frayhip_render(frayhip_scene* s, const frayhip_frame* f, float* rgb, int32_t* hit_id, double* hit_dist, frayhip_stats* st)
{
    if (!s || !f) { set_error("frayhip_render: null argument"); return FRAYHIP_E_ARG; }
    return render_host(s, f, nullptr, rgb, hit_id, hit_dist, st);
}

int frayhip_render_device_progressive(frayhip_scene* s, const frayhip_frame* f, const frayhip_progressive* p, float* d_rgb, int32_t* d_hit_id,
                                      double* d_hit_dist, void* hip_stream, frayhip_stats* st)
{
    if (const int rc = check_progressive(p, "frayhip_render_device_progressive")) return rc;
    if (!s || !f) { set_error("frayhip_render_device_progressive: null argument"); return FRAYHIP_E_ARG; }
    const frayhip_detail::Progress prog{p, nullptr};
    return render_dispatch(s, f, d_rgb, d_hit_id, d_hit_dist, (hipStream_t)hip_stream, st, &prog);
}

int frayhip_render_progressive(frayhip_scene* s, const frayhip_frame* f, const frayhip_progressive* p, float* rgb, int32_t* hit_id, double* hit_dist,
                               frayhip_stats* st)
{
    if (const int rc = check_progressive(p, "frayhip_render_progressive")) return rc;
    if (!s || !f) { set_error("frayhip_render_progressive: null argument"); return FRAYHIP_E_ARG; }
    return render_host(s, f, p, rgb, hit_id, hit_dist, st);
}

__global__ void k_debug_rng(uint32_t seed, int n, float* f, double* d, int32_t* it, int hi, uint32_t* work)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    MtLong g[3];
    for (int k = 0; k < 3; k++) { g[k].st = work + k; g[k].stride = 3; g[k].reseed(seed); }
    for (int i = 0; i < n; i++) {
        f[i] = rng_float(g[0]);
        d[i] = rng_double(g[1]);
        it[i] = rng_int0(g[2], hi);
    }
}

int frayhip_debug_rng(uint32_t seed, int n, float* floats, double* doubles, int32_t* ints, int int_hi)
{
    if (n < 0 || n > 4096 || int_hi < 0) { set_error("frayhip_debug_rng: bad argument"); return FRAYHIP_E_ARG; }
    // one allocation: floats | doubles | ints | three 624-word generator states
    unsigned char* buf = nullptr;
    const size_t oF = 0, oD = 4096 * 4, oI = oD + 4096 * 8, oW = oI + 4096 * 4, total = oW + 3 * 624 * 4;
    HIP_TRY(hipMalloc((void**)&buf, total));
    hipLaunchKernelGGL(k_debug_rng, dim3(1), dim3(64), 0, nullptr, seed, n, (float*)(buf + oF), (double*)(buf + oD), (int32_t*)(buf + oI), int_hi, (uint32_t*)(buf + oW));
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && floats) e = hipMemcpy(floats, buf + oF, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && doubles) e = hipMemcpy(doubles, buf + oD, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && ints) e = hipMemcpy(ints, buf + oI, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) { set_error(std::string("frayhip_debug_rng: ") + hipGetErrorString(e)); return frayhip_detail::hip_error_code(e); }
    return FRAYHIP_OK;
}

__global__ void k_debug_libm(int n, const double* x, double* out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double sn, cs;
        fray_sincos(x[i], &sn, &cs);
        out[i] = sn;
        out[n + i] = cs;
        double a = x[i];
        a = a - 2.0 * floor(a * 0.5) - 1.0;                 // folded into [-1, 1) for acos
        out[2 * n + i] = fray_acos(a);
        out[3 * n + i] = a;
    }
}

int frayhip_debug_libm(int n, const double* x, double* sin_out, double* cos_out, double* acos_out, double* acos_arg)
{
    if (n <= 0 || n > (1 << 22) || !x) { set_error("frayhip_debug_libm: bad argument"); return FRAYHIP_E_ARG; }
    double *dx = nullptr, *dout = nullptr;
    HIP_TRY(hipMalloc((void**)&dx, (size_t)n * 8));
    if (hipMalloc((void**)&dout, (size_t)n * 32) != hipSuccess) { (void)hipFree(dx); set_error("frayhip_debug_libm: out of device memory"); return FRAYHIP_E_NOMEM; }
    int rc = FRAYHIP_OK;
    if (hipMemcpy(dx, x, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) rc = FRAYHIP_E_NODEVICE;
    if (rc == FRAYHIP_OK) {
        hipLaunchKernelGGL(k_debug_libm, dim3(grid_for(n)), dim3(256), 0, nullptr, n, dx, dout);
        if (hipDeviceSynchronize() != hipSuccess) rc = FRAYHIP_E_NODEVICE;
    }
    double* outs[4] = {sin_out, cos_out, acos_out, acos_arg};
    for (int k = 0; k < 4 && rc == FRAYHIP_OK; k++)
        if (outs[k] && hipMemcpy(outs[k], dout + (size_t)k * n, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FRAYHIP_E_NODEVICE;
    (void)hipFree(dx); (void)hipFree(dout);
    if (rc != FRAYHIP_OK) set_error("frayhip_debug_libm: device error");
    return rc;
}

static int pack_impl(const float* d_frame, float* d_packed, int width, int height, int channels, int first, int stride, void* hip_stream, int unpack)
{
    if (!d_frame || !d_packed || channels < 1) { set_error("frayhip_pack_buckets_device: bad argument"); return FRAYHIP_E_ARG; }
    int nb = frayhip_bucket_count(width, height, first, stride);
    if (nb < 0) { set_error("frayhip_pack_buckets_device: bad bucket range"); return FRAYHIP_E_ARG; }
    DFrame F = frayhip_detail::frame_grid(width, height);
    F.bucketFirst = first; F.bucketStride = stride; F.nBuckets = nb;
    int nItems = nb * 2304;
    if (nItems > 0) hipLaunchKernelGGL(k_pack, dim3(grid_for(nItems)), dim3(256), 0, (hipStream_t)hip_stream, F, nItems, channels, (float*)d_frame, d_packed, unpack);
    HIP_TRY(hipGetLastError());
    return FRAYHIP_OK;
}
int frayhip_pack_buckets_device(const float* d_frame, float* d_packed, int width, int height, int channels, int bucket_first, int bucket_stride, void* hip_stream)
{
    return pack_impl(d_frame, d_packed, width, height, channels, bucket_first, bucket_stride, hip_stream, 0);
}
int frayhip_unpack_buckets_device(const float* d_packed, float* d_frame, int width, int height, int channels, int bucket_first, int bucket_stride, void* hip_stream)
{
    return pack_impl(d_frame, (float*)d_packed, width, height, channels, bucket_first, bucket_stride, hip_stream, 1);
}

}  // extern "C"

