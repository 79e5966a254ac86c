/*
 * frayhip.h -- C ABI of the MI355X-native renderer for fray's per-pixel ray-trace hot path.
 *
 * The reference (anrieff/fray) has no FFI; its seams are C++ globals and virtuals (SURVEY.md
 * section 8b).  Every entry point below names the reference interface it stands behind.
 * All structs are POD, little-endian, FP64 geometry / FP32 colour, int32 indices; nothing here
 * mentions torch, HIP or C++ types.  No exception crosses this boundary: every call returns
 * 0 on success or a negative FRAYHIP_E_* code, with text available from frayhip_last_error().
 *
 * Citations are relative to the reference tree (src/...).
 */
#ifndef FRAYHIP_H
#define FRAYHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: the bucket numbering changed meaning (bucket b sits in column (b % BW + FRAYHIP_BUCKET_SKEW * row) % BW, see frayhip_bucket_xy): a host built
 * against version 2 that packs or unpacks buckets itself (row-major, bx = b % BW) would scatter tiles to the wrong places, so it must not pass the
 * version check.  frayhip_bucket_xy and frayhip_comm_available were added with the same change. */
#define FRAYHIP_ABI_VERSION 3

/* ---- error codes ------------------------------------------------------------------------ */
enum {
    FRAYHIP_OK            = 0,
    FRAYHIP_E_ARG         = -1,  /* bad argument (null pointer, bad size, bad mode)          */
    FRAYHIP_E_PARSE       = -2,  /* scene file syntax error / missing file (scene.cpp:544-554) */
    FRAYHIP_E_NODEVICE    = -3,  /* no usable HIP device (none present, bad id, no driver)    */
    FRAYHIP_E_UNSUPPORTED = -4,  /* scene uses an element the device path does not implement  */
    FRAYHIP_E_NOMEM       = -5,  /* host or device allocation failed                           */
    FRAYHIP_E_HIP         = -6,  /* any other HIP runtime failure (launch, copy, event); text in frayhip_last_error() */
    FRAYHIP_E_CANCELLED   = -7,  /* a progressive frame was cancelled by its callback: the output holds the frame of the samples resolved */
};

/* ---- scene description (flattened `Scene`, scene.h:280-299) ------------------------------ */

/* Transform, matrix.h:72-98: row-vector convention v*M; m and invM are row-major 3x3. */
typedef struct frayhip_transform {
    double offset[3];
    double m[9];
    double invM[9];
} frayhip_transform;

enum { FRAYHIP_GEOM_PLANE = 0, FRAYHIP_GEOM_SPHERE = 1, FRAYHIP_GEOM_CUBE = 2,
       FRAYHIP_GEOM_MESH = 3, FRAYHIP_GEOM_CSG = 4 };

/* Every geometry of the scene in declaration order (scene.geometries); `index` selects the
 * record in the per-kind array. */
typedef struct frayhip_geom_ref { int32_t kind, index; } frayhip_geom_ref;

/* Node, geometry.h:158-176.  Only nodes WITH a shader are listed (scene.cpp:563-568), in file
 * order; the position in this array is the hit id. */
typedef struct frayhip_node {
    int32_t geom;        /* index into geoms[]                       */
    int32_t shader;      /* index into shaders[]                     */
    int32_t bump_tex;    /* index into textures[] or -1              */
    int32_t _pad;
    frayhip_transform T;
} frayhip_node;

typedef struct frayhip_plane  { double limit, height; } frayhip_plane;          /* geometry.h:56-70  */
typedef struct frayhip_sphere { double O[3]; double R; } frayhip_sphere;       /* geometry.h:72-90  */
typedef struct frayhip_cube   { double O[3]; double halfSide; } frayhip_cube;  /* geometry.h:92-115 */
enum { FRAYHIP_CSG_PLUS = 0, FRAYHIP_CSG_AND = 1, FRAYHIP_CSG_MINUS = 2 };
typedef struct frayhip_csg    { int32_t op, left, right, _pad; } frayhip_csg;  /* left/right: geoms[] */

/* Triangle, triangle.h:30-41 (same members, same meaning). */
typedef struct frayhip_triangle {
    int32_t v[3], n[3], t[3];
    int32_t _pad;
    double gnormal[3], dNdx[3], dNdy[3], AB[3], AC[3], ABcrossAC[3];
} frayhip_triangle;

/* KDTreeNode, mesh.h:35-53, linearised in the order buildKD visits nodes (pre-order).
 * axis 0..2 = inner node, 3 = leaf (Axis::AXIS_NONE).  Children are allocated pairwise in the
 * reference (mesh.cpp:57) and stay adjacent here: right child = child0 + 1. */
typedef struct frayhip_kdnode {
    int32_t axis;
    int32_t child0;      /* inner: index of left child; leaf: -1            */
    int32_t parent;      /* -1 for the root                                 */
    int32_t tri_begin;   /* leaf: first entry in trirefs[]                  */
    int32_t tri_count;   /* leaf: number of entries                         */
    int32_t _pad;
    double  split;       /* inner: splitPos                                 */
} frayhip_kdnode;

/* Mesh, mesh.h:55-100.  vertices/normals/uvs hold xyz triples; element 0 of each is the
 * dummy the OBJ loader inserts (mesh.cpp:209-211); normals is empty (n_normals == 0) when the
 * file has none (mesh.cpp:252). */
typedef struct frayhip_mesh {
    int32_t n_vertices, n_normals, n_uvs, n_triangles, n_kdnodes, n_trirefs;
    int32_t faceted, backfaceCulling, has_kd, _pad;
    double  bbox_min[3], bbox_max[3];
    const double*           vertices;
    const double*           normals;
    const double*           uvs;
    const frayhip_triangle* triangles;
    const frayhip_kdnode*   kdnodes;
    const int32_t*          trirefs;
    int32_t kd_max_depth, kd_depth_sum;   /* statistics printed by mesh.cpp:91 */
} frayhip_mesh;

enum { FRAYHIP_TEX_CHECKER = 0, FRAYHIP_TEX_BITMAP = 1, FRAYHIP_TEX_BUMP = 2, FRAYHIP_TEX_FRESNEL = 3 };
/* Texture family, shading.h:33-110, 211-222.  Bitmap texels are float RGB triples in
 * texels[texel_offset ...], row-major, as Bitmap::data (bitmap.h:31-35).  For BUMP the texels are
 * already differentiated (bitmap.cpp:300-315).  `scaling` is stored as the reference uses it
 * at sample time (BitmapTexture inverts it at parse, shading.h:66-67). */
typedef struct frayhip_texture {
    int32_t kind, width, height, _pad;
    float   color1[3], color2[3];
    double  scaling, bumpIntensity, ior;
    int64_t texel_offset;        /* in floats */
} frayhip_texture;

enum { FRAYHIP_SHADER_CONST = 0, FRAYHIP_SHADER_LAMBERT = 1, FRAYHIP_SHADER_PHONG = 2,
       FRAYHIP_SHADER_REFL = 3, FRAYHIP_SHADER_REFR = 4, FRAYHIP_SHADER_LAYERED = 5 };
/* Shader family, shading.h:112-255. */
typedef struct frayhip_shader {
    int32_t kind;
    int32_t texture;             /* diffuseTex -> textures[] or -1                        */
    float   color[3];
    float   specularColor[3];
    float   mult[3];             /* Refl / Refr multiplier colour                         */
    int32_t numSamples;          /* Refl                                                  */
    double  exponent, specularMultiplier;
    double  glossiness, deflectionScaling;   /* Refl::beginFrame, shading.h:197-201       */
    double  ior;
    int32_t layer_begin, layer_count;        /* Layered -> layers[]                       */
} frayhip_shader;

typedef struct frayhip_layer { int32_t shader, texture; float opacity[3]; int32_t _pad; } frayhip_layer;

enum { FRAYHIP_LIGHT_POINT = 0, FRAYHIP_LIGHT_RECT = 1 };
/* Light family, lights.h:32-99.  center/area are what RectLight::beginFrame computes
 * (lights.cpp:37-46); area keeps the reference's float*float rounding. */
typedef struct frayhip_light {
    int32_t kind, xSubd, ySubd, _pad;
    float   color[3], power;
    double  pos[3];
    frayhip_transform T;
    double  center[3];
    double  area;
} frayhip_light;

/* Camera, camera.h:37-55 (scene-file parameters; the per-frame corner vectors are derived by
 * the renderer exactly as Camera::beginFrame does, camera.cpp:34-57). */
typedef struct frayhip_camera {
    double pos[3];
    double yaw, pitch, roll, fov, aspectRatio, focalPlaneDist, fNumber, stereoSeparation;
    int32_t dof, autofocus, numDOFSamples, _pad;
    float  leftMask[3], rightMask[3];
} frayhip_camera;

/* GlobalSettings, scene.h:252-278 / scene.cpp:783-814. */
typedef struct frayhip_settings {
    int32_t frameWidth, frameHeight;
    float   ambientLight[3];
    int32_t wantAA, gi, maxTraceDepth, dbg;
    float   saturation;
    int32_t wantPrepass, numPaths, numThreads, interactive, fullscreen;
} frayhip_settings;

/* CubemapEnvironment, environment.h:50-78: faces in CubeOrder negx,negy,negz,posx,posy,posz. */
typedef struct frayhip_environment {
    int32_t present;             /* scene declares an environment                         */
    int32_t loaded;              /* all six faces decoded                                 */
    int32_t width[6], height[6];
    int64_t texel_offset[6];     /* in floats, into texels[]                              */
} frayhip_environment;

typedef struct frayhip_scene_desc {
    int32_t abi_version;
    int32_t n_nodes, n_geoms, n_planes, n_spheres, n_cubes, n_csgs, n_meshes;
    int32_t n_shaders, n_layers, n_textures, n_lights;
    int64_t n_texels;            /* floats */
    const frayhip_node*     nodes;
    const frayhip_geom_ref* geoms;
    const frayhip_plane*    planes;
    const frayhip_sphere*   spheres;
    const frayhip_cube*     cubes;
    const frayhip_csg*      csgs;
    const frayhip_mesh*     meshes;
    const frayhip_shader*   shaders;
    const frayhip_layer*    layers;
    const frayhip_texture*  textures;
    const frayhip_light*    lights;
    const float*            texels;
    frayhip_environment environment;
    frayhip_camera      camera;
    frayhip_settings    settings;
} frayhip_scene_desc;

/* ---- frame request ----------------------------------------------------------------------- */
enum {
    FRAYHIP_MODE_PRIMARY_ID = 0, /* camera ray through integer (x,y), closest hit only:
                                    the node/light loops of main.cpp:250-271               */
    FRAYHIP_MODE_RENDER     = 1, /* what render() does (main.cpp:373-405): Whitted, or path
                                    tracing when settings.gi                               */
};

/* Frame size is settings.frameWidth x frameHeight (the reference takes it from the SDL
 * surface created with those values, sdl.cpp:77-88, main.cpp:508).  Work is split in the
 * reference's 48x48 buckets (sdl.cpp:243-262); a call renders the buckets b with
 * b % bucket_stride == bucket_first, so N ranks with stride N cover the frame.  Pixels of other
 * buckets are left untouched in the output buffers.
 * Bucket b of a frame BW = ceil(W / 48) buckets wide is the one in bucket row by = b / BW and bucket
 * column bx = (b % BW + FRAYHIP_BUCKET_SKEW * by) % BW (frayhip_bucket_xy): every bucket row is rotated
 * against the one above it, so that a stride that divides BW (8 ranks on a 1920-wide frame: BW = 40)
 * deals diagonal stripes, not eight fixed sets of columns -- with plain row-major numbering rank r
 * would own the same five columns in every row, and the slowest rank's share of forest.fray was 8 %
 * above the mean. */
#define FRAYHIP_BUCKET_SKEW 3
typedef struct frayhip_frame {
    int32_t  mode;
    uint32_t seed;               /* RNG contract seed; the reference uses 42   */
    int32_t  bucket_first, bucket_stride;
    int32_t  spp_chunk;          /* path-tracing samples kept in flight per pixel; 0 = auto */
    int32_t  flags;              /* FRAYHIP_FRAME_* bits                                   */
} frayhip_frame;

enum {
    FRAYHIP_FRAME_STATS = 1,     /* also count rays / node tests / ... into frayhip_stats (uses the
                                    instrumented kernel variants: slower, same results)     */
};

typedef struct frayhip_stats {
    uint64_t closest_rays;       /* closest-hit queries (main.cpp:182-199 / 254-271)       */
    uint64_t shadow_rays;        /* visible() queries (main.cpp:64-80)                     */
    uint64_t node_tests;         /* Node::intersect calls                                  */
    uint64_t kd_inner_visits;    /* inner KD nodes entered                                 */
    uint64_t leaf_refs;          /* triangle indices read from leaves                      */
    uint64_t tri_tests;          /* Mesh::intersectTriangle calls                          */
    uint64_t prim_tests;         /* plane / sphere / cube / rect-light tests               */
    uint64_t smooth_hits;        /* winning hits that interpolated normals/uvs             */
    uint64_t samples;            /* camera samples                                         */
    uint64_t texture_fetches;
    double   ms_total;           /* wall time of the call                                  */
    double   ms_kernels;         /* device time between first and last kernel (HIP events) */
    double   ms_trace;           /* device time inside the dominant kernel: k_pt_bounce /
                                    k_whitted / k_primary (HIP events around each launch)   */
    uint64_t trace_launches;     /* number of launches summed into ms_trace                */
    double   alg_bytes_trace;    /* SURVEY 8(d) byte model evaluated on those launches       */
    /* path tracing only: the next-event shadow rays run in their own kernel (k_pt_shadow) */
    double   ms_shadow;          /* device time inside k_pt_shadow                           */
    uint64_t shadow_launches;
    double   alg_bytes_shadow;   /* byte model of the shadow-ray kernel                      */
    /* algorithmic FP64 operations of the same launches (Node::intersect ~90, triangle test
       ~45, box test ~30, primitive ~30 operations each), for the FP64-issue roofline      */
    double   alg_flops_trace;
    double   alg_flops_shadow;
} frayhip_stats;

/* ---- host scene layer (stands behind Scene::parseScene + Scene::beginRender,
 *      scene.cpp:751-767, main.cpp:503-514).  No GPU needed. -------------------------------- */
typedef struct frayhip_host_scene frayhip_host_scene;

/* Parses a .fray file (plus the OBJ/BMP/EXR files it names, relative to the scene file's
 * directory), runs the beginRender work (KD build, bump differentiate) and flattens. */
int  frayhip_scene_parse(const char* fray_path, frayhip_host_scene** out);
/* Mutable flattened view; the caller may edit .settings and .camera before creating a device
 * scene, which is how the reference's overrides are applied (scene.settings.* = ...). */
frayhip_scene_desc* frayhip_host_scene_desc(frayhip_host_scene* hs);
void frayhip_host_scene_free(frayhip_host_scene* hs);

/* ---- device side (stands behind render(), main.cpp:373) ----------------------------------- */
typedef struct frayhip_scene frayhip_scene;

/* Select the HIP device for this process (one process per GPU). */
int  frayhip_init(int device_id);
/* Deep-copies the description into device memory. */
int  frayhip_scene_create(const frayhip_scene_desc* desc, frayhip_scene** out);
void frayhip_scene_destroy(frayhip_scene* s);
/* Replaces the camera and the global settings of an uploaded scene without touching the geometry
 * (the reference's interactive loop mutates scene.camera between frames, main.cpp:437-491;
 * Camera::beginFrame re-derives everything per frame anyway).  Either pointer may be NULL. */
int  frayhip_scene_set_view(frayhip_scene* s, const frayhip_camera* camera, const frayhip_settings* settings);

/* ---- scene edits (stand behind the reference's mutable Scene: callers edit scene.nodes[i]->T, a light or a shader between frames and
 *      RectLight::beginFrame / Reflection::beginFrame re-derive the per-frame data, lights.cpp:37-46, shading.h:197-201) ----------------------
 * Replaces the EDITABLE part of an uploaded scene with what `desc` holds now.  After the call every entry point behaves exactly -- pictures, hit
 * records, work counters and the read-only figures of frayhip_scene_get_option -- as on a handle frayhip_scene_create(desc) would have made.
 * Editable: nodes[] (every field: geom may name any existing entry of geoms[], shader, bump_tex, T); planes[], spheres[], cubes[]; shaders[],
 *   layers[], lights[] (every field, a light's kind and subdivision included); of textures[]: color1, color2, scaling, bumpIntensity, ior.
 * Fixed (a difference is FRAYHIP_E_ARG, and frayhip_last_error() names the table): every element count, n_texels included; geoms[] and csgs[];
 *   every mesh's header scalars -- and by contract its arrays, which the call does not look at; every texture's kind, width, height and
 *   texel_offset; environment.  desc->camera and desc->settings are not read: frayhip_scene_set_view changes them.
 * What is read: the editable arrays, geoms[], csgs[], the mesh headers and the texture records.  No mesh array pointer and not desc->texels is
 *   dereferenced (they may dangle); host time and uploaded bytes do not depend on the triangle, KD-node, leaf-reference or texel counts.
 * The editable part gets frayhip_scene_create's range checks.  Every check, and the building of the new tables, comes before the first byte
 *   is uploaded: a call that returns FRAYHIP_E_ARG has changed nothing.  A scene whose frame is being rendered refuses the call
 *   (FRAYHIP_E_ARG), as frayhip_scene_set_view does.  A HIP failure during the upload returns its code, and the handle may then only be
 *   destroyed: its tables are partly the new ones.
 * The call blocks.  It runs after everything the scene's earlier calls enqueued (every render and query entry returns with its streams
 *   synchronised).  Kept: the workspace, the streams and their scratch arenas, every option, and the seed table (its key does not involve the
 *   scene's content).
 * frayhip_scene_get_option figures: "scene_updates" (updates since creation), "scene_update_bytes" (bytes the last update uploaded),
 *   "arena_bytes" (the size of the scene's device arena). */
int  frayhip_scene_update(frayhip_scene* s, const frayhip_scene_desc* desc);

/* The parser's own arithmetic, for callers who edit a description: host only, no device is touched.  FRAYHIP_E_ARG for a NULL pointer.
 * frayhip_transform_*: Transform of matrix.h:72-98, on {m, invM, offset} in place -- identity resets; scale multiplies m by diag(x, y, z) from
 *   the right and inverts; rotate (degrees: yaw, pitch, roll) multiplies by rotZ(roll) rotX(pitch) rotY(yaw) and inverts; translate adds to
 *   the offset.  The calls in the order of a block's scale / rotate / translate lines give the bytes frayhip_scene_parse stores.
 * frayhip_light_begin_frame: RectLight::beginFrame (lights.cpp:37-46) -- center and area from T (area keeps the float * float product); a
 *   point light gets the parser's zeros.
 * frayhip_shader_begin_frame: Reflection::beginFrame (shading.h:197-201) -- deflectionScaling from glossiness. */
int  frayhip_transform_identity(frayhip_transform* T);
int  frayhip_transform_scale(frayhip_transform* T, double x, double y, double z);
int  frayhip_transform_rotate(frayhip_transform* T, double yaw, double pitch, double roll);
int  frayhip_transform_translate(frayhip_transform* T, double x, double y, double z);
int  frayhip_light_begin_frame(frayhip_light* light);
int  frayhip_shader_begin_frame(frayhip_shader* shader);

/* Tunables of an uploaded scene (value ranges checked, FRAYHIP_E_ARG otherwise):
 *   "pt_lanes"      1..4   path-tracing batches in flight at once, each on its own HIP stream (default 4;
 *                          1 serialises every launch, which is what a per-kernel profile wants)
 *   "pt_budget_mib" MiB of device memory a path-traced frame may use for its queues (about 340 B per path in
 *                          flight; default 24576): a frame is cut into batches of samples that fit
 *   "speculate_fans" 0 / 1  glossy reflections of eight or more samples at depth 0 (Reflection::shade, shading.cpp:172-204) in a scene
 *                          whose lights draw no random numbers: the fan's directions are drawn ahead and its rays traced as work items of
 *                          their own, then looked up while none of them drew (default 1; the picture is the same either way,
 *                          hw9/dragon.fray 1080p 16.4 -> 7.8 ms)
 *   "fused_whitted_max" 0..1024  a Whitted frame of a scene without recursive shaders and without KD meshes whose lights take at most this many
 *                          samples per hit (default 4) asks visible() inside the shading kernel -- one launch instead of seed + shade + visible +
 *                          gather + resolve: zaphod.fray 1080p 0.30 -> 0.17 ms; 0 = always the separate launches (the picture is the same)
 *   "fp_contract"   0 / 1  0 (default): the reference's arithmetic everywhere (no fused multiply-add, IEEE division and square root, correctly
 *                          rounded sin / cos / acos): hit records AND colours are the CPU reference build's, bit for bit.  1: path tracing only -- every
 *                          bounce AFTER a camera sample's first closest hit and every next-event visibility query run kernels built with
 *                          -ffp-contract=fast, reciprocal / reciprocal-square-root with two refinement steps, plain-double sin / cos, and
 *                          sqrt(1 - c^2) for sin(acos c).  Primary hit records (MODE_PRIMARY_ID) and a sample's first bounce stay exact; shaded colour
 *                          stays inside 1e-4 RMS per channel (measured: 0 of 2 073 600 pixels of the 1080p x 64 spp Cornell frame differ at all, since
 *                          FP64 differences of 1e-16 vanish where geometry becomes an FP32 colour factor); cornell 1080p x 64 spp 92.4 -> 81.6 ms.
 *                          Where the option does nothing: scenes with Cube / CSG geometry have no contracted kernels (their frames are the exact
 *                          ones, "contracted_launches" 0), nor do Whitted frames (gi 0) or primary hit records; frames whose paths may draw more
 *                          than 227 random words per generator (maxTraceDepth >= 20: per-path generator state) keep every bounce exact and run
 *                          only the next-event visibility queries contracted.  tests/test_gpu_contract.py holds all of this and the primitives' bounds.
 *   "skip_null_segments" 0 / 1  path tracing, the timed kernels (frames rendered without FRAYHIP_FRAME_STATS): a next-event sample whose contribution is +0.0f in
 *                          all three channels by bit pattern -- Reflection / Refraction::eval, a Lambert surface facing away from the sampled light point -- is not
 *                          queued for its visibility query (default 1).  The query's answer could only choose between storing black and storing black, so the
 *                          picture is the same bit for bit (tests/test_gpu_null_segments.py); a -0.0f or NaN channel is traced as before.  0 queues every segment.
 *                          The counting kernels always trace every segment: shadow_rays stays the reference's count.
 *   "segment_planes" 0 / 1  path tracing, the timed any-hit kernel of scenes whose kernels are the leanest variants (no KD mesh, no Cube / CSG, no texture:
 *                          cornell_box's): before its node loop every next-event segment is tested against the planes of the scene's ELIGIBLE nodes -- untransformed
 *                          meshes without a KD-tree, of fewer than six triangles, with finite bounded coordinates and no zero normal; at most 16 planes and 16
 *                          nodes per scene, else none -- and a node is skipped by a wave of 64 segments when both ends of every one of them lie on one side of
 *                          every triangle's plane by a margin (default 1).  Under that certificate (fray_amd/csrc/dev_segcert.hpp: statement, proof,
 *                          tests/test_segcert.py) the reference's own arithmetic cannot report a hit of such a triangle nearer than the segment's end, so the
 *                          picture is the same bit for bit, in both arithmetics (tests/test_gpu_segment_planes.py).  0 asks every node, as do the counting
 *                          kernels always: node_tests and tri_tests stay the reference's counts.
 *   "certified_segments" 0 / 1  path tracing, the timed bounce kernel of the same leanest variants, in a scene whose EVERY node is either eligible for
 *                          "segment_planes" or a mesh inside an exact gate (an untransformed mesh without a KD-tree of six triangles or more; at most
 *                          eight): a next-event segment whose ray provably misses every gate and whose ends lie on one side of every plane of the
 *                          scene by the margin is unoccluded as the reference's own arithmetic computes it, so the kernel that sampled it stores its
 *                          term at once and the segment is neither queued nor traced (default 1).  The picture is the same bit for bit, in both
 *                          arithmetics (tests/test_gpu_certified_segments.py; tests/test_certified_segments_host.py runs the rule on the host).  No
 *                          effect while "segment_planes" is 0, in any other scene (a sphere, a plane, a Cube / CSG node, a transformed or a KD mesh,
 *                          too many planes or gates, no light, a plane that contains every light whole, or coordinates so large that a segment's start, 1e-6 off
 *                          its surface, is inside the margin of that surface's own plane on every such mesh: "certified_segments_eligible" reads 0) and on the counting kernels, which queue every segment:
 *                          shadow_rays stays the reference's count.  frayhip_scene_update recomputes the eligibility with the node tables and the lights.
 *   "seed_table_mib" 0..1048576  the cap, in MiB, of the scene's seed table (default 4096).  Every camera sample's generator starts from x[397] of the
 *                          mt19937 seeding recurrence of sample_seed(seed, pixel, sample) -- a word that depends on the contract seed, the frame size and the
 *                          bucket share and on nothing else, and that costs a 397-step chain (k_seed) per sample.  The table keeps these words, 4 bytes per
 *                          camera sample (1080p x 64 spp: 518 MiB), from one frayhip_render* frame of the scene to the next: a frame with the same seed, size
 *                          and bucket share launches k_seed only for sample planes the table does not hold yet -- none at all when it repeats the last
 *                          frame's, whatever changed in the camera, the view settings, spp_chunk, pt_lanes or fp_contract; a frame asking for more samples
 *                          seeds the new planes only.  A change of seed, size or bucket share refills the table (the same k_seed work as without it, written
 *                          to another address: frames rendered with seed + k, as a denoised sequence is, gain nothing and lose nothing but the memory).
 *                          The picture is the same bit for bit (tests/test_gpu_seed_table.py).  A frame whose table would pass the cap, or whose allocation
 *                          fails, renders as without the table; the workspace takes the table's memory back before it plans smaller batches.
 *                          0 = off: nothing is held, every batch seeds its own words.  Radiance queries, adaptive and feature frames do not use the table.
 * The environment variables FRAYHIP_PT_LANES / FRAYHIP_PT_BUDGET_MIB / FRAYHIP_SPECULATE_FANS / FRAYHIP_FP_CONTRACT / FRAYHIP_SKIP_NULL_SEGMENTS /
 * FRAYHIP_SEGMENT_PLANES / FRAYHIP_CERTIFIED_SEGMENTS / FRAYHIP_SEED_TABLE_MIB preset them at frayhip_scene_create. */
int  frayhip_scene_set_option(frayhip_scene* s, const char* name, int64_t value);
/* Reads an option back, or one of the last frame's read-only figures: "fans_filed" (camera samples whose first fan was drawn ahead),
 * "fan_children" (rays traced ahead), "fan_children_looked_up" (results used), "fans_given_up" (fans in which a ray drew a random
 * number after all, so that the rest of the fan was traced in place), "contracted_launches" (launches of the last frame that ran a kernel of
 * the "fp_contract" build), "shadow_segments" (the next-event segments the timed kernels of the last frayhip_render / frayhip_render_progressive
 * frame decided: the entries of its next-event queues, i.e. the visibility queries it actually traced, plus "shadow_segments_certified", the segments
 * option "certified_segments" decided without a query), "certified_segments_eligible" (1 when every node of the scene, as last uploaded or updated, is a
 * plane node or an exactly gated one, some light has a point off every plane and some plane node's own margins are below 1e-6), "segment_plane_nodes" (the scene's nodes eligible for option "segment_planes"; fixed at
 * frayhip_scene_create), "shadow_nodes_skipped" (the last such frame's sum, over the wave iterations of its any-hit launches -- 64 segments each -- of the
 * nodes skipped under that option), "whitted_path" (how the last Whitted frame ran: 0 = the recursive kernel, 1 = shade / visible / gather launches, 2 = fused), "pt_budget_effective_mib" (the queue budget frames currently plan with: pt_budget_mib clamped to the device's
 * free memory, halved when an allocation failed and the frame could be planned again), "seed_table_bytes" (what the seed table currently holds on the
 * device), "seed_launches" (k_seed launches of the last frame) and "seed_planes_reused" (sample planes the last frame took from the table).
 * "batch_lanes": the streams the last frame's batches ran on, as planned (1 unless path-traced). */
int  frayhip_scene_get_option(frayhip_scene* s, const char* name, int64_t* value);
/* Tight gates.  Path tracing, scenes with exact gates: a gate that stands for an ELIGIBLE mesh -- untransformed, no KD-tree, six to 32 triangles with
 * finite coordinates below 2^24, stored normals that are their edges' cross products, no sliver, at most six normal directions (a box has three) --
 * is tested by the producers against the box of the mesh's own triangles, with a guard against rays nearly parallel to a face, instead of the
 * mesh's bounding box.  The bounding box of a mesh loaded from an OBJ file also holds the loader's dummy vertex (0, 0, 0): cornell_box's two blocks
 * fill a fraction of theirs.  Under the certificate (fray_amd/csrc/dev_gatecert.hpp: statement, proof; tests/test_gatecert_host.py) no triangle of
 * the mesh accepts the ray as the reference's own arithmetic computes it, so the picture is the same bit for bit, in both arithmetics
 * (tests/test_gpu_tight_gates.py); more rays are filed gate-free and more next-event segments are certified.  On by default; the environment
 * variable FRAYHIP_TIGHT_GATES=0 presets it off at frayhip_scene_create.  Takes effect in frayhip_render* frames of scenes whose kernels are the
 * leanest variants (no KD mesh, no Cube / CSG, no texture), in the timed kernels of the exact arithmetic: the counting kernels and the fp_contract
 * copies keep the bounding boxes (they measured slower with it), as do the query, adaptive and feature entries.
 * enable: 1 / 0 switches it on / off (not while the scene renders), -1 leaves it.  enabled, eligible (either may be null): the switch, and the number
 * of gates of the scene, as last uploaded or updated, that are eligible. */
int  frayhip_scene_tight_gates(frayhip_scene* s, int enable, int64_t* enabled, int64_t* eligible);
/* Camera skip.  Path tracing, first bounce: a wave of camera rays -- one 8x8 pixel tile at one sample index -- leaves out every ELIGIBLE mesh that all its
 * rays provably miss.  Eligible: a mesh node that is untransformed, has no KD-tree and at most 32 triangles (two suffice: a wall), a node index below 32, and
 * triangles the certificate of fray_amd/csrc/dev_gatecert.hpp admits (as for tight gates above); the first 16 such nodes get a miss record, made from the
 * node's own triangles.  Under the certificate no triangle of the mesh accepts the ray as the reference's own arithmetic computes it, so the picture is the
 * same bit for bit (tests/test_gpu_camera_skip.py).  On by default; the environment variable FRAYHIP_CAMERA_SKIP=0 presets it off at frayhip_scene_create.
 * Takes effect in the frames of frayhip_render* whose first bounce makes its own camera rays (mono, register generators) on the leanest timed kernel of the
 * exact arithmetic -- a sample's first bounce runs that kernel under option "fp_contract" too; the counting kernels ask every node.
 * enable: 1 / 0 switches it on / off (not while the scene renders), -1 leaves it.  enabled, eligible, skipped, waves (each may be null): the switch; the
 * number of miss records of the scene, as last uploaded or updated; the last frame's (wave, node) pairs left out; and the first-bounce wave iterations of
 * 64 camera rays that evaluated the records (those with a ray in the frame). */
int  frayhip_scene_camera_skip(frayhip_scene* s, int enable, int64_t* enabled, int64_t* eligible, int64_t* skipped, int64_t* waves);
/* Camera tiles.  Path tracing, first bounce, the same frames and the same kernel as camera skip above: what is a property of a wave's 8x8 pixel tile is decided
 * once per frame instead of per lane and per sample.  A small kernel fills a table with one entry per tile of the frame's items -- the tile's pixel origin and,
 * for a pinhole camera (no depth of field), the eligible meshes that NO camera ray of the tile can hit, whatever its jitter: the certificate of camera skip
 * evaluated on the tile's four corner directions (fray_amd/csrc/dev_camtile.hpp) -- and a first-bounce wave reads its entry.  The table is made anew by every
 * such frame.  The skipped meshes are ones no ray of the tile hits as the reference's own arithmetic computes it, so the picture is the same bit for bit
 * (tests/test_gpu_camera_tiles.py); a tile's word may hold fewer meshes than its 64 rays at one sample index would have agreed on.  With a depth-of-field
 * camera, or with camera skip switched off, the words are zero (the per-wave test of camera skip serves a depth-of-field camera) and the table gives the pixel
 * origin only.  On by default; the environment variable FRAYHIP_CAMERA_TILES=0 presets it off at frayhip_scene_create.  frayhip_scene_camera_skip's `skipped`
 * and `waves` count the same things with either source of the word.
 * enable: 1 / 0 switches it on / off (not while the scene renders), -1 leaves it.  enabled (may be null): the switch. */
int  frayhip_scene_camera_tiles(frayhip_scene* s, int enable, int64_t* enabled);
/* Shade shortcuts.  Path tracing, the timed kernels of scenes without Cube / CSG geometry, KD meshes and textures, in both arithmetics: arithmetic whose
 * result is known before it runs is left out.  Bit 0 of `eligible`, the nodes: EVERY node is an untransformed mesh (offset +0, m = invM = I bit for bit) that is
 * flat, has no KD-tree, at most 32 triangles, a shader that reads no (u, v) and no bump texture -- a hit is then shaded without the node's transform
 * (multiplications by 0 and 1) and with the triangle's world normal from a table made at upload.  Bit 1, the lights: every light is a RectLight whose m and invM
 * have zero off-diagonal and finite diagonal entries and whose offset has three finite nonzero components (scaled along the axes and translated, not rotated)
 * -- its intersection and its samples use the three diagonal products; a light whose xSubd is a power of two finds a sample's cell by mask and shift.  Every
 * value that leaves the changed functions is the same bit for bit (the proofs: fray_amd/csrc/dev_shade.hpp finalize_hit, light_nth_sample; dev_trace.hpp
 * light_intersect), so the picture is (tests/test_gpu_shade_shortcuts.py).  On by default; the environment variable FRAYHIP_SHADE_SHORTCUTS=0 presets it off at
 * frayhip_scene_create.  The counting kernels take the general forms.
 * enable: 1 / 0 switches it on / off (not while the scene renders), -1 leaves it.  enabled, eligible (either may be null): the switch, and the two bits of the
 * scene as last uploaded or updated. */
int  frayhip_scene_shade_shortcuts(frayhip_scene* s, int enable, int64_t* enabled, int64_t* eligible);

/* Threads: a frayhip_scene renders one frame at a time (it owns one workspace and one set of
 * counters), as the reference calls render() from one thread at a time (main.cpp:407-412,448);
 * different scenes may be driven from different threads.  frayhip_last_error() is per thread. */
/* Blocking render.  Any output pointer may be NULL.  Host buffers, row-major:
 *   rgb      W*H*3 float  -- `vfb` (main.cpp:53,360), linear, unclamped
 *   hit_id   W*H   int32  -- node index, -1 miss, -2-i light i   (MODE_PRIMARY_ID)
 *   hit_dist W*H   double -- world distance, 1e99 on a miss       (MODE_PRIMARY_ID)          */
int  frayhip_render(frayhip_scene* s, const frayhip_frame* f,
                    float* rgb, int32_t* hit_id, double* hit_dist, frayhip_stats* st);
/* Same, with DEVICE pointers (hipMalloc'ed by the caller, e.g. a torch tensor's data_ptr);
 * work is enqueued on `hip_stream` (a hipStream_t, NULL = default stream) and the call
 * returns after the stream has been synchronised.  A path-traced frame also runs batches on
 * streams of its own; they start after everything already enqueued on `hip_stream` and are
 * joined back into it before the call returns, so the caller sees one stream's ordering. */
int  frayhip_render_device(frayhip_scene* s, const frayhip_frame* f,
                           float* d_rgb, int32_t* d_hit_id, double* d_hit_dist,
                           void* hip_stream, frayhip_stats* st);

/* ---- progressive frames (stand behind the reference's displayVFBRect / `rendering` seam, sdl.cpp:287-311, main.cpp:339-368) ----
 * A frame is rendered in batches of frayhip_frame.spp_chunk samples per pixel (0 = as many as the queue budget holds).  The per-pixel FP32
 * sum runs in sample order from batch to batch, and sample i of a pixel is seeded the same whatever the frame's spp, so after the batches
 * covering the first s samples, sum / (float)s IS the frame this scene renders with s samples per pixel, bit for bit: a preview is an exact
 * lower-spp frame, and a cancelled frame is an exact, usable one.
 *
 * Callback thread and timing: fn runs on the calling thread, after a batch's resolve has completed on the device.  samples_done strictly
 *   increases from call to call and always falls on a batch boundary.  The last call has final = 1 (its return value is ignored);
 *   MODE_PRIMARY_ID, maxTraceDepth < 0 and one-batch frames make exactly that one call.  A call that fails with an error makes no final call.
 * Cancel: a nonzero return means cancel.  No further batch is enqueued; the batches already in flight are finished and resolved in order,
 *   then rgb receives the mean of every resolved sample (the same FP32 division as the resolve), the final call reports that sample count
 *   and the call returns FRAYHIP_E_CANCELLED with rgb and *st valid (*st counts the work of the resolved batches).  A cancel that comes when
 *   every batch is already in flight cuts nothing: the frame completes and the call returns FRAYHIP_OK.
 * Cancel latency: at most the batches in flight when fn returned, which is at most the number of lanes (option "pt_lanes"; one for the
 *   Whitted integrators).  The caller chooses the granularity through frame.spp_chunk.
 * Previews: preview_ms < 0 asks for none, 0 for one after every batch but the last, > 0 for at most one per that many milliseconds of wall
 *   time (counted from the start of the call).  A preview writes the running mean of the call's buckets into the caller's rgb buffer, as
 *   the reference's vfb fills in while it renders; pixels of other buckets are untouched.  preview = 1 when rgb holds such a frame; the
 *   final call of a MODE_RENDER frame always carries the finished frame (preview = 1).  The host entry has copied the frame to the host rgb
 *   before calling back; the device entry's frame is complete in device memory (the batch's stream was synchronised) before calling back.
 *   The rgb pointer is valid during the call only.
 * Pacing: at most `lanes` batches are enqueued ahead of the one being reported, so the device keeps working while the host waits on a
 *   batch; a batch's resolve is enqueued after the previous batch's call returned, so the buffer is not rewritten while fn reads it.
 * Reentrancy: fn must not render or change the same scene: frayhip_render* and frayhip_scene_set_view / _set_option return FRAYHIP_E_ARG
 *   while the scene renders (the frame being rendered is unaffected).  Nor may fn destroy it.  Other scenes may be used. */
typedef struct frayhip_progress {
    int32_t samples_done;        /* samples per pixel resolved so far (a batch boundary)                                  */
    int32_t samples_total;       /* samples per pixel of the whole frame                                                   */
    int32_t batches_done, batches_total;
    double  ms_elapsed;          /* wall time since the call started                                                       */
    int32_t preview;             /* 1: rgb holds the running mean of the call's buckets                                    */
    int32_t final;               /* 1: the last call of this frame                                                         */
    const float* rgb;            /* the frame: host memory for frayhip_render_progressive, device memory for the device entry; NULL unless preview */
} frayhip_progress;

typedef struct frayhip_progressive {
    int  (*fn)(void* user, const frayhip_progress* p);     /* nonzero return = cancel                                     */
    void*  user;
    double preview_ms;           /* < 0 no previews, 0 after every batch, > 0 at most one per that many ms (NaN: FRAYHIP_E_ARG) */
} frayhip_progressive;

/* frayhip_render / frayhip_render_device with a progress request (p may not be NULL; p->fn may be NULL for a frame that only paces). */
int  frayhip_render_progressive(frayhip_scene* s, const frayhip_frame* f, const frayhip_progressive* p,
                                float* rgb, int32_t* hit_id, double* hit_dist, frayhip_stats* st);
int  frayhip_render_device_progressive(frayhip_scene* s, const frayhip_frame* f, const frayhip_progressive* p,
                                       float* d_rgb, int32_t* d_hit_id, double* d_hit_dist, void* hip_stream, frayhip_stats* st);

/* ---- ray queries (stand behind Camera::getScreenRay, camera.cpp:59-92; the closest-hit loops that debugRayTrace fires through a clicked
 *      pixel, main.cpp:178-199, 250-271, 426-435; and visible(), main.cpp:64-80) ----------------------------------------------------------
 * Rays the caller chooses, traced against an uploaded scene.  All arrays are row-major and contiguous; n rows each.  The _device entries take
 * DEVICE pointers, enqueue on `hip_stream` (NULL = default stream) and return after that stream has been synchronised, as
 * frayhip_render_device does; the host entries copy in, run the same device path and copy out.
 *
 * frayhip_camera_rays: Camera::getScreenRay(x, y, eye) of the scene's current view (frayhip_scene_set_view) for the film positions xy[n][2];
 *   eye 0 = CENTER, 1 = LEFT, 2 = RIGHT.  origin[n][3] and dir[n][3] (either may be NULL, not both).  The device's camera ray of a frame, on the
 *   same camera record: for integer positions these are the rays of FRAYHIP_MODE_PRIMARY_ID, bit for bit.  xy == NULL means every integer pixel
 *   in row-major order (x fastest) and requires n == frameWidth * frameHeight.  Thin-lens (DOF) rays draw random numbers and are not offered.
 * frayhip_trace_rays: the reference's closestHit -- every node in order, the first node wins ties, then the rect lights -- for origin[n][3],
 *   dir[n][3].  Directions are used as given, as Ray.dir is: node and light tests normalise in their own local frame, so any nonzero finite
 *   direction is defined.  Outputs, any of them may be NULL (not all three):
 *     hit_id[n]      node index, -1 miss, -2-i light i (the ids of FRAYHIP_MODE_PRIMARY_ID)
 *     hit_dist[n]    world distance, 1e99 on a miss
 *     hit_rec[n][9]  dist, ip[3], norm[3], u, v: the IntersectionInfo of the winner before bump mapping.  A rect light's record holds the ip and norm
 *                    RectLight::intersect writes (lights.cpp:79-103) and u = v = 0; a miss is {1e99, 0, ...}.  u, v are made for every geometry
 *                    (a sphere's atan2 / asin ones included, whatever the scene's textures).  NULL: the winner is never finalised.
 * frayhip_visible: visible(a[i], b[i]) as main.cpp:64-80 computes it (dir = normalize(b - a), maxDist = |a - b|, lights do not occlude):
 *   vis[i] = 1 when the segment is visible, 0 otherwise.
 * Degenerate input is answered without tracing (the outcome the reference's arithmetic gives anyway, and no NaN enters the KD walk):
 *   a ray with a non-finite component, or whose direction's squared length dir.x^2 + dir.y^2 + dir.z^2 is 0 (a zero direction) or overflows,
 *   is a miss; a segment with a non-finite endpoint, or whose length |b - a| is 0 (a == b) or overflows, is visible.
 * flags: FRAYHIP_FRAME_STATS selects the counting kernel variants.  *st may be NULL; when given it holds ms_total, ms_kernels and the query kernel's
 *   device time in ms_trace / trace_launches (frayhip_visible: ms_shadow / shadow_launches), and with the stats flag the work counters of the rays
 *   traced: closest_rays (shadow_rays), node_tests, kd_inner_visits, leaf_refs, tri_tests, prim_tests, smooth_hits.  The alg_* fields stay 0.
 * FRAYHIP_E_ARG, before the device is touched: a NULL scene, n < 0 or n > INT32_MAX, a NULL input with n > 0, no output, a double / int32 device
 *   pointer that is not 8 / 4-byte aligned, eye outside 0..2, and any call on a scene whose frame is being rendered (from inside its progress
 *   callback).  n == 0 is a successful no-op.  A query changes no option of the scene and none of the last frame's figures that
 *   frayhip_scene_get_option reports. */
int  frayhip_camera_rays(frayhip_scene* s, int64_t n, const double* xy, int eye, double* origin, double* dir);
int  frayhip_camera_rays_device(frayhip_scene* s, int64_t n, const double* d_xy, int eye,
                                double* d_origin, double* d_dir, void* hip_stream);
int  frayhip_trace_rays(frayhip_scene* s, int64_t n, const double* origin, const double* dir, int flags,
                        int32_t* hit_id, double* hit_dist, double* hit_rec, frayhip_stats* st);
int  frayhip_trace_rays_device(frayhip_scene* s, int64_t n, const double* d_origin, const double* d_dir, int flags,
                               int32_t* d_hit_id, double* d_hit_dist, double* d_hit_rec, void* hip_stream, frayhip_stats* st);
int  frayhip_visible(frayhip_scene* s, int64_t n, const double* a, const double* b, int flags, uint8_t* vis, frayhip_stats* st);
int  frayhip_visible_device(frayhip_scene* s, int64_t n, const double* d_a, const double* d_b, int flags,
                            uint8_t* d_vis, void* hip_stream, frayhip_stats* st);

/* ---- radiance queries (stand behind trace(ray, rnd), main.cpp:286-293: raytrace(ray) for Whitted scenes, pathtrace(ray, Color(1, 1, 1), rnd)
 *      with `gi on`; and the integrator debugRayTrace fires through a clicked pixel, main.cpp:426-435) -----------------------------------------
 * The colour of rays the caller chooses, under the scene's current settings and integrator (settings.gi, as frayhip_scene_set_view left it).
 * Arrays as in the ray queries above: row-major, contiguous, n rows; the _device entry takes DEVICE pointers (keys included), enqueues on
 * `hip_stream` (NULL = default stream) and returns after that stream has been synchronised; the host entry copies in, runs the same device path
 * and copies out.  All work of a call runs on that one stream.
 *
 * The samples.  Ray i has samples k = sample_first .. sample_first + spp - 1.  Sample k uses the RNG contract's generators of pixel
 *   index key_i = keys[i] (keys == NULL: key_i = i) and sample k: both are seeded with sample_seed(seed, key_i, k); the sample's own generator
 *   (`rnd`, from which a frame draws its pixel jitter) is then advanced by rng_skip words, and the shaders' (getRandomGen(), from which a frame
 *   draws the lens sample) starts at word 0.  The sample runs the scene's integrator on Ray{origin_i, dir_i, depth 0}.  raytrace() draws nothing
 *   from `rnd`, so rng_skip does not change a Whitted colour.
 * The result.  rgb[i][3] = (the FP32 sum of the sample colours, in sample order) / (float)spp: the frame's resolve (k_pt_resolve_terms).
 *   Reproducing a frame: a non-DOF Whitted sample is the camera ray through its film position with rng_skip 0, sample_first = the sample and
 *   key = y * frameWidth + x; a non-DOF path-traced sample the same with rng_skip 2 (the frame draws two jitter floats from `rnd`, then traces).
 * Not applied: camera, AA offsets, jitter, lens, stereo eyes, saturation (the reference applies it only in the stereo blend, main.cpp:306-317) and
 *   bucket selection.  The caller's ray is the sample's ray.  Directions are used as given, as frayhip_trace_rays uses them.
 * Degenerate rays (frayhip_trace_rays' rule: a non-finite component, or a direction whose squared length is 0 or overflows) are answered without
 *   tracing: rgb = 0, and their samples are not counted.  With maxTraceDepth < 0 every ray is black, as in the frame.
 * Arithmetic is always the reference's (exact).  Option fp_contract does not apply: its kernels assume unit directions (dev_trace.hpp), and the
 *   caller's need not be.  Speculative glossy fans are not used either.  Neither changes a result.
 * A query changes no option of the scene and none of the last frame's figures that frayhip_scene_get_option reports (whitted_path,
 *   contracted_launches, the fan counts, ...).
 * flags: FRAYHIP_FRAME_STATS selects the counting kernel variants.  *st may be NULL; when given it holds ms_total, ms_kernels, samples (the samples
 *   traced, with or without the flag), ms_trace / trace_launches (k_whitted_rays, or k_pt_bounce) and ms_shadow / shadow_launches (k_pt_shadow),
 *   and with the flag the work counters closest_rays, shadow_rays, node_tests, kd_inner_visits, leaf_refs, tri_tests, prim_tests, smooth_hits,
 *   texture_fetches.  The alg_* fields stay 0.
 * FRAYHIP_E_ARG, before the device is touched, with the reason in frayhip_last_error(): a NULL scene, request or rgb; n < 0 or n > INT32_MAX, or a
 *   NULL origin / dir with n > 0; spp < 1, sample_first < 0, or sample_first + spp > INT32_MAX; rng_skip outside 0..8; a device pointer that is
 *   misaligned (8 bytes for origin / dir, 4 for keys and rgb); any call on a scene whose frame is being rendered (from inside its progress
 *   callback).  n == 0 is a successful no-op.
 * FRAYHIP_E_UNSUPPORTED: the envelope of frames (Whitted shade() nesting deeper than 40, a generator past 227 words, a CsgOp operand with more
 *   intersections than the device path holds), and path tracing with maxTraceDepth >= 20: a frame's path generators then outgrow their
 *   registers (8 + 10 * (maxTraceDepth + 2) > 227 words) and the kernel that carries them derives their seeds from the frame's pixels.
 * Why rng_skip stops at 8: a frame reserves 8 words per sample for the camera when it picks its generator form, so a skip of up to 8 never
 *   changes which form a scene uses. */
typedef struct frayhip_shade_request {
    uint32_t seed;          /* contract seed, as frayhip_frame.seed (the reference uses 42)                       */
    int32_t  spp;           /* samples per ray, >= 1                                                               */
    int32_t  sample_first;  /* index of the first sample, >= 0; sample_first + spp <= INT32_MAX                    */
    int32_t  rng_skip;      /* words of the sample's own generator discarded before the trace, 0..8                */
    int32_t  flags;         /* FRAYHIP_FRAME_STATS                                                                 */
    int32_t  _pad;
    const uint32_t* keys;   /* n keys (host memory for the host entry, device memory for _device); NULL: key = ray index */
} frayhip_shade_request;

int  frayhip_shade_rays(frayhip_scene* s, int64_t n, const double* origin, const double* dir,
                        const frayhip_shade_request* r, float* rgb, frayhip_stats* st);
int  frayhip_shade_rays_device(frayhip_scene* s, int64_t n, const double* d_origin, const double* d_dir,
                               const frayhip_shade_request* r, float* d_rgb, void* hip_stream, frayhip_stats* st);

/* ---- adaptive frames (per-pixel sample counts for a path-traced frame) ---------------------------------------------------------------------
 * A path-traced, mono frame (settings.gi on, camera.stereoSeparation == 0) over the call's buckets (frame.bucket_first / bucket_stride, as
 * frayhip_render) in which every pixel takes only as many samples as its own noise estimate asks for.  spp is the frame's sample count
 * (main.cpp:395-400: the largest of 5 with wantAA or 1, numDOFSamples with DOF, numPaths); min_spp is the caller's, 2 <= min_spp <= spp.
 *
 * Ladder.  Sample counts go up r_0 = floor(min_spp / 2), r_1 = min_spp, r_{j+1} = min(2 * r_j, spp), ending at the first rung equal to spp.
 *   Every pixel runs rungs 0 and 1.  Sample i of a pixel is seeded independently of the frame's spp and the per-pixel FP32 sum runs in sample
 *   order, so a pixel's mean after r samples IS that pixel of the frame of r samples per pixel, bit for bit.
 * Error at rung j >= 1.  m = the pixel's mean after r_j samples, h = its mean after r_{j-1} samples (FP32 triples).  In double, no contraction,
 *   each FP32 operand widened to double first:
 *       num = (|m.r - h.r| + |m.g - h.g|) + |m.b - h.b|
 *       den = err_floor + ((m.r + m.g) + m.b)
 *       err = num / den
 *   Below the cap r_j = 2 r_{j-1}, so m - h is half the difference of two independent half-estimates: the two-buffer noise estimate without
 *   a second buffer.
 * Stopping.  A pixel stops at the first rung j >= 1 where err <= threshold, or where r_j == spp.  A NaN error never stops a pixel early.
 * Outputs, per pixel of the call's buckets: rgb[3] = the mean at the pixel's final rung (= frayhip_render of the same scene with spp := r_final,
 *   bit for bit); spp_out = r_final; err_out = (float)err at the final rung.  Pixels outside the call's buckets are untouched in all three
 *   buffers.  The decision is per pixel (no neighbourhood), so calls over disjoint buckets make up the whole frame's call exactly.
 * Arithmetic: always the exact kernels.  Option fp_contract does not apply (its kernels are never launched, and "contracted_launches" reads 0
 *   afterwards): with fp_contract = 1 the outputs equal those with fp_contract = 0.
 * Black frames: with maxTraceDepth < 0 every pixel is 0, with spp_out = min_spp and err_out = 0 (rungs = 2).
 * Batching: results do not depend on frame.spp_chunk (the most samples per pixel in one batch; 0 = auto), option pt_budget_mib or pt_lanes,
 *   nor on the order of the active pixels.  All work of a call runs on one stream.
 * frame: mode must be FRAYHIP_MODE_RENDER; FRAYHIP_FRAME_STATS selects the counting kernel variants.  *st may be NULL; when given it holds
 *   ms_total, ms_kernels, samples (== a->samples, with or without the flag), ms_trace / trace_launches (k_pt_bounce), ms_shadow /
 *   shadow_launches (k_pt_shadow) and, with the flag, the work counters.  The alg_* fields stay 0.
 * rgb is required (W*H*3); spp_out (W*H int32) and err_out (W*H float) may be NULL.  The _device entry takes DEVICE pointers and follows
 *   frayhip_render_device's stream contract (enqueued on hip_stream, NULL = default stream; returns after it has been synchronised).
 * FRAYHIP_E_ARG, before the device is touched, with the reason in frayhip_last_error(): a NULL scene, frame, request or rgb; mode !=
 *   FRAYHIP_MODE_RENDER; min_spp < 2 or min_spp > spp; a NaN or negative threshold; an err_floor that is not finite and positive; bucket
 *   arguments that frayhip_render refuses; a call on a scene whose frame is being rendered.
 * FRAYHIP_E_UNSUPPORTED: gi off (Whitted); stereo; long generators (8 + 10 * (maxTraceDepth + 2) > 227 words, i.e. maxTraceDepth >= 20),
 *   refused for frayhip_shade_rays' reason: their kernel derives a path's seed from the frame's dense pixel slots. */
typedef struct frayhip_adaptive {
    int32_t  min_spp;        /* in:  2 <= min_spp <= the frame's spp                                  */
    int32_t  _pad;
    double   threshold;      /* in:  >= 0 (+inf allowed: every pixel stops at min_spp)               */
    double   err_floor;      /* in:  > 0 and finite: the error's denominator floor                    */
    int32_t  rungs;          /* out: ladder rungs run, r_0 included                                   */
    int32_t  _pad2;
    uint64_t samples;        /* out: sum of spp_out over the call's pixels                            */
} frayhip_adaptive;

int  frayhip_render_adaptive(frayhip_scene* s, const frayhip_frame* f, frayhip_adaptive* a,
                             float* rgb, int32_t* spp_out, float* err_out, frayhip_stats* st);
int  frayhip_render_device_adaptive(frayhip_scene* s, const frayhip_frame* f, frayhip_adaptive* a,
                                    float* d_rgb, int32_t* d_spp, float* d_err, void* hip_stream, frayhip_stats* st);

/* ---- resumable frames (samples added to a frame that is already rendered) ---------------------------------------------------------------------
 * The running per-pixel sum of a frame as a caller-held buffer, the STATE: W*H rows of FRAYHIP_ACCUM_CHANNELS floats, row-major, one 16-byte row
 * per pixel: sum.r, sum.g, sum.b, m2.  A call renders samples sample_first .. sample_first + sample_count - 1 of every pixel of the call's buckets
 * (frame.bucket_first / bucket_stride, as frayhip_render) into it, under the scene's current view, settings and integrator.  Pixels of other
 * buckets are untouched in accum, rgb and noise.
 *
 * Which samples.  Sample i of a pixel is sample i of any frayhip_render frame of this scene and frame.seed -- film position (AA offset or
 *   jitter), lens and both generators -- whatever the frame's own sample count (numPaths, numDOFSamples), which plays no part.  One exception: a
 *   frame whose samples are not jittered (Whitted without DOF) has only its 1 (or, with wantAA, 5) samples, and sample_first + sample_count
 *   beyond them is FRAYHIP_E_ARG.  For jittered frames the bound is 2^24, so that (float)N is exact.
 * State, per pixel, all FP32, in sample order, without contraction.  c_i = the colour the frame's resolve adds for sample i: a path's terms
 *   folded innermost first (term[n-1], then term[k] + result for k = n-2 .. 0); for a stereo frame the blended eyes.  For each sample in order:
 *       sum = sum + c_i                       (per channel)
 *       l   = ((c_i.r + c_i.g) + c_i.b) / 3.0f
 *       m2  = m2 + l * l
 *   With sample_first == 0 the buffer's contents are ignored and the row starts as the frame's sum does, at (0, 0, 0, 0).  With sample_first > 0
 *   the buffer is taken as the state of samples 0 .. sample_first - 1: the caller's word is trusted.
 * Outputs, N = samples_done.  rgb (optional, W*H*3) = sum / (float)N per channel, the frame's own division: after samples 0 .. N-1 it IS
 *   frayhip_render with N samples per pixel, bit for bit, however the samples were cut into calls and batches.  noise (optional, W*H)
 *   estimates the variance of the luminance of the mean:
 *       lbar  = ((rgb.r + rgb.g) + rgb.b) / 3.0f
 *       v     = max(0, m2 / (float)N - lbar * lbar)
 *       noise = v / (float)(N - 1)            for N >= 2
 *       noise = lbar * lbar                   for N == 1: one sample knows nothing about its spread, so it is "as uncertain as the value"
 *   It is in rgb's domain, not demodulated: it goes into frayhip_denoise_signal (as `variance`, with rgb as `signal`) with demodulate = 0.
 * Progress and cancel.  p may be NULL.  With it the contract of frayhip_render_progressive holds (callback thread, pacing, cancel latency);
 *   previews are the running mean of ALL samples the state holds, and samples_done / samples_total in frayhip_progress count from sample 0.
 *   After a cancel the call returns FRAYHIP_E_CANCELLED, the state holds exactly the resolved samples, r->samples_done says how many, rgb
 *   and noise are made from them, and the next call continues from there.
 * Behaves as a frame.  frame.spp_chunk is the batch size (0 = as many as the queue budget holds); the options pt_lanes, pt_budget_mib,
 *   fp_contract, skip_null_segments, segment_planes, speculate_fans and fused_whitted_max act as in frayhip_render, and none of the first two
 *   changes a bit of the state.  The last frame's figures (frayhip_scene_get_option) are updated as a frame updates them.  With
 *   FRAYHIP_FRAME_STATS *st counts this call's samples only, so the counters of calls that tile [0, N) add up to the one-shot frame's.
 * Seed table.  A call with sample_first == 0 uses the table as a frame does; one with sample_first > 0 neither reads nor alters it (its planes
 *   would never be read again) and seeds into the workspace.
 * Black frames.  With maxTraceDepth < 0 the call adds +0 for each sample.
 * Nothing a frame supports is refused: mono and stereo, DOF, long generators and Cube / CSG scenes all take this path.
 * The host entry copies accum in only when sample_first > 0 (or when the call renders a subset of the buckets, with rgb and noise, so that the
 *   other pixels keep their values) and copies accum, rgb and noise out.  The _device entry takes DEVICE pointers -- d_accum 16-byte aligned, the
 *   others 4-byte aligned -- and follows frayhip_render_device's stream contract.
 * FRAYHIP_E_ARG, before the device is touched, with the entry's name in frayhip_last_error(): a NULL scene, frame, request or accum; mode !=
 *   FRAYHIP_MODE_RENDER; sample_first < 0, sample_count < 1, or their sum past the bound above; bucket arguments that frayhip_render refuses;
 *   a NaN preview_ms; an output overlapping accum or another output; a misaligned device pointer; a call on a scene whose frame is being
 *   rendered. */
#define FRAYHIP_ACCUM_CHANNELS 4   /* per pixel, row-major: sum.r, sum.g, sum.b, m2 -- one 16-byte row */
typedef struct frayhip_samples {
    int32_t sample_first;    /* in:  index of the first sample to render, >= 0                        */
    int32_t sample_count;    /* in:  how many, >= 1                                                   */
    int32_t samples_done;    /* out: samples per pixel the state holds after the call                 */
    int32_t _pad;
} frayhip_samples;

int  frayhip_render_samples(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p,
                            float* accum, float* rgb, float* noise, frayhip_stats* st);
int  frayhip_render_samples_device(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p,
                                   float* d_accum, float* d_rgb, float* d_noise, void* hip_stream, frayhip_stats* st);

/* ---- component frames (direct and indirect light as two resumable states) ---------------------------------------------------------------------
 * For a mono, path-traced frame (settings.gi on, stereoSeparation == 0): frayhip_render_samples with the samples' colours kept apart as direct
 * and indirect light, at no extra ray.  Sample i of a pixel is a list of terms t[0 .. n-1], n >= 1 -- bounce b of its path writes term b -- and
 * the frame's resolve adds their fold, innermost first.  Here, per channel, all FP32, without contraction:
 *       d_i = t[0]                            as it is stored, no addition
 *       n_i = fold(t[1 .. n-1])               result = (0, 0, 0); then result = t[k] + result for k = n-1 .. 1; (0, 0, 0) when n == 1
 *   so c_i == d_i + n_i: one FP32 addition per channel gives the sample colour of frayhip_render / frayhip_render_samples, bit for bit.
 *   Direct light is the next-event contribution at the camera ray's hit, or the colour of the light or the environment the camera ray sees
 *   itself, or black where the reference returns black at depth 0.  Indirect light is everything a later bounce contributes; a first hit on a
 *   mirror or on glass has direct light 0.
 * Two states, each laid out and accumulated as frayhip_render_samples' state (rows {sum.r, sum.g, sum.b, m2}, FRAYHIP_ACCUM_CHANNELS floats; the
 *   sum in sample order, l = ((r + g) + b) / 3.0f, m2 = m2 + l * l): accum_direct takes the d_i, accum_indirect the n_i.  The outputs per state
 *   are that entry's: rgb_* = sum / (float)N and noise_* (the formula above, of that component's luminance, in rgb's domain: it goes into
 *   frayhip_denoise_signal with demodulate = 0).  All four are optional.  rgb_direct after samples 0 .. N-1 is the value of the N-sample frame
 *   of the same scene with maxTraceDepth = 0.
 * The contract is frayhip_render_samples' throughout: which samples, buckets (pixels outside the call's buckets are untouched in all six
 *   buffers), sample_first > 0 trusting the caller's states, the host entry's copy-in rule (per state), the seed table, spp_chunk, the options and
 *   the last frame's figures, *st, the _device entry's pointers (both states 16-byte aligned) and stream contract, long generators
 *   (maxTraceDepth >= 20) and black frames (maxTraceDepth < 0: +0 per sample into both states, the samples counted once).  p's callback and
 *   cancel work as there; after a cancel both states hold the same resolved samples and r->samples_done says how many.
 * The differences:
 *   Previews are not offered: a p with preview_ms >= 0 is FRAYHIP_E_ARG, and every callback has preview == 0 and rgb == NULL.
 *   FRAYHIP_E_ARG also answers a NULL or misaligned second state, and any overlap among the six buffers.
 *   FRAYHIP_E_UNSUPPORTED: settings.gi off (a Whitted frame has no term list) and stereo frames (their resolve blends per-sample eye colours).
 *   Option fp_contract: a sample's first closest hit and its shading never run the contracted kernels, and of its next-event segments the
 *   contracted any-hit kernel decides only visible / occluded, so the direct state is unchanged bit for bit unless such an answer flips (none
 *   does in any frame of the tests); the indirect state carries the option's documented bound. */
int  frayhip_render_components(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p,
                               float* accum_direct, float* accum_indirect, float* rgb_direct, float* rgb_indirect,
                               float* noise_direct, float* noise_indirect, frayhip_stats* st);
int  frayhip_render_components_device(frayhip_scene* s, const frayhip_frame* f, frayhip_samples* r, const frayhip_progressive* p,
                                      float* d_accum_direct, float* d_accum_indirect, float* d_rgb_direct, float* d_rgb_indirect,
                                      float* d_noise_direct, float* d_noise_indirect, void* hip_stream, frayhip_stats* st);

/* ---- sample maps (per-pixel sample counts on a resumable frame) ---------------------------------------------------------------------------------
 * frayhip_render_samples gives every pixel of the call's buckets the same number of samples; here the caller says how many more each pixel gets.
 * For a mono, path-traced frame (settings.gi on, camera.stereoSeparation == 0).  accum is frayhip_render_samples' state (W*H rows {sum.r, sum.g,
 * sum.b, m2}); count (W*H int32, in/out) says how many samples each pixel's row holds; add (W*H int32, in) how many more it gets.
 *
 * Per pixel p of the call's buckets (frame.bucket_first / bucket_stride, as frayhip_render), n = count[p], a = add[p]:
 *   a > 0   the pixel's samples n .. n + a - 1 -- the (seed, pixel, sample) samples frayhip_render and frayhip_render_samples trace -- are added to
 *           its row in sample order with that entry's arithmetic (a sample's terms folded innermost first, sum = sum + c, l = ((c.r + c.g) + c.b)
 *           / 3.0f, m2 = m2 + l * l).  With n == 0 the row's contents are ignored and it starts at (0, 0, 0, 0).  Then count[p] = n + a.
 *   a == 0  row and count are untouched.
 *   After the call the row IS the row frayhip_render_samples produces for samples 0 .. N-1, N = count[p], bit for bit, however the samples were
 *   cut into map calls, uniform calls and batches; the caller's word about what the row held before is trusted, as there.
 * rgb (W*H*3) and noise (W*H), both optional, are written for EVERY pixel of the call's buckets, with frayhip_render_samples' formulas and the
 *   pixel's own N: rgb = sum / (float)N (= frayhip_render at N samples per pixel, bit for bit) and the noise estimate given there.  A pixel with
 *   N == 0 knows nothing: it gets rgb (0, 0, 0) and noise 0 -- give every pixel a sample before the frame is shown or denoised.
 * Pixels outside the call's buckets are untouched in accum, count, rgb and noise, and their add is not read.
 * Independence: no bit depends on frame.spp_chunk (the most samples of a pixel in one batch; 0 = auto), on the options pt_budget_mib or
 *   pt_lanes, on the order or composition of waves, or on the handle's call history.  All work of a call runs on one stream.
 * Arithmetic: always the exact kernels, as adaptive frames: option fp_contract does not apply and "contracted_launches" reads 0 afterwards.
 * Seed table: neither read nor altered, as a frayhip_render_samples call with sample_first > 0.
 * Black frames: with maxTraceDepth < 0 the call adds +0 for each sample, and the samples are counted.
 * A call whose add is zero in all its pixels launches no tracing kernel and returns FRAYHIP_OK with samples == 0 (rgb and noise are still written).
 * How it runs: layers of at most cn samples per pixel (cn from the work budget or spp_chunk).  The layer at offset k0 lists the pixels with
 *   add > k0; entry i takes min(cn, add_i - k0) samples, and an exclusive scan of these gives every entry a contiguous range of path slots, so a
 *   batch is dense: no path is traced for a sample nobody asked for, and the number of launches does not grow with the number of distinct values
 *   in add.  Kernels: k_map_init, k_map_count / k_compact_scan / k_map_offsets, k_map_expand, k_seed_map, k_pt_init_map, the frame's k_meta_dense,
 *   k_pt_bounce / k_scan / k_pt_shadow, k_map_fold, k_map_resolve, k_map_flag / k_compact_*, k_map_finish (samplemap_variant.hip).
 * *st as frayhip_render_adaptive: ms_total, ms_kernels, samples (== m->samples, with or without FRAYHIP_FRAME_STATS), ms_trace / trace_launches,
 *   ms_shadow / shadow_launches and, with the flag, the work counters of this call's samples only.
 * The host entry copies accum, count and add in (rgb and noise too when the call renders a subset of the buckets) and accum, count, rgb and noise
 *   out.  The _device entry takes DEVICE pointers -- d_accum 16-byte aligned, the others 4-byte -- and follows frayhip_render_device's stream
 *   contract.
 * FRAYHIP_E_ARG, with the entry's name in frayhip_last_error(): a NULL scene, frame, request, accum, count or add; mode != FRAYHIP_MODE_RENDER;
 *   bucket arguments that frayhip_render refuses; any overlap among the five buffers; a misaligned device pointer; a call on a scene whose frame
 *   is being rendered; and any add[p] < 0, count[p] < 0 or count[p] + add[p] > 2^24 in the call's buckets.  The host entry checks the planes
 *   before it touches the device; the device entry checks them in its first kernel and returns with nothing written.
 * FRAYHIP_E_UNSUPPORTED: gi off (Whitted), stereo and long generators (maxTraceDepth >= 20), for frayhip_render_adaptive's reasons.
 * Not offered: a sample budget normalised over the frame, progress callbacks and cancel (component states under a map: see below).
 *
 * Component states under a map (frayhip_render_components_map): the call above for the two states of frayhip_render_components, accum_direct and
 *   accum_indirect, with ONE count plane -- the two states always hold the same samples.  The tracing is the map call's own; only the end differs:
 *   a sample's term 0 is added, as stored, to the direct row and the fold of its terms 1 .. n-1 (begun at (0, 0, 0), innermost first; (0, 0, 0) when
 *   n == 1) to the indirect row, both in sample order with the arithmetic above (k_map_fold_split, k_map_resolve_split; k_map_finish_split writes
 *   count += add once and each component's rgb and noise from its own row with the pixel's N; k_map_black_split answers maxTraceDepth < 0: one +0
 *   into both rows, the samples counted once).  After the call each state's row of a pixel holding N samples IS the row frayhip_render_components
 *   leaves for samples 0 .. N-1, bit for bit.  rgb_direct, rgb_indirect, noise_direct and noise_indirect are all optional; a pixel with N == 0
 *   gets zeros in all of them.  Everything else is the contract above: buckets (pixels outside are untouched in all seven written buffers and
 *   their add is not read), a == 0, n == 0 (both rows ignored), the host entry's copy-in rule per buffer, independence, exact kernels only, the
 *   seed table, *st and m.  FRAYHIP_E_ARG as above with the entry's name, and also a NULL or (device) misaligned second state -- both states
 *   16-byte aligned -- and any overlap among the eight buffers ("X must not overlap Y", with the argument names below).
 *   FRAYHIP_E_UNSUPPORTED as above. */
typedef struct frayhip_samples_map {
    uint64_t samples;        /* out: sum of add over the pixels the call rendered                               */
    int32_t  count_min;      /* out: smallest and largest count after the call among the pixels of the call's   */
    int32_t  count_max;      /*      buckets (0, 0 when the call has no pixel)                                  */
} frayhip_samples_map;

int  frayhip_render_samples_map(frayhip_scene* s, const frayhip_frame* f, frayhip_samples_map* m, float* accum, int32_t* count,
                                const int32_t* add, float* rgb, float* noise, frayhip_stats* st);
int  frayhip_render_samples_map_device(frayhip_scene* s, const frayhip_frame* f, frayhip_samples_map* m, float* d_accum, int32_t* d_count,
                                       const int32_t* d_add, float* d_rgb, float* d_noise, void* hip_stream, frayhip_stats* st);
int  frayhip_render_components_map(frayhip_scene* s, const frayhip_frame* f, frayhip_samples_map* m, float* accum_direct, float* accum_indirect,
                                   int32_t* count, const int32_t* add, float* rgb_direct, float* rgb_indirect, float* noise_direct,
                                   float* noise_indirect, frayhip_stats* st);
int  frayhip_render_components_map_device(frayhip_scene* s, const frayhip_frame* f, frayhip_samples_map* m, float* d_accum_direct,
                                          float* d_accum_indirect, int32_t* d_count, const int32_t* d_add, float* d_rgb_direct,
                                          float* d_rgb_indirect, float* d_noise_direct, float* d_noise_indirect, void* hip_stream,
                                          frayhip_stats* st);

/* The map from a state (scene-free, one kernel: k_sample_map, samplemap.hip): how many more samples each pixel needs before the standard error
 * of its mean's luminance is `tolerance` times that luminance (or times lum_floor, for a dark pixel).  FP32 throughout, no contraction
 * (tests/sample_map_ref.py restates it in numpy).  Per pixel, N = count[p], over all W*H pixels:
 *       N >= max_count:  add = 0
 *       N <  min_count:  target = min_count
 *       else  mean = sum / (float)N;  lbar = ((mean.r + mean.g) + mean.b) / 3.0f
 *             v = fmaxf(0, m2 / (float)N - lbar * lbar);  noise = N >= 2 ? v / (float)(N - 1) : lbar * lbar
 *             ref = fmaxf(lbar, lum_floor);  t = tolerance * ref;  need = ceilf((float)N * (noise / (t * t)))
 *             target = need <= (float)max_count ? max(N, (int)need) : max_count       (a NaN need asks for max_count: never stops a pixel early)
 *             target = min(target, grow * N)
 *       add = min(min(target, max_count) - N, max_add)
 *   grow bounds how far one pass trusts an estimate made from N samples; 2 is a maintainer's choice, not a measurement.
 * pixels = the number of pixels with add > 0 and samples = the sum of add, over all W*H pixels: a caller who renders a bucket share ignores the
 *   rest, as frayhip_render_samples_map does.
 * Device pointers: accum 16-byte aligned, count and add 4-byte; the stream contract and *st (ms_total, ms_kernels) as frayhip_change_frame_device.
 * FRAYHIP_E_ARG, before the device is touched: width or height < 1 or W*H > 2^30; a NULL pointer; a tolerance or lum_floor that is not finite and
 *   > 0; min_count < 1, max_count < min_count or > 2^24; max_add < 1; grow outside 2..16; overlapping buffers; a misaligned device pointer.
 * The map from a PAIR of component states (frayhip_sample_map_pair; the same kernel, k_sample_map<PAIR>; tests/sample_map_pair_ref.py restates it):
 *   one count plane, the same parameters.  For each component c in {direct, indirect}: mean_c, lbar_c, v_c and noise_c as above from that state's
 *   row and the pixel's N; then lbar = lbar_d + lbar_i and noise = noise_d + noise_i, and everything from ref = fmaxf(lbar, lum_floor) on, and
 *   the N >= max_count and N < min_count cases, are unchanged.  Adding the two variances ignores the covariance of a sample's direct and indirect
 *   light: a maintainer's choice, not a measurement -- the split filter treats the components as separate signals, and their errors add in the
 *   final sum.  FRAYHIP_E_ARG as above, and a NULL or (device) misaligned second state and any overlap among the four buffers. */
/* A struct tag without a typedef, as frayhip_denoise. */
struct frayhip_sample_map {
    float    tolerance;      /* in:  relative standard error aimed at; finite and > 0, default 0.05                      */
    float    lum_floor;      /* in:  the luminance a dark pixel's error is measured against; finite and > 0, default 0.01 */
    int32_t  min_count;      /* in:  every pixel is brought to this count first; 1 <= min_count <= max_count, default 4   */
    int32_t  max_count;      /* in:  no pixel goes past it; <= 2^24; no default (0): the caller sets it                   */
    int32_t  max_add;        /* in:  the most one map gives a pixel; >= 1, default 2^24                                   */
    int32_t  grow;           /* in:  a pixel's target is at most grow * N; 2..16, default 2                               */
    uint64_t pixels;         /* out: pixels with add > 0                                                                  */
    uint64_t samples;        /* out: the sum of add                                                                       */
};
int  frayhip_sample_map_defaults(struct frayhip_sample_map* p);
int  frayhip_sample_map(int width, int height, const float* accum, const int32_t* count, struct frayhip_sample_map* p, int32_t* add,
                        frayhip_stats* st);
int  frayhip_sample_map_device(int width, int height, const float* d_accum, const int32_t* d_count, struct frayhip_sample_map* p,
                               int32_t* d_add, void* hip_stream, frayhip_stats* st);
int  frayhip_sample_map_pair(int width, int height, const float* accum_direct, const float* accum_indirect, const int32_t* count,
                             struct frayhip_sample_map* p, int32_t* add, frayhip_stats* st);
int  frayhip_sample_map_pair_device(int width, int height, const float* d_accum_direct, const float* d_accum_indirect, const int32_t* d_count,
                                    struct frayhip_sample_map* p, int32_t* d_add, void* hip_stream, frayhip_stats* st);

/* The map under a frame-wide sample budget (frayhip_sample_map_budget; samplemap_budget.hip; tests/sample_map_budget_ref.py restates it).
 * Let A(tau)[p] be the add that frayhip_sample_map gives pixel p with tolerance = tau and every other parameter as passed
 * (frayhip_sample_map_pair's add when accum_indirect is not NULL), S(tau) the sum of A(tau)[p] over all W*H pixels, tau0 = p->tolerance and
 * taumax = FLT_MAX.  For a fixed pixel A(tau)[p] does not increase with tau: tolerance * ref, t * t, noise / (t * t), fn * (...) and ceilf are
 * each correctly rounded and so monotone, the integer steps after them are non-decreasing in need, and a row whose need is NaN or infinite
 * either asks for max_count at every tau or drops to a finite need once (fray_amd/csrc/samplemap_formula.hpp has the cases).  So S does not
 * increase either, and for a budget of any value:
 *   stage 0  S(tau0) <= budget:  add = A(tau0), frayhip_sample_map's plane bit for bit; tolerance_used = tau0, cap_used = -1.
 *   stage 1  else, S(taumax) <= budget:  tolerance_used = the smallest float tau in (tau0, taumax] with S(tau) <= budget (positive floats are
 *            ordered as their bit patterns); add = A(tolerance_used), cap_used = -1.  The one tolerance is raised until the frame can afford it:
 *            the relative error aimed at stays equal across pixels, and the caller learns which error the budget buys.
 *   stage 2  else -- the demand no tolerance removes (pixels below min_count, rows whose need is NaN or infinite) exceeds the budget:
 *            tolerance_used = taumax, cap_used = the largest integer c in [0, max_add] with sum min(A(taumax)[p], c) <= budget,
 *            add = min(A(taumax), cap_used).
 * p->pixels and p->samples describe the final plane (samples <= budget always); demand = S(tau0).  What stage 1 or stage 2 leaves unspent is
 * not handed out to other pixels: a stated limit.
 * Device code: one pass reduces every row to {noise, ref} in a workspace of the call and sums S(tau0) and S(taumax); eight search launches
 * evaluate 16 candidates each of the tolerance's bit pattern (stage 1) or of the cap (stage 2), each launch deriving its interval from the
 * totals of those before it in a control block in device memory; a last pass writes add.  Stream order is the only ordering, the call
 * synchronises once, whatever the data, and every total is an exact integer sum, so the answer depends on neither grid nor timing.
 * FRAYHIP_E_ARG, before the device is touched: everything frayhip_sample_map (accum_indirect NULL) or frayhip_sample_map_pair refuses, in their
 * order and words; a NULL b; b->reserved != 0.  Device pointers, the stream contract and *st as frayhip_sample_map_device. */
struct frayhip_sample_budget {
    uint64_t budget;          /* in:  the most samples the map may hand out, over all W*H pixels; any value        */
    uint64_t demand;          /* out: S(tau0), what the tolerance asked for                                        */
    float    tolerance_used;  /* out: the tolerance the plane was made with                                        */
    int32_t  cap_used;        /* out: the per-pixel cap of stage 2; -1: none                                       */
    int32_t  stage;           /* out: 0, 1, 2                                                                      */
    int32_t  reserved;        /* in:  0                                                                            */
};
int  frayhip_sample_map_budget(int width, int height, const float* accum, const float* accum_indirect /* NULL: one state */, const int32_t* count,
                               struct frayhip_sample_map* p, struct frayhip_sample_budget* b, int32_t* add, frayhip_stats* st);
int  frayhip_sample_map_budget_device(int width, int height, const float* d_accum, const float* d_accum_indirect /* NULL: one state */,
                                      const int32_t* d_count, struct frayhip_sample_map* p, struct frayhip_sample_budget* b, int32_t* d_add,
                                      void* hip_stream, frayhip_stats* st);

/* ---- feature frames (first-hit guides for a denoiser) ---------------------------------------------------------------------------------------
 * For every pixel of the call's buckets (frame.bucket_first / bucket_stride, as frayhip_render; other pixels untouched), the FP32 mean, in
 * sample order, of the first-hit features of the frame's own camera samples 0 .. n_samples - 1: sample i is the film position and the pinhole
 * or thin-lens ray that sample i of the MODE_RENDER frame traces, with the same seed (AA offsets for a Whitted frame with wantAA, jitter for gi
 * or DOF).  Ten floats per pixel, feat[(y * W + x) * FRAYHIP_FEAT_CHANNELS + k]:
 *   0..2 position, 3..5 normal, 6..8 albedo, 9 depth.
 * Per sample:
 *   node hit       position = IntersectionInfo.ip, normal = IntersectionInfo.norm after applyBumpMapping (not face-forwarded), depth = the
 *                  world distance; albedo = the colour the shader starts from: Lambert / Phong color (times the diffuse texture's sample),
 *                  Refl / Refr mult, Const color, Layered the blend of Layered::shade (shading.cpp:357-367) over its layers' albedos with the
 *                  same opacities (opacity textures sampled as there; a Layered shader inside two enclosing Layered shaders counts as black)
 *   rect-light hit position / normal as RectLight::intersect leaves them, depth = distance, albedo = the light's color
 *   miss           position, normal, depth 0; albedo = the environment's colour in the ray's direction (black without an environment)
 * Each feature is converted to float per sample and summed in float in sample order; the mean is sum / (float)n_samples.
 * maxTraceDepth < 0: every feature of the call's pixels is 0.
 * The call changes no option and none of the last frame's figures (contracted_launches, whitted_path, fan counters); fp_contract does not
 *   apply.  *st may be NULL; when given it holds ms_total, ms_kernels, samples (n_samples per pixel of the call) and ms_trace /
 *   trace_launches (k_features); with FRAYHIP_FRAME_STATS the counting kernel variant runs and the work counters are filled in.
 * The _device entry takes a DEVICE pointer (4-byte aligned) and follows frayhip_render_device's stream contract.
 * FRAYHIP_E_ARG, before the device is touched: a NULL scene, frame or feat; mode != FRAYHIP_MODE_RENDER; n_samples < 1 or > the frame's spp;
 *   bucket arguments that frayhip_render refuses; a misaligned device pointer; a call on a scene whose frame is being rendered.
 * FRAYHIP_E_UNSUPPORTED: stereo frames; path tracing with long generators (maxTraceDepth >= 20), refused for frayhip_shade_rays' reason --
 *   the feature pass never answers for rays other than the frame's. */
#define FRAYHIP_FEAT_CHANNELS 10   /* per pixel: position[3], normal[3], albedo[3], depth */
int  frayhip_render_features(frayhip_scene* s, const frayhip_frame* f, int n_samples, float* feat, frayhip_stats* st);
int  frayhip_render_features_device(frayhip_scene* s, const frayhip_frame* f, int n_samples, float* d_feat,
                                    void* hip_stream, frayhip_stats* st);

/* ---- specular feature frames (virtual-hit guides: mirrors and glass followed to the first non-specular hit) ------------------------------------
 * frayhip_render_features with every camera sample followed through Refl / Refr nodes.  Reflection::spawnRay and Refraction::spawnRay draw no
 * random number, so the chain behind a specular first hit is a function of the camera sample alone.  Same ten channels, so the filter and the
 * temporal entries take such a frame as they take a first-hit one.  Per camera sample, (o0, d0) being the sample's ray as frayhip_render_features
 * makes it: b = 0, T = 0.0 (FP64), M = I (3x3, FP64), no albedo product yet.
 *   specular step  taken when the closest hit of the current ray is a node whose OWN shader is Refl or Refr (a Layered shader is never
 *                  followed), b < max_bounces, and, for Refr, refract() did not return the zero vector (total internal reflection is not
 *                  followed).  The hit is finished and bumped as a first hit is; the next ray is the one Reflection / Refraction::spawnRay
 *                  returns (path-traced and Whitted frames alike: a glossy Refl is followed along its ideal direction); T = T + dist;
 *                  A = mult (first step) or A * mult; for Refl, with m the hit's normal after the bump,
 *                      u[i] = (M[i][0] m.x + M[i][1] m.y) + M[i][2] m.z,   M[i][j] = M[i][j] - (2 u[i]) m[j]          (M <- M (I - 2 m m^T));
 *                  Refr leaves M alone; b = b + 1.
 *   terminal       the first hit at which no step is taken: any node, a rect light, a miss, or a Refl / Refr hit at the bounce limit or under
 *                  total internal reflection.
 *                  b == 0        frayhip_render_features' row of this sample, bit for bit
 *                  b > 0, hit    position = o0 + d0 * (T + dist) (FP64: the point at the path's length along the primary ray, the mirror image
 *                                for one planar mirror), normal = M n with the row dots in the order above, n the normal the first-hit rule
 *                                stores; albedo = A * the first-hit rule's albedo at this hit; depth = T + dist
 *                  b > 0, miss   position, normal, depth 0 (the reflected sky takes no history, as a primary miss takes none);
 *                                albedo = A * the environment's colour in the last direction
 * Conversion to float, the sums in sample order and the division by n_samples are the feature channels'.  bounces (W*H floats, may be NULL in
 * both entries): (float)b per sample, reduced the same way.
 * max_bounces is 1 .. 8: it caps the loop; the kernel's state does not grow with it.
 * A scene none of whose nodes carries a Refl / Refr shader (looked up per call, so frayhip_scene_update's edits count) takes
 * frayhip_render_features' kernel and a zero plane.
 * Everything else is frayhip_render_features' contract: buckets, untouched pixels outside them (both outputs), options and last-frame figures
 * left alone, *st (with FRAYHIP_FRAME_STATS the work counters include every segment's search), the stream contract of the _device entry (both
 * device pointers 4-byte aligned), maxTraceDepth < 0 gives zeros in both outputs.
 * FRAYHIP_E_ARG, before the device is touched: what frayhip_render_features refuses, max_bounces outside 1 .. 8, a misaligned d_bounces,
 *   feat and bounces overlapping.  FRAYHIP_E_UNSUPPORTED: as there.
 * Not covered: motion frames through a chain (frayhip_render_features_motion carries first hits only, so a sequence under scene edits cannot
 *   use these guides), Layered glass (no Fresnel branch is chosen), glossy lobes, unfolding the normal through a refraction. */
#define FRAYHIP_SPECULAR_MAX_BOUNCES 8
int  frayhip_render_features_specular(frayhip_scene* s, const frayhip_frame* f, int n_samples, int max_bounces, float* feat,
                                      float* bounces /* W*H, may be NULL */, frayhip_stats* st);
int  frayhip_render_features_specular_device(frayhip_scene* s, const frayhip_frame* f, int n_samples, int max_bounces, float* d_feat,
                                             float* d_bounces /* W*H, may be NULL */, void* hip_stream, frayhip_stats* st);

/* ---- motion frames (where the first hit was in the previous frame's state of the scene) ------------------------------------------------------
 * frayhip_render_features with a second output for temporal accumulation across frayhip_scene_update: prev_T (a HOST pointer in both entries,
 * n_prev records, n_prev = the uploaded scene's node count) holds the transforms the scene's nodes had when the previous frame was rendered.
 * Node i is MOVED when any of the 21 doubles of prev_T[i] differs by bit pattern from the node's current {offset, m, invM}.
 * One traced pass writes both frames.  feat is what frayhip_render_features writes, bit for bit.  motion: eight floats per pixel, two 16-byte
 * rows, motion[(y * W + x) * FRAYHIP_MOTION_CHANNELS + k]:  0..2 P', 3 moved, 4..6 n', 7 zero.  Per sample:
 *   a node that is not moved   P' = the sample's ip, n' = its norm after the bump (the FP64 values the feature frame converts), moved = 0
 *   moved node i               P' = ((ip - off_now) * invM_now) * m_prev + off_prev      Transform::untransformPoint of the transform now, then
 *                              n' = (norm * invM_now) * m_prev                            transformPoint of the previous one; moved = 1
 *                              FP64, no contraction; each product is Vector * Matrix of matrix.h:53-60, (v.x m[0][j] + v.y m[1][j]) + v.z m[2][j];
 *                              n' is carried the way Node::intersect carries a normal (through m, not the inverse transpose) and not rescaled
 *   rect light, or miss        P', n' as the feature frame's position and normal, moved = 0
 * Each value is converted to float per sample, summed in float in sample order and divided by (float)n_samples, as the feature channels are
 * (so `moved` is the share of the pixel's samples that hit a moved node).  maxTraceDepth < 0: all zeros.
 * The previous {offset, m} and a moved byte per node go to a small device table that every call fills; the scene keeps its allocation, so
 * a call in a sequence allocates nothing.
 * Everything else is frayhip_render_features' contract: buckets, untouched pixels outside them, options and last-frame figures left alone, *st,
 * and the stream contract of the _device entry (both device pointers 4-byte aligned).
 * FRAYHIP_E_ARG, before the device is touched: what frayhip_render_features refuses, a NULL prev_T or motion, n_prev != the node count, a
 *   non-finite double in prev_T, feat and motion overlapping.  FRAYHIP_E_UNSUPPORTED: as there.
 * Not covered: moved lights; shadows and reflections of moved objects (their pixels' first hits did not move, so they ghost as in a static
 *   sequence; a specular feature frame follows STATIC reflections under camera motion, and has no motion frame); motion blur; vertex edits
 *   (frayhip_scene_update does not take them).  Moved lights and those shadows and reflections are what
 *   a change frame detects (frayhip_change_frame, frayhip_temporal_accumulate_adaptive below): the motion frame itself still follows a node's
 *   own pixels only. */
#define FRAYHIP_MOTION_CHANNELS 8   /* per pixel, two 16-byte rows: {P'.xyz, moved}, {n'.xyz, 0} */
int  frayhip_render_features_motion(frayhip_scene* s, const frayhip_frame* f, int n_samples, const frayhip_transform* prev_T, int n_prev,
                                    float* feat, float* motion, frayhip_stats* st);
int  frayhip_render_features_motion_device(frayhip_scene* s, const frayhip_frame* f, int n_samples, const frayhip_transform* prev_T, int n_prev,
                                           float* d_feat, float* d_motion, void* hip_stream, frayhip_stats* st);

/* ---- denoising (edge-avoiding a-trous wavelet filter, scene-free) --------------------------------------------------------------------------
 * A spatial SVGF-style filter of an rgb frame (W*H*3 floats) guided by a feature frame (W*H*FRAYHIP_FEAT_CHANNELS floats, as
 * frayhip_render_features writes it), FP32 throughout, no contraction.  Level k = 0 .. levels - 1 takes the taps q = p + 2^k (i, j),
 * i, j in -2..2 (j outer, i inner), skipping taps outside the image, with
 *     w   = h * w_n * w_z * w_a * w_l          h: the B3-spline (1/16, 1/4, 3/8, 1/4, 1/16) outer product
 *     w_n = max(0, n_p . n_q)^sigma_normal     on the normals scaled to unit length (a mean of several samples' normals is shorter);
 *                                              0 when exactly one of the two normals is zero, 1 when both are
 *     w_z = exp(-|z_p - z_q| / (sigma_depth * |grad z_p . (q - p)| + 1e-4))     z: depth; grad: central differences, one-sided at borders
 *     w_a = exp(-|a_p - a_q|_1 / sigma_albedo)
 *     w_l = exp(-|l_p - l_q| / (sigma_luminance * sqrt(max(0, var_p)) + 1e-4))  with rgb_half
 *     w_l = exp(-|l_p - l_q| / (sigma_luminance * 2^-k))                        without it
 * where l = (r + g + b) / 3 of the signal being filtered.  The level's output is c_p + sum(w (c_q - c_p)) / sum(w), which is
 * sum(w c_q) / sum(w) written so that a flat region stays exactly flat; the centre tap is always included.
 * Demodulation (demodulate = 1): the signal is rgb / max(albedo, 1e-3) per channel, and the last level multiplies max(albedo_p, 1e-3) back.
 * Noise estimate with rgb_half (the frame of the first half of rgb's samples): var_p = (l(rgb_p) - l(rgb_half_p))^2, both sides demodulated
 *   when demodulate is set, prefiltered with the 3x3 binomial kernel (1 2 1) x (1 2 1) / 16 normalised over the taps inside the image; after
 *   each level var_p := sum(w^2 var_q) / (sum w)^2.
 * Kernels: one launch that packs the guides, demodulates and prefilters the variance, then one launch per level (the last remodulates).
 * Buffers: out (W*H*3) must not overlap rgb, rgb_half or feat.  Work buffers are allocated per call (FRAYHIP_E_NOMEM when that fails).  The
 *   _device entry takes DEVICE pointers (4-byte aligned), enqueues on hip_stream and returns after synchronising it.
 * *st may be NULL; when given it holds ms_total and ms_kernels (the other fields are 0).
 * FRAYHIP_E_ARG, before the device is touched: width or height < 1 or W*H > 2^30; NULL rgb, feat, p or out; levels outside 1..10; demodulate
 *   not 0 or 1; a NaN, infinite or negative sigma, or sigma_luminance, sigma_depth or sigma_albedo equal to 0; out overlapping an input. */
/* A struct tag without a typedef: the name is also the entry point's, so C and C++ callers write `struct frayhip_denoise`. */
struct frayhip_denoise {
    int32_t levels;          /* a-trous iterations, step 2^k, k = 0..levels-1; 1..10, default 5                  */
    int32_t demodulate;      /* 1: filter rgb / max(albedo, 1e-3) per channel and multiply back (default 1)       */
    float   sigma_luminance; /* default 4                                                                          */
    float   sigma_normal;    /* exponent on max(0, n_p . n_q), default 128                                         */
    float   sigma_depth;     /* default 1                                                                          */
    float   sigma_albedo;    /* default 0.1                                                                        */
};
int  frayhip_denoise_defaults(struct frayhip_denoise* p);
int  frayhip_denoise(int width, int height, const float* rgb, const float* rgb_half, const float* feat,
                     const struct frayhip_denoise* p, float* out, frayhip_stats* st);
int  frayhip_denoise_device(int width, int height, const float* d_rgb, const float* d_rgb_half, const float* d_feat,
                            const struct frayhip_denoise* p, float* d_out, void* hip_stream, frayhip_stats* st);
/* The a-trous levels alone, on a signal and a variance the caller already has (frayhip_temporal_accumulate's outputs): signal (W*H*3) takes the
 * place of the signal k_dn_prepare derives from rgb, variance (W*H) that of the prefiltered estimate, and the levels run as they do with
 * rgb_half (w_l from the variance).  With demodulate the signal is taken as already demodulated, and the last level multiplies
 * max(albedo_p, 1e-3) back.  Guides, buffers, stream contract, *st and the FRAYHIP_E_ARG cases as frayhip_denoise (signal for rgb; a NULL
 * variance is refused; out must not overlap signal, variance or feat). */
int  frayhip_denoise_signal(int width, int height, const float* signal, const float* variance, const float* feat,
                            const struct frayhip_denoise* p, float* out, frayhip_stats* st);
int  frayhip_denoise_signal_device(int width, int height, const float* d_signal, const float* d_variance, const float* d_feat,
                                   const struct frayhip_denoise* p, float* d_out, void* hip_stream, frayhip_stats* st);

/* ---- temporal accumulation (the temporal stage of SVGF, scene-free) --------------------------------------------------------------------------
 * Reprojects the previous frame's accumulated colour and luminance moments into the current view through the feature frame's world positions,
 * rejects history that belongs to another surface, blends the new frame in, and hands frayhip_denoise_signal a per-pixel variance that comes
 * from the moments.  FP32 throughout, no contraction, every sum in the order written here (tests/temporal_ref.py restates it in numpy).
 *
 * frayhip_view: a camera as the kernel reads it.  frayhip_view_from_camera derives the frame of Camera::beginFrame (FP64, as the renderer
 * does) for a W x H film and rounds it to FP32.  getScreenRay(x, y) is parallel to front + right * tan_x * (2x/W - 1) + up * tan_y * (1 - 2y/H),
 * so a world point P lands on the film of that view at
 *     d  = P - pos;  zc = d . front;  xc = d . right;  yc = d . up              dots as (a0*b0 + a1*b1) + a2*b2
 *     fx = (xc / zc / tan_x + 1) * 0.5 * W
 *     fy = (1 - yc / zc / tan_y) * 0.5 * H                                       (behind the camera when zc <= 0)
 * Stereo and DOF play no part: the view is the centre camera's pinhole.  Host arithmetic only; no device is touched.
 * FRAYHIP_E_ARG: a NULL pointer, width or height < 1, a non-finite pos, yaw, pitch, roll, fov or aspectRatio, fov outside (0, 180),
 *   aspectRatio <= 0.
 *
 * History: FRAYHIP_HISTORY_CHANNELS = 12 floats per pixel, three 16-byte rows: {acc.rgb, N}, {P.xyz, m1}, {n.xyz, m2} -- the accumulated
 * signal and its sample count N (a float: a bilinear fetch may return a fractional count), the pixel's world position and unit normal (the
 * feature frame's normal scaled to unit length as the filter does; zero for a miss), and the running means m1, m2 of the signal's luminance
 * l = (r + g + b) / 3 and of its square.  hist_in and prev_view are both NULL (first frame) or both given; hist_out must not overlap hist_in
 * (the caller ping-pongs two buffers).  signal (W*H*3) is the accumulated colour in the filter's domain, variance (W*H) its luminance variance.
 *
 * Per pixel p:
 *  1. c = rgb_p, or rgb_p / max(albedo_p, 1e-3) per channel with demodulate; l = l(c); P, n, z from feat.  A pixel whose normal is exactly
 *     zero takes no history.
 *  2. P is projected into prev_view; u = fx - film_offset, v = fy - film_offset (film_offset: where inside pixel i its samples lie on average,
 *     0.5 for jittered samples, 0 for rays through the integer film position); x0 = floor(u), y0 = floor(v); the four taps (x0 + i, y0 + j),
 *     j outer, with the bilinear weights b.  A tap counts when it lies inside the image, its stored normal is not zero,
 *     n . n_q >= normal_min_dot, and its stored position lies on p's surface: |(P_q - P) . n| <= plane_tolerance * sqrt(d . d).  With
 *     sum(b) > 0 over the counted taps the history is sum(b h_q) / sum(b) for acc, m1, m2 and N; otherwise there is none.
 *  3. N = min(N_hist + 1, max_history), alpha = max(alpha_min, 1 / N); acc = h + alpha (c - h) per channel, likewise m1 with l and m2 with
 *     l * l.  Without history: acc = c, m1 = l, m2 = l * l, N = 1.
 *  4. Variance.  N >= variance_history: max(0, m2 - m1 * m1).  Below it, a second kernel over the finished hist_out: the 7 x 7 window around
 *     p, j outer, i inner, the taps inside the image whose stored normal is not zero, with n . n_q >= normal_min_dot and
 *     |(P_q - P) . n| <= plane_tolerance * z_p (for a p whose normal is zero: the taps whose normal is zero too); mean1, mean2 the unweighted
 *     means of their m1 and m2 (p's own m1, m2 when no tap counts); max(0, mean2 - mean1 * mean1) * (variance_history / N).
 * Kernels: k_tp_accumulate, then k_tp_variance when variance_history > 1.  No work buffers.  The _device entry takes DEVICE pointers (the two
 *   histories 16-byte aligned, the rest 4-byte; prev_view and p stay HOST pointers), enqueues on hip_stream and returns after synchronising it.
 * *st may be NULL; when given it holds ms_total and ms_kernels (the other fields are 0).
 * FRAYHIP_E_ARG, before the device is touched: width or height < 1 or W*H > 2^30; NULL rgb, feat, p, hist_out, signal or variance; one of
 *   hist_in / prev_view without the other; a view whose size is not W x H or with a non-finite field or a tan <= 0; demodulate not 0 or 1;
 *   max_history outside 1..4096; variance_history outside 1..4096; alpha_min outside 0..1; a non-finite film_offset; plane_tolerance negative
 *   or not finite; normal_min_dot outside -1..1; NaNs in any of them; an output overlapping an input or another output; a misaligned device
 *   pointer. */
#define FRAYHIP_HISTORY_CHANNELS 12
typedef struct frayhip_view {
    float   pos[3], right[3], up[3], front[3];   /* Camera::pos, rightDir, upDir, frontDir                                 */
    float   tan_x, tan_y;                        /* aspectRatio * m and m of Camera::beginFrame                            */
    int32_t width, height;
} frayhip_view;
int  frayhip_view_from_camera(const frayhip_camera* camera, int width, int height, frayhip_view* out);

/* A struct tag without a typedef, as frayhip_denoise. */
struct frayhip_temporal {
    int32_t demodulate;        /* 1: accumulate rgb / max(albedo, 1e-3), as the filter does (default 1)                      */
    int32_t max_history;       /* N is clamped to this; 1..4096, default 32                                                  */
    int32_t variance_history;  /* below this N the variance is the spatial estimate; 1..4096, default 4                      */
    float   alpha_min;         /* blend factor is max(alpha_min, 1 / N); 0..1, default 0.05                                  */
    float   film_offset;       /* pixel i was sampled around film x = i + film_offset; default 0.5                           */
    float   plane_tolerance;   /* |(P_q - P) . n| <= plane_tolerance * |P - pos_prev| keeps a tap; default 0.02              */
    float   normal_min_dot;    /* n . n_q >= this keeps a tap; default 0.9                                                   */
};
int  frayhip_temporal_defaults(struct frayhip_temporal* p);
int  frayhip_temporal_accumulate(int width, int height, const float* rgb, const float* feat, const frayhip_view* prev_view,
                                 const float* hist_in, const struct frayhip_temporal* p, float* hist_out, float* signal, float* variance,
                                 frayhip_stats* st);
int  frayhip_temporal_accumulate_device(int width, int height, const float* d_rgb, const float* d_feat, const frayhip_view* prev_view,
                                        const float* d_hist_in, const struct frayhip_temporal* p, float* d_hist_out, float* d_signal,
                                        float* d_variance, void* hip_stream, frayhip_stats* st);
/* The same with a motion frame (frayhip_render_features_motion; W*H*FRAYHIP_MOTION_CHANNELS floats, 16-byte aligned on the device): step 2
 * projects the pixel's P' into prev_view instead of P, and the taps are tested against P' and against n' scaled to unit length the way the
 * normal is (exactly zero stays zero): n' . n_q >= normal_min_dot and |(P_q - P') . n'| <= plane_tolerance * |P' - pos_prev|.  A pixel whose
 * current normal is exactly zero takes no history, and neither does one whose n' is exactly zero.  hist_out stores the CURRENT position and unit
 * normal; steps 1, 3 and 4 (k_tp_variance on the finished hist_out) are unchanged.  With a motion frame whose P', n' equal feat's position and
 * normal (nothing moved) every output bit is frayhip_temporal_accumulate's.  FRAYHIP_E_ARG: that entry's list, and a NULL, overlapping (with an
 * output) or misaligned motion. */
int  frayhip_temporal_accumulate_motion(int width, int height, const float* rgb, const float* feat, const float* motion, const frayhip_view* prev_view,
                                        const float* hist_in, const struct frayhip_temporal* p, float* hist_out, float* signal, float* variance,
                                        frayhip_stats* st);
int  frayhip_temporal_accumulate_motion_device(int width, int height, const float* d_rgb, const float* d_feat, const float* d_motion,
                                               const frayhip_view* prev_view, const float* d_hist_in, const struct frayhip_temporal* p,
                                               float* d_hist_out, float* d_signal, float* d_variance, void* hip_stream, frayhip_stats* st);

/* ---- split temporal accumulation (one history per light component) --------------------------------------------------------------------------
 * The stage above for two signals of one frame in one call: a frame's direct and indirect light (frayhip_render_components), each with a
 * history length of its own.  A shadow that moves across a static floor passes every surface test (the floor's first hit did not move) and so
 * stays in a single history for max_history frames; it lives in the direct component, which can take a short history while the indirect
 * component, the noisier one, keeps a long one.
 *
 * Split history: FRAYHIP_HISTORY_SPLIT_CHANNELS = 20 floats per pixel, five 16-byte rows:
 *     0 {accD.rgb, N_D}   1 {P.xyz, m1_D}   2 {n.xyz, m2_D}   3 {accI.rgb, N_I}   4 {m1_I, m2_I, +0.0f, +0.0f}
 * Rows 0-2 are, as they stand, the direct component's 12-channel history; the indirect component's is {row 3}, {P, m1_I}, {n, m2_I}.
 *
 * p_direct and p_indirect may differ in max_history, variance_history and alpha_min.  The fields that decide which taps count -- demodulate,
 * film_offset, plane_tolerance, normal_min_dot -- must agree bit for bit.  motion NULL: the arithmetic of frayhip_temporal_accumulate;
 * otherwise (a motion frame, as that entry takes it) the arithmetic of frayhip_temporal_accumulate_motion.  The library sets no default of
 * its own for the two lengths (frayhip_temporal_defaults fills either struct); the Python sequence and the CLI give the direct component a
 * max_history of 8 and leave the indirect one's at 32 where the caller names none.  The 8 is a maintainer's choice, not a measurement: a moved
 * shadow's residue after j frames is (1 - 1/8)^j of the step instead of (1 - 1/32)^j, and direct light at one next-event sample per path
 * sample is the less noisy component.
 *
 * The contract.  For every pixel the call produces two groups of outputs, each equal BIT FOR BIT to a call of the entry above:
 *   direct    rows 0-2 of hist_out, signal_direct and variance_direct are what frayhip_temporal_accumulate[_motion] returns for rgb_direct,
 *             p_direct and rows 0-2 of hist_in;
 *   indirect  {row 3}, {P, m1_I}, {n, m2_I} of hist_out, signal_indirect and variance_indirect are what it returns for rgb_indirect,
 *             p_indirect and the same three rows of hist_in.
 * It holds because the tap tests and the bilinear weights depend only on P, n, the view and the shared fields; everything per component is the
 * same expression, with every sum in the order written above, on the other component's inputs.
 * Kernels: k_tp_accumulate_split (the projection, the footprint and the surface tests once, each counted tap's five rows read once), then
 *   k_tp_variance_split when max(variance_history_D, variance_history_I) > 1 (the window's surface tests once; a component whose
 *   variance_history is 1 never takes the window).  No work buffers.  Device pointers, the stream contract and *st as above (the histories and
 *   the motion frame 16-byte aligned).
 * FRAYHIP_E_ARG, before the device is touched: the list above, per struct and per output (NULL rgb_direct, rgb_indirect, feat, p_direct,
 *   p_indirect or any of the five outputs; any output overlapping any input or another output), and a shared field that differs between
 *   p_direct and p_indirect. */
#define FRAYHIP_HISTORY_SPLIT_CHANNELS 20
int  frayhip_temporal_accumulate_split(int width, int height, const float* rgb_direct, const float* rgb_indirect, const float* feat,
                                       const float* motion, const frayhip_view* prev_view, const float* hist_in,
                                       const struct frayhip_temporal* p_direct, const struct frayhip_temporal* p_indirect, float* hist_out,
                                       float* signal_direct, float* signal_indirect, float* variance_direct, float* variance_indirect,
                                       frayhip_stats* st);
int  frayhip_temporal_accumulate_split_device(int width, int height, const float* d_rgb_direct, const float* d_rgb_indirect, const float* d_feat,
                                              const float* d_motion, const frayhip_view* prev_view, const float* d_hist_in,
                                              const struct frayhip_temporal* p_direct, const struct frayhip_temporal* p_indirect,
                                              float* d_hist_out, float* d_signal_direct, float* d_signal_indirect, float* d_variance_direct,
                                              float* d_variance_indirect, void* hip_stream, frayhip_stats* st);

/* ---- change frames (where the light a pixel receives changed between two states of the scene, scene-free) ------------------------------------
 * A frame is a function of (scene, view, seed) bit for bit, so what an edit changed can be detected exactly: render samples [0, n) of a view
 * and seed before the edit and the same samples after it (two frayhip_render_samples or frayhip_render_components states); a pixel none of
 * whose paths met anything that changed holds the same bits in both, and its difference is exactly zero.  frayhip_change_frame turns such a
 * pair into a per-pixel change in [0, 1], and frayhip_temporal_accumulate_adaptive shortens the history where it is not zero -- which covers
 * moved lights and the shadows and reflections of moved objects, whose pixels pass every surface test.  (Reflections of a static scene under
 * a moving camera need no change frame: frayhip_render_features_specular gives their pixels the guides of what the mirror shows.)
 *
 * accum_before, accum_after: two FRAYHIP_ACCUM_CHANNELS states (W*H*4 floats) that hold the same samples of the same seed and view; the
 * caller's word is trusted.  The sample count cancels, so the states' sums are used as they stand.  motion: a motion frame or NULL.  FP32
 * throughout, no contraction (tests/change_ref.py restates it in numpy).
 * Per texel q:  la = ((sum.r + sum.g) + sum.b) / 3.0f of accum_before, lb likewise of accum_after; m_q = fmaxf(la, lb), d_q = fabsf(lb - la);
 *   d_q = m_q = 0 when la or lb is not finite, when m_q <= 0, and, with a motion frame, when the texel's `moved` channel is not 0 (a moved
 *   node's own pixels are the motion frame's business).
 * Per pixel p:  sd = sum(d_q), sm = sum(m_q) over the (2 radius + 1)^2 window around p, j outer, i inner, skipping taps outside the image;
 *   change_p = sm > 0 ? fminf(1.0f, gain * (sd / sm)) : 0.0f.  No surface tests in the window: a shadow crosses object edges.
 * radius 3 and gain 1 are a maintainer's choice, not a measurement.
 * Kernel: k_ch_frame, one launch; a 16x16 block stages the (d, m) pairs of the 22x22 texels its windows can reach in LDS (each state row read
 *   once, as a float4), then each thread sums its window from the tile.  No work buffers.  Device pointers: both states and the motion frame
 *   16-byte aligned, change 4-byte; the stream contract and *st as frayhip_temporal_accumulate_device.
 * FRAYHIP_E_ARG, before the device is touched: width or height < 1 or W*H > 2^30; a NULL pointer other than motion; radius outside 0..3; a
 *   gain that is NaN, infinite or <= 0; change overlapping an input; a misaligned device pointer. */
/* A struct tag without a typedef, as frayhip_denoise. */
struct frayhip_change {
    int32_t radius;            /* the window is (2 radius + 1)^2 texels; 0..3, default 3                                     */
    float   gain;              /* change = min(1, gain * sum|difference| / sum(max)); finite and > 0, default 1             */
};
int  frayhip_change_defaults(struct frayhip_change* p);
int  frayhip_change_frame(int width, int height, const float* accum_before, const float* accum_after, const float* motion,
                          const struct frayhip_change* p, float* change, frayhip_stats* st);
int  frayhip_change_frame_device(int width, int height, const float* d_accum_before, const float* d_accum_after, const float* d_motion,
                                 const struct frayhip_change* p, float* d_change, void* hip_stream, frayhip_stats* st);
/* Gradient-adaptive accumulation: frayhip_temporal_accumulate when motion is NULL and frayhip_temporal_accumulate_motion otherwise, with a
 * change frame (W*H floats) that shortens the history per pixel.  Step 3 becomes, with g = change_p, read only where a history was fetched
 * (sum(b) > 0):
 *   !(g < 1.0f)   (1, above 1, NaN) the pixel takes no history: acc = c, m1 = l, m2 = l * l, N = 1
 *   g > 0         N0 = fminf(N_hist + 1, max_history); a0 = fmaxf(alpha_min, 1 / N0); alpha = a0 + g * (1.0f - a0);
 *                 N = fminf(N0, 1.0f / alpha); the blend of step 3 with this alpha
 *   otherwise     (+0, -0, negative) step 3 as it stands, so a change frame of zeros gives every output bit of the plain (or motion) entry
 * k_tp_variance runs unchanged on the finished hist_out: a pixel whose N dropped below variance_history takes the spatial estimate again.
 * Kernel: k_tp_accumulate<MOTION, true>; the plain and the motion entries keep their instantiations.  FRAYHIP_E_ARG: the plain entry's list,
 *   and a NULL, misaligned or overlapping (with an output) change. */
int  frayhip_temporal_accumulate_adaptive(int width, int height, const float* rgb, const float* feat, const float* motion, const float* change,
                                          const frayhip_view* prev_view, const float* hist_in, const struct frayhip_temporal* p, float* hist_out,
                                          float* signal, float* variance, frayhip_stats* st);
int  frayhip_temporal_accumulate_adaptive_device(int width, int height, const float* d_rgb, const float* d_feat, const float* d_motion,
                                                 const float* d_change, const frayhip_view* prev_view, const float* d_hist_in,
                                                 const struct frayhip_temporal* p, float* d_hist_out, float* d_signal, float* d_variance,
                                                 void* hip_stream, frayhip_stats* st);
/* The same for a split history: frayhip_temporal_accumulate_split with one change frame per component (W*H floats each; 0 direct, 1 indirect),
 * in one call on the 20-channel history.  motion may be NULL; both change frames are required.  Inputs may alias each other: one change frame
 * passed for both components is legal.
 *
 * The contract.  For every pixel the call produces two groups of outputs, each equal BIT FOR BIT to a call of
 * frayhip_temporal_accumulate_adaptive (whose motion rule is this entry's):
 *   direct    rows 0-2 of hist_out, signal_direct and variance_direct are what it returns for rgb_direct, p_direct, change_direct and rows 0-2
 *             of hist_in;
 *   indirect  {row 3}, {P, m1_I}, {n, m2_I} of hist_out, signal_indirect and variance_indirect are what it returns for rgb_indirect,
 *             p_indirect, change_indirect and the same three rows of hist_in.
 * Each component takes one of the three cases above by its own change, so the two may take different cases in one pixel; a change is read only
 * where a history was fetched (sum(b) > 0, which the components share).  Two consequences: two change frames of +0 give every output bit of
 * frayhip_temporal_accumulate_split, and two change frames of 1 give the hist_in = NULL call.
 * Kernels: k_tp_accumulate_split<MOTION, true> (the projection, the footprint, the surface tests and the tap reads once, as in the split
 *   entry; only the blend is per-component adaptive), then k_tp_variance_split unchanged and under the same condition: a pixel whose N the
 *   change dropped below its component's variance_history takes the window again.  The split entry keeps its instantiations.  No work
 *   buffers.  Device pointers, the stream contract and *st as the split entry's (the change frames 4-byte aligned).
 * FRAYHIP_E_ARG, before the device is touched: the split entry's list, and a NULL or misaligned change frame or one that an output overlaps. */
int  frayhip_temporal_accumulate_split_adaptive(int width, int height, const float* rgb_direct, const float* rgb_indirect, const float* feat,
                                                const float* motion, const float* change_direct, const float* change_indirect,
                                                const frayhip_view* prev_view, const float* hist_in, const struct frayhip_temporal* p_direct,
                                                const struct frayhip_temporal* p_indirect, float* hist_out, float* signal_direct,
                                                float* signal_indirect, float* variance_direct, float* variance_indirect, frayhip_stats* st);
int  frayhip_temporal_accumulate_split_adaptive_device(int width, int height, const float* d_rgb_direct, const float* d_rgb_indirect,
                                                       const float* d_feat, const float* d_motion, const float* d_change_direct,
                                                       const float* d_change_indirect, const frayhip_view* prev_view, const float* d_hist_in,
                                                       const struct frayhip_temporal* p_direct, const struct frayhip_temporal* p_indirect,
                                                       float* d_hist_out, float* d_signal_direct, float* d_signal_indirect,
                                                       float* d_variance_direct, float* d_variance_indirect, void* hip_stream,
                                                       frayhip_stats* st);

/* ---- weighted accumulation and history maps (samples spent where the reprojected history is short, scene-free) --------------------------------
 * A sequence may give its pixels different numbers of samples per frame (frayhip_render_samples_map renders any count plane).  Two pieces make
 * the temporal stage follow: an accumulation whose blend factor comes from sample weight instead of a frame count, and a map that says, from
 * the history reprojected into this view, how many samples each pixel gets this frame.
 *
 * Units plane: W*H floats beside the 12-channel history (whose layout is unchanged), ping-ponged by the caller as the history is: the sample
 * weight a pixel's history holds, in units of the sequence's base sample count.  N (row 0 of the history) keeps counting FRAMES: the variance
 * rules (variance_history, k_tp_variance) ask how many observations the luminance moments have seen, and a pixel that received eight units in
 * its first frame has still seen one.  Units count WEIGHT: if a pixel gets 8x the samples in its first frame and 1x in its second, a blend by
 * 1 / N would weigh the two equally and leave the pixel noisier than the first frame left it.
 *
 * frayhip_temporal_accumulate_weighted: frayhip_temporal_accumulate with a weight plane (W*H floats: the units this frame gives each pixel) and
 * the two units planes.  motion NULL or a motion frame (the arithmetic of the _motion entry), change NULL or a change frame (the arithmetic of
 * the _adaptive entry), or both.  hist_in, units_in and prev_view are all NULL (first frame) or all given.  Per pixel, with the steps of
 * "temporal accumulation":
 *   weight   w = weight_p; if (!(w >= 1.0f)) w = 1.0f; w = fminf(w, max_history).  NaN, 0 and negatives count as 1.
 *   step 2   the same taps, tests and weights b; the counted taps also sum hu += b * units_in[q], in tap order beside N's sum, and hu = hu / sum(b)
 *            where the others are divided.
 *   step 3   no history (sum(b) == 0, a miss, or a change frame with !(g < 1)):  acc = c, m1 = l, m2 = l * l, N = 1, U = w.
 *            plain (no change frame, or !(g > 0)):  N = fminf(N_hist + 1, max_history); U = fminf(hu + w, max_history);
 *              alpha = fmaxf(alpha_min, w / U); the blends of step 3 with this alpha.
 *            0 < g < 1:  N0 = fminf(N_hist + 1, max_history); U0 = fminf(hu + w, max_history); a0 = fmaxf(alpha_min, w / U0);
 *              alpha = a0 + g * (1.0f - a0); U = fminf(U0, w / alpha); N = fminf(N0, 1.0f / alpha); the blends with this alpha.
 *   outputs  row 0 .w of hist_out stores N; units_out[p] = U.
 *   step 4   unchanged, on N: a boosted pixel in its first frame has N = 1 and takes the spatial estimate.
 * The contract.  With a weight plane of 1.0f everywhere and units_in equal to hist_in's N channel bit for bit (or on the first frame), hist_out,
 * signal and variance are the matching existing entry's (plain, _motion or _adaptive) bit for bit, and units_out equals hist_out's N channel bit
 * for bit: hu is then the sum that N_hist is, so U is N, and w / U is 1.0f / N on the same operands.
 * Kernels: k_tp_accumulate<MOTION, ADAPTIVE, true>, then k_tp_variance as above; the other entries keep their instantiations.  No work buffers.
 *   Device pointers, the stream contract and *st as frayhip_temporal_accumulate_device (weight and the units planes 4-byte aligned).
 * FRAYHIP_E_ARG, before the device is touched: the adaptive entry's list (motion and change may each be NULL); a NULL, misaligned or
 *   output-overlapping weight or units_in; a NULL units_out or one that overlaps any other buffer; units_in without hist_in or the reverse.
 *
 * frayhip_history_map: per pixel,
 *   held   0 on the first frame, where step 2 fetches no history (a miss, zc <= 0, the footprint off the image, no counted tap) and where a
 *          change frame has !(g < 1); otherwise hu, exactly the hu of the weighted entry's step 2 (one device function serves both kernels);
 *          with 0 < g < 1 it is hu * (1.0f - g).  Then if (!(held >= 0)) held = 0.
 *   k      (int)floorf(fminf(held, (float)p->max_history)): the whole units the pixel already holds.
 *   units  for a target t: units(t) = min(max(t - k, 1), max_units); add = base * units, weight = (float)units.  Whole units, so that add is a
 *          multiple of base and the weight plane says exactly what was rendered.
 *   S(t) = base * the sum over all pixels of units(t), an exact 64-bit integer that does not decrease with t; target_used is the largest t in
 *   [1, target] with S(t) <= budget.  The unspent rest is not handed out: a stated limit, as in the budgeted sample map.  A budget below
 *   base * W * H makes even S(1) unaffordable: FRAYHIP_E_ARG, found from the arguments alone.
 * target 8 and max_units 8 are a maintainer's choice, not a measurement.
 * Kernels: k_hm_held (the fetch; held into a workspace of the call and into the caller's plane when given; k counted into max_history + 1 bins,
 *   per block in LDS, flushed with integer atomics), k_hm_select (one block: S(t) for every t from the bins' prefix sums; target_used, samples
 *   and boosted into a control record in device memory), k_hm_map (add and weight at the record's target).  Three launches on one stream and
 *   one synchronisation per call, whatever the data; every total is an exact integer sum, so the answer depends on neither grid nor timing.
 *   Device pointers: the history and the motion frame 16-byte aligned, the rest 4-byte; prev_view, p and m stay HOST pointers; the stream
 *   contract and *st as frayhip_temporal_accumulate_device.
 * FRAYHIP_E_ARG, before the device is touched: width or height < 1 or W*H > 2^30; a NULL feat, p, m, add or weight; hist_in, units_in and
 *   prev_view not all given or all NULL; a bad view or temporal parameter as the accumulation refuses it; base < 1; target outside
 *   1..p->max_history; max_units < 1; base * max_units > 2^24; reserved != 0; budget < base * W * H; an output overlapping an input or another
 *   output; a misaligned device pointer. */
int  frayhip_temporal_accumulate_weighted(int width, int height, const float* rgb, const float* feat, const float* motion /* NULL ok */,
                                          const float* change /* NULL ok */, const float* weight, const frayhip_view* prev_view, const float* hist_in,
                                          const float* units_in, const struct frayhip_temporal* p, float* hist_out, float* units_out, float* signal,
                                          float* variance, frayhip_stats* st);
int  frayhip_temporal_accumulate_weighted_device(int width, int height, const float* d_rgb, const float* d_feat, const float* d_motion /* NULL ok */,
                                                 const float* d_change /* NULL ok */, const float* d_weight, const frayhip_view* prev_view,
                                                 const float* d_hist_in, const float* d_units_in, const struct frayhip_temporal* p, float* d_hist_out,
                                                 float* d_units_out, float* d_signal, float* d_variance, void* hip_stream, frayhip_stats* st);
/* A struct tag without a typedef, as frayhip_denoise. */
struct frayhip_history_map {
    int32_t  base;          /* in:  samples a pixel with a full history gets; >= 1; no default (0): the caller sets it               */
    int32_t  target;        /* in:  units a pixel's history should amount to after this frame; 1..p->max_history, default 8           */
    int32_t  max_units;     /* in:  the most units one frame gives a pixel; >= 1, base * max_units <= 2^24, default 8                 */
    int32_t  reserved;      /* in:  0                                                                                                 */
    uint64_t budget;        /* in:  the most samples the plane may hold; UINT64_MAX (the default): none                               */
    uint64_t samples;       /* out: the sum of add                                                                                    */
    uint64_t boosted;       /* out: pixels with more than one unit                                                                    */
    int32_t  target_used;   /* out: the t the plane was made with                                                                     */
    int32_t  pad;
};
int  frayhip_history_map_defaults(struct frayhip_history_map* m);
int  frayhip_history_map(int width, int height, const float* feat, const float* motion /* NULL ok */, const float* change /* NULL ok */,
                         const frayhip_view* prev_view, const float* hist_in, const float* units_in, const struct frayhip_temporal* p,
                         struct frayhip_history_map* m, int32_t* add, float* weight, float* held /* NULL ok */, frayhip_stats* st);
int  frayhip_history_map_device(int width, int height, const float* d_feat, const float* d_motion /* NULL ok */, const float* d_change /* NULL ok */,
                                const frayhip_view* prev_view, const float* d_hist_in, const float* d_units_in, const struct frayhip_temporal* p,
                                struct frayhip_history_map* m, int32_t* d_add, float* d_weight, float* d_held /* NULL ok */, void* hip_stream,
                                frayhip_stats* st);

/* Not covered: SVGF's wider 3 x 3 retry when no bilinear tap counts, feeding a filtered level back into the history, moved lights and the
 * shadows and reflections of moved objects (only a pixel's own first hit is carried back: frayhip_render_features_motion), motion blur,
 * specular motion vectors for moved objects (what a static mirror or pane of glass shows under a moving camera IS followed, by the virtual-hit
 * guides of frayhip_render_features_specular; a moved object seen in a mirror, Layered glass and glossy lobes are not), learned
 * denoisers, frayhip_render_adaptive's frames (they return no variance; a state refined under a sample map does: "sample maps") and stereo frames,
 * and denoising across ranks (gather the frame and its features first: frayhip_gather_buckets takes a
 * channel count).  With a change frame the accumulation does shorten the history under a moved light and under the shadows and reflections of
 * moved objects (the history is dropped or faded there, not carried to where the shadow went).  Still not covered with it: a moved node's own pixels entering changed light (their difference is masked: they are the motion frame's
 * business), view-dependent change under camera motion, and any tuning beyond gain.  Not covered by the weighted accumulation and the history
 * map: split (20-channel) histories, handing the budget's unspent rest to other pixels, and a noise-driven map (frayhip_sample_map) inside a
 * sequence. */

/* Multi-GPU tile exchange helpers.  pack: gathers this rank's buckets from a
 * full-frame device buffer into a compact bucket-major buffer of
 * frayhip_bucket_count(W,H,first,stride) * 48*48*channels floats; unpack is the inverse and
 * is run by the gathering rank once per peer. */
int  frayhip_bucket_count(int width, int height, int bucket_first, int bucket_stride);
int  frayhip_bucket_xy(int width, int height, int bucket, int* bx, int* by);   /* bucket column and row of bucket b (the rule above) */
int  frayhip_pack_buckets_device(const float* d_frame, float* d_packed, int width, int height,
                                 int channels, int bucket_first, int bucket_stride, void* hip_stream);
int  frayhip_unpack_buckets_device(const float* d_packed, float* d_frame, int width, int height,
                                   int channels, int bucket_first, int bucket_stride, void* hip_stream);

/* The exchange itself, inside the library: rank r (of `world`) has rendered the buckets b with b % world == r into
 * its own full-size device frame (frayhip_frame.bucket_first = r, bucket_stride = world); frayhip_gather_buckets
 * moves every other rank's buckets into rank `root`'s frame -- pack, direct peer -> root RCCL transfers over xGMI
 * (grouped ncclRecv on the root, one ncclSend per peer), unpack -- enqueued on `hip_stream` of each rank.  Collective:
 * every rank of the communicator calls it.  One process per GPU; frayhip_init(device) first.
 *   frayhip_comm_unique_id   rank 0 obtains the 128-byte ncclUniqueId and hands it to the other ranks by whatever
 *                            means the host has (MPI, a file, torch.distributed, a socket)
 *   frayhip_comm_create      every rank, with the same id; world == 1 needs no id and no RCCL
 *   frayhip_comm_from_nccl   wraps an ncclComm_t the host already owns (not destroyed by frayhip_comm_destroy); FRAYHIP_E_ARG when the
 *                            communicator's own size / rank (ncclCommCount / ncclCommUserRank) are not the caller's
 *   frayhip_comm_ranks       the number of ranks RCCL itself sees in the communicator (ncclCommCount; 1 for a world of one made without
 *                            RCCL), negative error code on failure: what a host prints to show that the exchange really spans N GPUs
 *   frayhip_comm_available   1 when RCCL can be bound in this process, 0 otherwise: frayhip_comm_create blocks inside
 *                            ncclCommInitRank until EVERY rank has entered it, so the ranks agree on this first
 *   frayhip_comm_library     the file the RCCL entry points were bound from ("" when none could be): which RCCL carries the frames
 * RCCL is bound at run time (an RCCL the process already holds is used, none is loaded beside it; the environment variable
 * FRAYHIP_RCCL_LIBRARY, read at the first comm call, names a specific build to bind instead): FRAYHIP_E_UNSUPPORTED
 * when the host has none.  Gathers on one communicator share its staging buffer; a gather waits, on its own stream,
 * for the previous gather of that communicator, so they may be issued on different streams. */
#define FRAYHIP_COMM_ID_BYTES 128
typedef struct frayhip_comm frayhip_comm;
int  frayhip_comm_available(void);
const char* frayhip_comm_library(void);
int  frayhip_comm_unique_id(void* id128);
int  frayhip_comm_create(const void* id128, int rank, int world, frayhip_comm** out);
int  frayhip_comm_from_nccl(void* nccl_comm, int rank, int world, frayhip_comm** out);
int  frayhip_comm_ranks(frayhip_comm* c);
void frayhip_comm_destroy(frayhip_comm* c);
int  frayhip_gather_buckets(frayhip_comm* c, float* d_frame, int width, int height, int channels, int root, void* hip_stream);

/* vfb -> RGB32 with clamp, no gamma (displayVFB, sdl.cpp:63-74; Color::toRGB32, color.h:59-65). */
int  frayhip_to_rgb32(const float* rgb, uint32_t* out, int n_pixels);

/* Writes a float RGB frame as a 24-bit BMP the way Bitmap::saveBMP does (bitmap.cpp:197-236:
 * clamp + round per toRGB32, bottom-up rows padded to 4 bytes). */
int  frayhip_save_bmp(const char* path, const float* rgb, int width, int height);

/* Test hook: runs the device restatement of the reference's random numbers (std::mt19937 +
 * libstdc++ distributions, random_generator.cpp:41-80) for one seed and returns, for i < n,
 * the i-th randfloat() of a fresh generator, the i-th randdouble() of a second and the i-th
 * randint(0, int_hi) of a third (host buffers, any may be NULL; n <= 4096, which crosses the
 * generator's 227-word register window and two full state twists). */
int  frayhip_debug_rng(uint32_t seed, int n, float* floats, double* doubles, int32_t* ints, int int_hi);

/* Test hook: the device's sin / cos / acos behind hemisphereSample / unitDiscSample (main.cpp:92-116,
 * random_generator.cpp:71-80; the reference takes them from glibc, the device code has its own correctly rounded
 * ones, fray_amd/csrc/dev_trig.hpp) -- sincos(x[i]) and acos(fold(x[i])), so that a test can state how often they
 * equal the host's.  fold(x) = x - 2*floor(x/2) - 1 in [-1, 1) is returned in acos_arg.  Host buffers of n doubles,
 * any output may be NULL. */
int  frayhip_debug_libm(int n, const double* x, double* sin_out, double* cos_out, double* acos_out, double* acos_arg);

/* Test hook: the relaxed arithmetic of option "fp_contract" (the kernels of fray_amd/csrc/render_contract.hip, built with -ffp-contract=fast
 * -DFRAY_ARITH=1; this entry lives in the same build and calls the same inline functions) on caller-supplied operands, item i < n:
 *   op 0: out[i] = fray_rcp(a[i])          op 1: out[i] = fray_div(a[i], b[i])
 *   op 2: out[i] = fray_rsqrt(a[i])        op 3: out[i] = fray_sqrt(a[i])
 *   op 4: out[3i..3i+2] = normalized(a[3i..3i+2])
 *   op 5: out[3i..3i+2] = the direction visible(a, b) traces along: d = b - a, d * fray_rcp(length(d)) (a, b: points of 3 doubles)
 *   op 6: out[2i], out[2i+1] = the relaxed fray_sincos(a[i]): sin, cos
 *   op 7: out[2i], out[2i+1] = fray_acos_sincos(a[i]): sin(acos v), cos(acos v)
 * Host buffers; b is read by ops 1 and 5 only.  n <= 2^22.  FRAYHIP_E_ARG for a bad op, n or buffer. */
int  frayhip_debug_arith(int op, int n, const double* a, const double* b, double* out);

const char* frayhip_last_error(void);
int  frayhip_abi_version(void);
/* sizeof() of a struct of this header by name ("frayhip_mesh", ...), -1 if unknown: lets a
 * foreign-language binding check its mirror of the layouts. */
int  frayhip_sizeof(const char* struct_name);

#ifdef __cplusplus
}
#endif
#endif /* FRAYHIP_H */
