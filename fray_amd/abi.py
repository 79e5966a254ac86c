"""ctypes mirror of include/frayhip.h (the C ABI of libfrayhip.so).

Field order and types follow the header one for one; tests/test_abi.py checks the struct sizes
against the library's own sizeof table so that the two cannot drift apart silently.
"""
import ctypes as C

i32, u32, i64, u64, f32, f64 = C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double
P = C.POINTER

ABI_VERSION = 3

OK, E_ARG, E_PARSE, E_NODEVICE, E_UNSUPPORTED, E_NOMEM, E_HIP, E_CANCELLED = 0, -1, -2, -3, -4, -5, -6, -7
GEOM_PLANE, GEOM_SPHERE, GEOM_CUBE, GEOM_MESH, GEOM_CSG = range(5)
TEX_CHECKER, TEX_BITMAP, TEX_BUMP, TEX_FRESNEL = range(4)
SHADER_CONST, SHADER_LAMBERT, SHADER_PHONG, SHADER_REFL, SHADER_REFR, SHADER_LAYERED = range(6)
LIGHT_POINT, LIGHT_RECT = range(2)
MODE_PRIMARY_ID, MODE_RENDER = 0, 1
FRAME_STATS = 1
# the names frayhip_scene_set_option accepts, and what frayhip_scene_get_option reports besides them (tests/test_call_history.py holds both to capi.hip)
OPTION_NAMES = ("pt_lanes", "pt_budget_mib", "speculate_fans", "fused_whitted_max", "fp_contract", "seed_table_mib", "skip_null_segments",
                "segment_planes", "certified_segments")
FIGURE_NAMES = ("contracted_launches", "shadow_segments", "segment_plane_nodes", "certified_segments_eligible", "shadow_segments_certified",
                "shadow_nodes_skipped", "seed_table_bytes", "seed_launches", "seed_planes_reused", "batch_lanes", "whitted_path",
                "pt_budget_effective_mib", "scene_updates", "scene_update_bytes", "arena_bytes", "fans_filed", "fan_children",
                "fan_children_looked_up", "fans_given_up")


class Transform(C.Structure):
    _fields_ = [("offset", f64 * 3), ("m", f64 * 9), ("invM", f64 * 9)]


class GeomRef(C.Structure):
    _fields_ = [("kind", i32), ("index", i32)]


class Node(C.Structure):
    _fields_ = [("geom", i32), ("shader", i32), ("bump_tex", i32), ("_pad", i32), ("T", Transform)]


class Plane(C.Structure):
    _fields_ = [("limit", f64), ("height", f64)]


class Sphere(C.Structure):
    _fields_ = [("O", f64 * 3), ("R", f64)]


class Cube(C.Structure):
    _fields_ = [("O", f64 * 3), ("halfSide", f64)]


class Csg(C.Structure):
    _fields_ = [("op", i32), ("left", i32), ("right", i32), ("_pad", i32)]


class Triangle(C.Structure):
    _fields_ = [("v", i32 * 3), ("n", i32 * 3), ("t", i32 * 3), ("_pad", i32),
                ("gnormal", f64 * 3), ("dNdx", f64 * 3), ("dNdy", f64 * 3),
                ("AB", f64 * 3), ("AC", f64 * 3), ("ABcrossAC", f64 * 3)]


class KDNode(C.Structure):
    _fields_ = [("axis", i32), ("child0", i32), ("parent", i32), ("tri_begin", i32),
                ("tri_count", i32), ("_pad", i32), ("split", f64)]


class Mesh(C.Structure):
    _fields_ = [("n_vertices", i32), ("n_normals", i32), ("n_uvs", i32), ("n_triangles", i32),
                ("n_kdnodes", i32), ("n_trirefs", i32),
                ("faceted", i32), ("backfaceCulling", i32), ("has_kd", i32), ("_pad", i32),
                ("bbox_min", f64 * 3), ("bbox_max", f64 * 3),
                ("vertices", P(f64)), ("normals", P(f64)), ("uvs", P(f64)),
                ("triangles", P(Triangle)), ("kdnodes", P(KDNode)), ("trirefs", P(i32)),
                ("kd_max_depth", i32), ("kd_depth_sum", i32)]


class Texture(C.Structure):
    _fields_ = [("kind", i32), ("width", i32), ("height", i32), ("_pad", i32),
                ("color1", f32 * 3), ("color2", f32 * 3),
                ("scaling", f64), ("bumpIntensity", f64), ("ior", f64), ("texel_offset", i64)]


class Shader(C.Structure):
    _fields_ = [("kind", i32), ("texture", i32), ("color", f32 * 3), ("specularColor", f32 * 3),
                ("mult", f32 * 3), ("numSamples", i32),
                ("exponent", f64), ("specularMultiplier", f64), ("glossiness", f64),
                ("deflectionScaling", f64), ("ior", f64), ("layer_begin", i32), ("layer_count", i32)]


class Layer(C.Structure):
    _fields_ = [("shader", i32), ("texture", i32), ("opacity", f32 * 3), ("_pad", i32)]


class Light(C.Structure):
    _fields_ = [("kind", i32), ("xSubd", i32), ("ySubd", i32), ("_pad", i32),
                ("color", f32 * 3), ("power", f32), ("pos", f64 * 3), ("T", Transform),
                ("center", f64 * 3), ("area", f64)]


class Camera(C.Structure):
    _fields_ = [("pos", f64 * 3), ("yaw", f64), ("pitch", f64), ("roll", f64), ("fov", f64),
                ("aspectRatio", f64), ("focalPlaneDist", f64), ("fNumber", f64),
                ("stereoSeparation", f64),
                ("dof", i32), ("autofocus", i32), ("numDOFSamples", i32), ("_pad", i32),
                ("leftMask", f32 * 3), ("rightMask", f32 * 3)]


class Settings(C.Structure):
    _fields_ = [("frameWidth", i32), ("frameHeight", i32), ("ambientLight", f32 * 3),
                ("wantAA", i32), ("gi", i32), ("maxTraceDepth", i32), ("dbg", i32),
                ("saturation", f32), ("wantPrepass", i32), ("numPaths", i32), ("numThreads", i32),
                ("interactive", i32), ("fullscreen", i32)]


class Environment(C.Structure):
    _fields_ = [("present", i32), ("loaded", i32), ("width", i32 * 6), ("height", i32 * 6),
                ("texel_offset", i64 * 6)]


class SceneDesc(C.Structure):
    _fields_ = [("abi_version", i32),
                ("n_nodes", i32), ("n_geoms", i32), ("n_planes", i32), ("n_spheres", i32),
                ("n_cubes", i32), ("n_csgs", i32), ("n_meshes", i32),
                ("n_shaders", i32), ("n_layers", i32), ("n_textures", i32), ("n_lights", i32),
                ("n_texels", i64),
                ("nodes", P(Node)), ("geoms", P(GeomRef)), ("planes", P(Plane)),
                ("spheres", P(Sphere)), ("cubes", P(Cube)), ("csgs", P(Csg)), ("meshes", P(Mesh)),
                ("shaders", P(Shader)), ("layers", P(Layer)), ("textures", P(Texture)),
                ("lights", P(Light)), ("texels", P(f32)),
                ("environment", Environment), ("camera", Camera), ("settings", Settings)]


class Frame(C.Structure):
    _fields_ = [("mode", i32), ("seed", u32), ("bucket_first", i32), ("bucket_stride", i32),
                ("spp_chunk", i32), ("flags", i32)]


class Stats(C.Structure):
    _fields_ = [("closest_rays", u64), ("shadow_rays", u64), ("node_tests", u64),
                ("kd_inner_visits", u64), ("leaf_refs", u64), ("tri_tests", u64),
                ("prim_tests", u64), ("smooth_hits", u64), ("samples", u64),
                ("texture_fetches", u64),
                ("ms_total", f64), ("ms_kernels", f64), ("ms_trace", f64),
                ("trace_launches", u64), ("alg_bytes_trace", f64),
                ("ms_shadow", f64), ("shadow_launches", u64), ("alg_bytes_shadow", f64),
                ("alg_flops_trace", f64), ("alg_flops_shadow", f64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Progress(C.Structure):
    _fields_ = [("samples_done", i32), ("samples_total", i32), ("batches_done", i32), ("batches_total", i32),
                ("ms_elapsed", f64), ("preview", i32), ("final", i32), ("rgb", P(f32))]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "rgb"}


# int (*fn)(void* user, const frayhip_progress*)
PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, P(Progress))


class Progressive(C.Structure):
    _fields_ = [("fn", PROGRESS_FN), ("user", C.c_void_p), ("preview_ms", f64)]


class ShadeRequest(C.Structure):
    _fields_ = [("seed", u32), ("spp", i32), ("sample_first", i32), ("rng_skip", i32), ("flags", i32), ("_pad", i32),
                ("keys", C.c_void_p)]


class Adaptive(C.Structure):
    _fields_ = [("min_spp", i32), ("_pad", i32), ("threshold", f64), ("err_floor", f64), ("rungs", i32), ("_pad2", i32),
                ("samples", u64)]


ACCUM_CHANNELS = 4      # FRAYHIP_ACCUM_CHANNELS: sum.r, sum.g, sum.b, m2


class Samples(C.Structure):
    _fields_ = [("sample_first", i32), ("sample_count", i32), ("samples_done", i32), ("_pad", i32)]


class SamplesMap(C.Structure):
    _fields_ = [("samples", u64), ("count_min", i32), ("count_max", i32)]


# struct frayhip_sample_map (a struct tag without a typedef, as frayhip_denoise: the name is also the entry point's)
class SampleMap(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("lum_floor", C.c_float), ("min_count", i32), ("max_count", i32), ("max_add", i32), ("grow", i32),
                ("pixels", u64), ("samples", u64)]


# struct frayhip_sample_budget (frayhip_sample_map_budget's second struct; a tag without a typedef as well)
class SampleBudget(C.Structure):
    _fields_ = [("budget", u64), ("demand", u64), ("tolerance_used", C.c_float), ("cap_used", i32), ("stage", i32), ("reserved", i32)]


# struct frayhip_denoise (a struct tag without a typedef: the name is also the entry point's, so it is not in STRUCTS, which mirrors the typedefs)
class Denoise(C.Structure):
    _fields_ = [("levels", i32), ("demodulate", i32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float)]


FEAT_CHANNELS = 10      # FRAYHIP_FEAT_CHANNELS: position[3], normal[3], albedo[3], depth
MOTION_CHANNELS = 8     # FRAYHIP_MOTION_CHANNELS: {P'.xyz, moved}, {n'.xyz, 0}
SPECULAR_MAX_BOUNCES = 8   # FRAYHIP_SPECULAR_MAX_BOUNCES: frayhip_render_features_specular's max_bounces is 1 .. 8


class View(C.Structure):
    _fields_ = [("pos", f32 * 3), ("right", f32 * 3), ("up", f32 * 3), ("front", f32 * 3), ("tan_x", C.c_float), ("tan_y", C.c_float),
                ("width", i32), ("height", i32)]


# struct frayhip_temporal (a struct tag without a typedef, as frayhip_denoise)
class Temporal(C.Structure):
    _fields_ = [("demodulate", i32), ("max_history", i32), ("variance_history", i32), ("alpha_min", C.c_float), ("film_offset", C.c_float),
                ("plane_tolerance", C.c_float), ("normal_min_dot", C.c_float)]


# struct frayhip_change (a struct tag without a typedef, as frayhip_denoise)
class Change(C.Structure):
    _fields_ = [("radius", i32), ("gain", C.c_float)]


# struct frayhip_history_map (a struct tag without a typedef, as frayhip_denoise: the name is also the entry point's)
class HistoryMap(C.Structure):
    _fields_ = [("base", i32), ("target", i32), ("max_units", i32), ("reserved", i32), ("budget", u64), ("samples", u64), ("boosted", u64),
                ("target_used", i32), ("pad", i32)]


NO_BUDGET = (1 << 64) - 1   # frayhip_history_map.budget: none (UINT64_MAX)
HISTORY_CHANNELS = 12   # FRAYHIP_HISTORY_CHANNELS: {acc.rgb, N}, {P.xyz, m1}, {n.xyz, m2}
HISTORY_SPLIT_CHANNELS = 20   # FRAYHIP_HISTORY_SPLIT_CHANNELS: {accD.rgb, N_D}, {P.xyz, m1_D}, {n.xyz, m2_D}, {accI.rgb, N_I}, {m1_I, m2_I, 0, 0}


STRUCTS = {"frayhip_transform": Transform, "frayhip_geom_ref": GeomRef, "frayhip_node": Node,
           "frayhip_plane": Plane, "frayhip_sphere": Sphere, "frayhip_cube": Cube,
           "frayhip_csg": Csg, "frayhip_triangle": Triangle, "frayhip_kdnode": KDNode,
           "frayhip_mesh": Mesh, "frayhip_texture": Texture, "frayhip_shader": Shader,
           "frayhip_layer": Layer, "frayhip_light": Light, "frayhip_camera": Camera,
           "frayhip_settings": Settings, "frayhip_environment": Environment,
           "frayhip_scene_desc": SceneDesc, "frayhip_frame": Frame, "frayhip_stats": Stats,
           "frayhip_progress": Progress, "frayhip_progressive": Progressive,
           "frayhip_shade_request": ShadeRequest, "frayhip_adaptive": Adaptive, "frayhip_samples": Samples,
           "frayhip_view": View, "frayhip_samples_map": SamplesMap}

# Every symbol include/frayhip.h declares: name -> (restype, argtypes)
VP = C.c_void_p
SYMBOLS = {
    "frayhip_scene_parse": (C.c_int, [C.c_char_p, P(VP)]),
    "frayhip_host_scene_desc": (P(SceneDesc), [VP]),
    "frayhip_host_scene_free": (None, [VP]),
    "frayhip_init": (C.c_int, [C.c_int]),
    "frayhip_scene_create": (C.c_int, [P(SceneDesc), P(VP)]),
    "frayhip_scene_destroy": (None, [VP]),
    "frayhip_scene_set_view": (C.c_int, [VP, P(Camera), P(Settings)]),
    "frayhip_scene_update": (C.c_int, [VP, P(SceneDesc)]),
    "frayhip_transform_identity": (C.c_int, [P(Transform)]),
    "frayhip_transform_scale": (C.c_int, [P(Transform), f64, f64, f64]),
    "frayhip_transform_rotate": (C.c_int, [P(Transform), f64, f64, f64]),
    "frayhip_transform_translate": (C.c_int, [P(Transform), f64, f64, f64]),
    "frayhip_light_begin_frame": (C.c_int, [P(Light)]),
    "frayhip_shader_begin_frame": (C.c_int, [P(Shader)]),
    "frayhip_scene_set_option": (C.c_int, [VP, C.c_char_p, i64]),
    "frayhip_scene_get_option": (C.c_int, [VP, C.c_char_p, P(i64)]),
    "frayhip_scene_tight_gates": (C.c_int, [VP, C.c_int, P(i64), P(i64)]),
    "frayhip_scene_camera_skip": (C.c_int, [VP, C.c_int, P(i64), P(i64), P(i64), P(i64)]),
    "frayhip_scene_camera_tiles": (C.c_int, [VP, C.c_int, P(i64)]),
    "frayhip_scene_shade_shortcuts": (C.c_int, [VP, C.c_int, P(i64), P(i64)]),
    "frayhip_render": (C.c_int, [VP, P(Frame), VP, VP, VP, P(Stats)]),
    "frayhip_render_device": (C.c_int, [VP, P(Frame), VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_progressive": (C.c_int, [VP, P(Frame), P(Progressive), VP, VP, VP, P(Stats)]),
    "frayhip_render_device_progressive": (C.c_int, [VP, P(Frame), P(Progressive), VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_adaptive": (C.c_int, [VP, P(Frame), P(Adaptive), VP, VP, VP, P(Stats)]),
    "frayhip_render_device_adaptive": (C.c_int, [VP, P(Frame), P(Adaptive), VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_samples": (C.c_int, [VP, P(Frame), P(Samples), P(Progressive), VP, VP, VP, P(Stats)]),
    "frayhip_render_samples_device": (C.c_int, [VP, P(Frame), P(Samples), P(Progressive), VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_components": (C.c_int, [VP, P(Frame), P(Samples), P(Progressive), VP, VP, VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_components_device": (C.c_int, [VP, P(Frame), P(Samples), P(Progressive), VP, VP, VP, VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_samples_map": (C.c_int, [VP, P(Frame), P(SamplesMap), VP, VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_samples_map_device": (C.c_int, [VP, P(Frame), P(SamplesMap), VP, VP, VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_components_map": (C.c_int, [VP, P(Frame), P(SamplesMap), VP, VP, VP, VP, VP, VP, VP, VP, P(Stats)]),
    "frayhip_render_components_map_device": (C.c_int, [VP, P(Frame), P(SamplesMap), VP, VP, VP, VP, VP, VP, VP, VP, VP, P(Stats)]),
    "frayhip_sample_map_defaults": (C.c_int, [P(SampleMap)]),
    "frayhip_sample_map": (C.c_int, [C.c_int, C.c_int, VP, VP, P(SampleMap), VP, P(Stats)]),
    "frayhip_sample_map_device": (C.c_int, [C.c_int, C.c_int, VP, VP, P(SampleMap), VP, VP, P(Stats)]),
    "frayhip_sample_map_pair": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(SampleMap), VP, P(Stats)]),
    "frayhip_sample_map_pair_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(SampleMap), VP, VP, P(Stats)]),
    "frayhip_sample_map_budget": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(SampleMap), P(SampleBudget), VP, P(Stats)]),
    "frayhip_sample_map_budget_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(SampleMap), P(SampleBudget), VP, VP, P(Stats)]),
    "frayhip_render_features": (C.c_int, [VP, P(Frame), C.c_int, VP, P(Stats)]),
    "frayhip_render_features_device": (C.c_int, [VP, P(Frame), C.c_int, VP, VP, P(Stats)]),
    "frayhip_render_features_specular": (C.c_int, [VP, P(Frame), C.c_int, C.c_int, VP, VP, P(Stats)]),
    "frayhip_render_features_specular_device": (C.c_int, [VP, P(Frame), C.c_int, C.c_int, VP, VP, VP, P(Stats)]),
    "frayhip_render_features_motion": (C.c_int, [VP, P(Frame), C.c_int, P(Transform), C.c_int, VP, VP, P(Stats)]),
    "frayhip_render_features_motion_device": (C.c_int, [VP, P(Frame), C.c_int, P(Transform), C.c_int, VP, VP, VP, P(Stats)]),
    "frayhip_denoise_defaults": (C.c_int, [P(Denoise)]),
    "frayhip_denoise": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(Denoise), VP, P(Stats)]),
    "frayhip_denoise_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(Denoise), VP, VP, P(Stats)]),
    "frayhip_denoise_signal": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(Denoise), VP, P(Stats)]),
    "frayhip_denoise_signal_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(Denoise), VP, VP, P(Stats)]),
    "frayhip_view_from_camera": (C.c_int, [P(Camera), C.c_int, C.c_int, P(View)]),
    "frayhip_temporal_defaults": (C.c_int, [P(Temporal)]),
    "frayhip_temporal_accumulate": (C.c_int, [C.c_int, C.c_int, VP, VP, P(View), VP, P(Temporal), VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_device": (C.c_int, [C.c_int, C.c_int, VP, VP, P(View), VP, P(Temporal), VP, VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_motion": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(View), VP, P(Temporal), VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_motion_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(View), VP, P(Temporal), VP, VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_split": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, VP, P(View), VP, P(Temporal), P(Temporal), VP, VP, VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_split_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, VP, P(View), VP, P(Temporal), P(Temporal), VP, VP, VP, VP, VP, VP,
                                                           P(Stats)]),
    "frayhip_change_defaults": (C.c_int, [P(Change)]),
    "frayhip_change_frame": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(Change), VP, P(Stats)]),
    "frayhip_change_frame_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(Change), VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_adaptive": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, VP, P(View), VP, P(Temporal), VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_adaptive_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, VP, P(View), VP, P(Temporal), VP, VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_split_adaptive": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, VP, VP, VP, P(View), VP, P(Temporal), P(Temporal), VP, VP, VP, VP,
                                                             VP, P(Stats)]),
    "frayhip_temporal_accumulate_split_adaptive_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, VP, VP, VP, P(View), VP, P(Temporal), P(Temporal), VP, VP,
                                                                    VP, VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_weighted": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, VP, VP, P(View), VP, VP, P(Temporal), VP, VP, VP, VP, P(Stats)]),
    "frayhip_temporal_accumulate_weighted_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, VP, VP, P(View), VP, VP, P(Temporal), VP, VP, VP, VP, VP,
                                                              P(Stats)]),
    "frayhip_history_map_defaults": (C.c_int, [P(HistoryMap)]),
    "frayhip_history_map": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(View), VP, VP, P(Temporal), P(HistoryMap), VP, VP, VP, P(Stats)]),
    "frayhip_history_map_device": (C.c_int, [C.c_int, C.c_int, VP, VP, VP, P(View), VP, VP, P(Temporal), P(HistoryMap), VP, VP, VP, VP, P(Stats)]),
    "frayhip_camera_rays": (C.c_int, [VP, i64, VP, C.c_int, VP, VP]),
    "frayhip_camera_rays_device": (C.c_int, [VP, i64, VP, C.c_int, VP, VP, VP]),
    "frayhip_trace_rays": (C.c_int, [VP, i64, VP, VP, C.c_int, VP, VP, VP, P(Stats)]),
    "frayhip_trace_rays_device": (C.c_int, [VP, i64, VP, VP, C.c_int, VP, VP, VP, VP, P(Stats)]),
    "frayhip_visible": (C.c_int, [VP, i64, VP, VP, C.c_int, VP, P(Stats)]),
    "frayhip_visible_device": (C.c_int, [VP, i64, VP, VP, C.c_int, VP, VP, P(Stats)]),
    "frayhip_shade_rays": (C.c_int, [VP, i64, VP, VP, P(ShadeRequest), VP, P(Stats)]),
    "frayhip_shade_rays_device": (C.c_int, [VP, i64, VP, VP, P(ShadeRequest), VP, VP, P(Stats)]),
    "frayhip_bucket_count": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "frayhip_pack_buckets_device": (C.c_int, [VP, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "frayhip_unpack_buckets_device": (C.c_int, [VP, VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "frayhip_bucket_xy": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "frayhip_comm_available": (C.c_int, []),
    "frayhip_comm_library": (C.c_char_p, []),
    "frayhip_comm_unique_id": (C.c_int, [VP]),
    "frayhip_comm_create": (C.c_int, [VP, C.c_int, C.c_int, P(VP)]),
    "frayhip_comm_from_nccl": (C.c_int, [VP, C.c_int, C.c_int, P(VP)]),
    "frayhip_comm_ranks": (C.c_int, [VP]),
    "frayhip_comm_destroy": (None, [VP]),
    "frayhip_gather_buckets": (C.c_int, [VP, VP, C.c_int, C.c_int, C.c_int, C.c_int, VP]),
    "frayhip_to_rgb32": (C.c_int, [VP, VP, C.c_int]),
    "frayhip_save_bmp": (C.c_int, [C.c_char_p, VP, C.c_int, C.c_int]),
    "frayhip_debug_rng": (C.c_int, [u32, C.c_int, VP, VP, VP, C.c_int]),
    "frayhip_debug_libm": (C.c_int, [C.c_int, VP, VP, VP, VP, VP]),
    "frayhip_debug_arith": (C.c_int, [C.c_int, C.c_int, VP, VP, VP]),
    "frayhip_last_error": (C.c_char_p, []),
    "frayhip_abi_version": (C.c_int, []),
    "frayhip_sizeof": (C.c_int, [C.c_char_p]),
}


def bind(lib):
    """Attach restype/argtypes for every declared symbol; raises AttributeError if one is missing."""
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
