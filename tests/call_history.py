"""Operations on a scene handle and the orders to run them in (DESIGN.md "What the call histories show").  Not a test module.

An OPERATION is a complete configuration plus one call: before its call it writes the frame size, every settings and camera field, every settable
option, the tight-gates switch (frayhip_scene_tight_gates, which is no option name) and -- through Scene.update, when they differ from what the handle
holds -- the editable tables.  So the only thing one operation hands to the
next is what the library keeps behind the handle (render_state.hpp: the workspace, the statistics block and its tile cursors, the queue tables, the seed
table, the warm mask, the effective budget, the motion table, the event pools, the lane streams), and that is what the sequences below vary.  An
operation's answer is a dict of arrays and integers; answers are compared byte for byte.

Nothing here imports torch or opens the GPU: a Handle is given the fray_amd module, the generators and the comparer are plain Python, and
tests/test_call_history.py runs them over a fake handle.  tests/test_gpu_call_history.py runs them on the device."""
import ctypes as C
import random

import numpy as np

import scene_edits
from test_gpu_trace_host import SCENES_BY_WORD

SCENES = [n for n, _ in SCENES_BY_WORD]

# every name frayhip_scene_set_option accepts, with the value a handle is created with (render_state.hpp); tests/test_call_history.py holds this list
# to the library's, so that a new option fails there until the operations set it
OPTION_DEFAULTS = dict(pt_lanes=4, pt_budget_mib=24576, speculate_fans=1, fused_whitted_max=4, fp_contract=0, seed_table_mib=4096,
                       skip_null_segments=1, segment_planes=1, certified_segments=1)
TIGHT_GATES_DEFAULT = 1         # frayhip_scene_tight_gates: the switch a handle is created with (render_state.hpp tightGates), written like an option
# the settings and camera fields an operation may set; every other field is written from the scene file's record before every call
SETTINGS_SET = ("frameWidth", "frameHeight", "wantAA", "gi", "maxTraceDepth", "numPaths")
CAMERA_SET = ("dof", "stereoSeparation")
SETTINGS_DEFAULTS = dict(frameWidth=64, frameHeight=48, wantAA=0, gi=1, maxTraceDepth=None, numPaths=6)      # None: the scene file's
CAMERA_DEFAULTS = dict(dof=0, stereoSeparation=0.0)
EDITABLE = ("nodes", "lights", "shaders", "layers", "textures", "spheres", "planes", "cubes")

COUNTERS = ("closest_rays", "shadow_rays", "node_tests", "kd_inner_visits", "leaf_refs", "tri_tests", "prim_tests", "smooth_hits", "samples",
            "texture_fetches")
# what frayhip_scene_get_option reports besides the options themselves
FIGURES = ("contracted_launches", "shadow_segments", "segment_plane_nodes", "certified_segments_eligible", "shadow_segments_certified",
           "shadow_nodes_skipped", "seed_table_bytes", "seed_launches", "seed_planes_reused", "batch_lanes", "whitted_path", "pt_budget_effective_mib",
           "scene_updates", "scene_update_bytes", "arena_bytes", "fans_filed", "fan_children", "fan_children_looked_up", "fans_given_up")

# The figures "of the last frame" have one writer each, and a call that does not reach it leaves the frame before's in place:
#   render_impl.hpp writes batch_lanes at its head and the segment, fan and contracted figures once the frame is traced (any mode, cancelled frames too);
#   whitted_path only in its Whitted branch; adaptive_impl (adaptive_variant.hip) zeroes the contracted and fan figures and touches no other;
#   the query, feature and refused calls write none.
FAN_FIGURES = ("fans_filed", "fan_children", "fan_children_looked_up", "fans_given_up")
FRAME_FIGURES = ("contracted_launches", "shadow_segments", "shadow_segments_certified", "shadow_nodes_skipped", "batch_lanes") + FAN_FIGURES
OWNED = {"frame": FRAME_FIGURES, "whitted": FRAME_FIGURES + ("whitted_path",), "adaptive": ("contracted_launches",) + FAN_FIGURES, "none": ()}
LAST_FRAME_FIGURES = OWNED["whitted"]

# per scene: the node the edits and the motion frame move, a stereo separation at the scene's scale, and the two edits (tokens of tests/scene_edits.py)
_BOXED = scene_edits.CASES["boxed-textured"]["edit"]
_CSG = scene_edits.CASES["csg-nested"]["edit"]
SCENE_FACTS = {
    "cornell_box": dict(node=6, stereo=12.0, edit_node=scene_edits.CASES["cornell-block"]["edit"], edit_other=scene_edits.CASES["cornell-light"]["edit"]),
    # boxed-textured, cut where its node move begins: the checker's colours and the dice's bump first, the teapot's transform second
    "boxed": dict(node=7, stereo=0.25, edit_node=_BOXED[_BOXED.index("node", _BOXED.index("bump")):], edit_other=_BOXED[:_BOXED.index("node", _BOXED.index("bump"))]),
    # csg-nested, cut likewise: node `a` moves; a sphere's radius and a cube's half side (the scene has one light and no shader the case edits)
    "csg_nested": dict(node=1, stereo=0.25, edit_node=_CSG[:_CSG.index("sphere")], edit_other=_CSG[_CSG.index("sphere"):]),
    # no case of scene_edits.py is of this scene: the plates move, the light takes 3 x 3 samples
    "textured_plain": dict(node=2, stereo=0.25, edit_node="node 2 reset node 2 translate 4 2.5 1 node 2 scale 2 2 2".split(), edit_other="light 0 subd 3 3".split()),
}


class Op:
    """name; settings / camera / options: what differs from the defaults above; tight_gates: the switch of frayhip_scene_tight_gates, 1 or 0;
    tables: "original", "edit_node" or "edit_other"; call(handle) -> answer;
    kind: which of the last frame's figures the call writes (OWNED);
    work: the workspace the call left on a fresh handle, in bytes (filled in by whoever measured it; big_then_small reads it)."""

    def __init__(self, name, call, settings=None, camera=None, options=None, tables="original", kind="frame", tight_gates=TIGHT_GATES_DEFAULT):
        self.name, self.call, self.tables, self.work, self.kind, self.tight_gates = name, call, tables, None, kind, tight_gates
        assert kind in OWNED and tight_gates in (0, 1), (kind, tight_gates)
        self.settings, self.camera, self.options = dict(settings or {}), dict(camera or {}), dict(options or {})
        assert set(self.settings) <= set(SETTINGS_SET) and set(self.camera) <= set(CAMERA_SET) and set(self.options) <= set(OPTION_DEFAULTS), name

    def config(self):
        """the complete configuration: every option, the tight-gates switch, every settable settings and camera field, and the tables"""
        return dict(settings=dict(SETTINGS_DEFAULTS, **self.settings), camera=dict(CAMERA_DEFAULTS, **self.camera),
                    options=dict(OPTION_DEFAULTS, **self.options), tight_gates=self.tight_gates, tables=self.tables)

    def __repr__(self):
        return "Op(%s)" % self.name


# ---- a handle -----------------------------------------------------------------------------------------------------------------------------------
class Handle:
    """One fray_amd.Scene and its device handle.  run(op) writes op's complete configuration, makes its call and returns its answer with the figures of
    frayhip_scene_get_option under "fig:<name>".  renew() destroys the device handle and creates a new one from the original description."""

    def __init__(self, fray, name, path):
        self.fray, self.abi, self.name = fray, fray.abi, name
        self.s = fray.Scene.parseScene(path)
        self.facts = SCENE_FACTS[name]
        self.settings0, self.camera0 = bytes(self.s.desc.settings), bytes(self.s.desc.camera)
        self.tables0 = {t: bytes(getattr(self.s, t)) for t in EDITABLE}
        self.tables, self.edited = None, False
        self.renew()

    def _write_tables(self, which):
        for t in EDITABLE:
            if self.tables0[t]:
                C.memmove(getattr(self.s, t), self.tables0[t], len(self.tables0[t]))
        if which != "original":
            scene_edits.apply(self.fray, self.s, self.facts[which])

    def renew(self):
        self._write_tables("original")
        self.s.beginRender()
        self.tables, self.edited = "original", False
        return self

    def close(self):
        self.s.close()

    def configure(self, op):
        s, cfg = self.s, op.config()
        C.memmove(C.byref(s.desc.settings), self.settings0, len(self.settings0))
        C.memmove(C.byref(s.desc.camera), self.camera0, len(self.camera0))
        for k, v in cfg["settings"].items():
            if v is not None:
                setattr(s.settings, k, v)
        for k, v in cfg["camera"].items():
            setattr(s.camera, k, self.facts["stereo"] if (k == "stereoSeparation" and v is True) else v)
        s.beginFrame()
        for k, v in cfg["options"].items():
            s.set_option(k, v)
        s.tight_gates(cfg["tight_gates"])
        if cfg["tables"] != self.tables:
            self._write_tables(cfg["tables"])
            s.update()
            self.tables, self.edited = cfg["tables"], True

    def run(self, op):
        self.configure(op)
        ans = op.call(self)
        for k in FIGURES:
            ans["fig:" + k] = self.s.get_option(k)
        return ans


def _stats(ans, st):
    for k in COUNTERS:
        ans["stat:" + k] = int(st[k])
    return ans


def expected_whitted_path(h, fused_max):
    """render_impl's choice, restated from the description: 0 with a recursive shader on a node (Refl, Refr, Layered), else 2 (fused) where the lights
    take at most fused_whitted_max samples per hit and the scene's kernels are not the KD or Cube / CSG variants, else 1"""
    d, abi = h.s.desc, h.abi
    if any(d.shaders[d.nodes[i].shader].kind in (abi.SHADER_REFL, abi.SHADER_REFR, abi.SHADER_LAYERED) for i in range(d.n_nodes)):
        return 0
    T = sum(L.xSubd * L.ySubd if L.kind == abi.LIGHT_RECT else 1 for L in h.s.lights)
    kd = any(d.meshes[i].has_kd for i in range(d.n_meshes)) or any(d.geoms[d.nodes[i].geom].kind in (abi.GEOM_CUBE, abi.GEOM_CSG) for i in range(d.n_nodes))
    return 2 if (T <= fused_max and not kd) else 1


# ---- the calls ----------------------------------------------------------------------------------------------------------------------------------
def frame(**kw):
    stats = kw.get("stats", False)
    kw.setdefault("seed", 42)

    def call(h):
        rgb, st = h.s.render(**kw)
        ans = {"rgb": rgb}
        return _stats(ans, st) if stats else ans
    return call


def whitted_frame(h):
    rgb, _ = h.s.render(seed=42)
    path = h.s.get_option("whitted_path")
    want = expected_whitted_path(h, h.s.get_option("fused_whitted_max"))
    assert path == want, ("whitted_path", path, "expected", want)
    return {"rgb": rgb}


def budget_frame(h):
    """the smallest budget the option accepts: more batches than lanes, read from the frame's own progress reports"""
    seen = {}

    def progress(info):
        seen.update(batches=info["batches_total"])
        return False
    rgb, st = h.s.render(seed=42, progress=progress)
    lanes = h.s.get_option("batch_lanes")
    assert not st["cancelled"] and seen["batches"] > lanes, ("batches", seen.get("batches"), "lanes", lanes)
    return {"rgb": rgb, "batches": seen["batches"]}


def primary(h):
    ids, dist, _ = h.s.primary_hits()
    return {"ids": ids, "dist": dist}


def progressive(h):
    shots = []

    def progress(info):
        if info["preview"]:
            shots.append(info["image"].copy())
        return False
    rgb, st = h.s.render(seed=42, spp_chunk=2, progress=progress, preview_ms=0)
    assert not st["cancelled"] and len(shots) == 3, len(shots)              # 6 samples in batches of 2
    ans = {"rgb": rgb}
    ans.update(("preview%d" % i, p) for i, p in enumerate(shots))
    return ans


def progressive_cancelled(h):
    rgb, st = h.s.render(seed=42, spp_chunk=2, progress=lambda info: True)
    assert st["cancelled"] and 0 < st["samples_done"] < 12, st
    return {"rgb": rgb, "samples_done": st["samples_done"]}


def samples_3_5(h):
    _, state = h.s.render_samples(3, spp_chunk=2, seed=42)
    rgb, state, noise = h.s.render_samples(5, state, spp_chunk=2, seed=42, noise=True)
    assert state.samples_done == 8
    return {"rgb": rgb, "state": state.state, "noise": noise}


def samples_resumed(h):
    first, state, st = h.s.render_samples(12, spp_chunk=2, seed=42, progress=lambda info: True)
    k = state.samples_done
    assert st["cancelled"] and 0 < k < 12, (st, k)
    rgb, state = h.s.render_samples(12 - k, state, spp_chunk=2, seed=42)
    assert state.samples_done == 12
    return {"cancelled_rgb": first, "rgb": rgb, "state": state.state, "cancelled_at": k}


def adaptive(h):
    rgb, spp, err, info = h.s.render_adaptive(0.05, min_spp=2, seed=42)
    return {"rgb": rgb, "spp": spp, "err": err, "rungs": info["rungs"], "samples": info["samples"]}


def features(h):
    return {"feat": h.s.render_features(4, seed=42)}


def features_motion(h):
    prev = h.s.node_transforms()
    i = h.facts["node"]
    h.fray.Transform(prev[i]).translate(0.5, 0.25, -0.5).store(prev[i])
    feat, motion = h.s.render_features_motion(prev, 4, seed=42)
    return {"feat": feat, "motion": motion}


def _rows(h, step=3):
    """a few hundred of the frame's own camera rays: every third pixel of every third row"""
    o, d = h.s.camera_rays()
    return np.ascontiguousarray(o[::step, ::step].reshape(-1, 3)), np.ascontiguousarray(d[::step, ::step].reshape(-1, 3))


def camera_rays(h):
    o, d = h.s.camera_rays()
    return {"origin": o, "dir": d}


def trace_rays(h):
    o, d = _rows(h, 2)
    g = h.s.trace_rays(o, d, record=True)
    return {"hit_id": g["hit_id"], "hit_dist": g["hit_dist"], "hit_rec": g["hit_rec"]}


def visible(h):
    """from the camera rays' hit points to the first light and back towards the eye"""
    o, d = _rows(h, 2)
    g = h.s.trace_rays(o, d, record=True)
    hit = g["hit_id"] >= 0
    a = np.ascontiguousarray(g["hit_rec"][hit, 1:4])
    L = h.s.lights[0]
    target = np.array(L.center[:] if L.kind == 1 else L.pos[:])
    a2 = np.concatenate([a, a])
    b2 = np.concatenate([np.broadcast_to(target, a.shape), o[hit] + 0.25 * (a - o[hit])])
    vis, _ = h.s.visible(a2, np.ascontiguousarray(b2))
    return {"vis": vis, "segments": len(a2)}


def shade_whitted(h):
    o, d = _rows(h)
    return {"rgb": h.s.shade_rays(o, d, seed=42)}


def shade_paths(h):
    o, d = _rows(h)
    keys = (np.arange(len(o), dtype=np.uint32) * np.uint32(7) + np.uint32(11))
    return {"rgb": h.s.shade_rays(o, d, spp=3, seed=42, rng_skip=2, keys=keys)}


def device_frame(h):
    import torch
    W, H = h.s.frame_size
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda")
        h.s.render_device(out.data_ptr(), seed=42, stream=side.cuda_stream)
    side.synchronize()
    return {"rgb": out.cpu().numpy()}


def _refusal(h, fn):
    try:
        fn()
    except h.fray.FrayError as e:
        return {"code": e.code, "text": str(e)}
    raise AssertionError("the call was not refused")


def refused_adaptive(h):
    ans = _refusal(h, lambda: h.s.render_adaptive(0.05, min_spp=2, seed=42))
    assert ans["code"] == h.abi.E_UNSUPPORTED, ans
    return ans


def refused_argument(h):
    """frayhip_render without a frame to write: refused after the entry has cleared its statistics block and recorded its first event"""
    fr = h.abi.Frame(mode=h.abi.MODE_RENDER, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, flags=0)
    st = h.abi.Stats()
    rc = h.fray.lib.frayhip_render(h.s._dev, C.byref(fr), None, None, None, C.byref(st))
    assert rc == h.abi.E_ARG, rc
    return {"code": rc, "text": (h.fray.lib.frayhip_last_error() or b"").decode()}


class CallbackRaised(Exception):
    pass


def raising_callback(h):
    def progress(info):
        raise CallbackRaised("at %d of %d" % (info["samples_done"], info["samples_total"]))
    try:
        h.s.render(seed=42, spp_chunk=2, progress=progress)
    except CallbackRaised as e:
        return {"text": str(e)}
    raise AssertionError("the callback's exception was swallowed")


WHITTED = dict(gi=0, wantAA=0)
# scene -> the operations it refuses, which operations() leaves out.  None: run once each on a fresh handle, all four scenes accept all of theirs
# (cornell_box and csg_nested render Whitted frames with k_whitted, boxed with the wavefront launches, textured_plain fused and, at
# fused_whitted_max = 0, with the wavefront launches: the three values of whitted_path)
REFUSED = {}


def operations(name):
    """the operations of one scene, in a fixed order"""
    assert name in SCENE_FACTS, name
    ops = [
        Op("pt", frame()),
        Op("pt-chunk3", frame(spp_chunk=3)),
        Op("pt-seed43", frame(seed=43)),                # every other call's seed is 42: the seed table's planes are of another key
        Op("pt-97x61", frame(), dict(frameWidth=97, frameHeight=61)),
        Op("pt-33x17", frame(), dict(frameWidth=33, frameHeight=17)),
        Op("pt-share", frame(bucket_first=1, bucket_stride=3)),
        Op("pt-stats", frame(stats=True)),
        Op("pt-stereo", frame(), camera=dict(stereoSeparation=True)),
        Op("pt-deep", frame(), dict(frameWidth=32, frameHeight=24, maxTraceDepth=40)),
        Op("pt-contract", frame(), options=dict(fp_contract=1)),
        Op("pt-no-planes", frame(), options=dict(segment_planes=0)),
        Op("pt-no-certified", frame(), options=dict(certified_segments=0)),
        Op("pt-null-segments", frame(), options=dict(skip_null_segments=0)),
        Op("pt-no-seed-table", frame(), options=dict(seed_table_mib=0)),
        Op("pt-1-lane", frame(), options=dict(pt_lanes=1)),
        # 64 MiB is the floor work_budget() keeps under any option value: about 200 000 paths in flight, 22 samples a batch on three lanes at this size
        Op("pt-budget", budget_frame, dict(numPaths=80), options=dict(pt_budget_mib=1)),
        Op("whitted-aa", whitted_frame, dict(gi=0, wantAA=1), kind="whitted"),
        Op("whitted", whitted_frame, WHITTED, kind="whitted"),
        Op("whitted-unfused", whitted_frame, WHITTED, options=dict(fused_whitted_max=0), kind="whitted"),
        Op("primary", primary),
        Op("black", frame(), dict(maxTraceDepth=-1)),
        Op("progressive", progressive),
        # twelve samples in batches of two: more batches than the lanes have in flight when the first callback runs, so the cancel cuts the frame short
        Op("progressive-cancelled", progressive_cancelled, dict(numPaths=12)),
        Op("samples-3-5", samples_3_5),
        Op("samples-resumed", samples_resumed, dict(numPaths=12)),
        Op("adaptive", adaptive, kind="adaptive"),
        Op("features", features, kind="none"),
        Op("features-motion", features_motion, kind="none"),
        Op("camera-rays", camera_rays, kind="none"),
        Op("trace-rays", trace_rays, kind="none"),
        Op("visible", visible, kind="none"),
        Op("shade-whitted", shade_whitted, WHITTED, kind="none"),
        Op("shade-paths", shade_paths, kind="none"),
        Op("edit-node", frame(), tables="edit_node"),
        Op("edit-other", frame(), tables="edit_other"),
        Op("original-again", frame(spp_chunk=1)),
        Op("device-frame", device_frame),
        Op("refused-adaptive", refused_adaptive, dict(gi=0, wantAA=1), kind="none"),            # five samples a pixel: min_spp = 2 is in range, the integrator is not
        Op("refused-argument", refused_argument, kind="none"),
        Op("raising-callback", raising_callback),
    ]
    if name == "cornell_box":
        # the scene with eligible gates (its two blocks): the switch off hands render_impl the table's plain half; after every other operation, which sets it on
        ops.append(Op("pt-no-tight-gates", frame(), tight_gates=0))
    dropped = REFUSED.get(name, ())
    assert set(dropped) <= {o.name for o in ops}
    return [o for o in ops if o.name not in dropped]


# ---- sequences ----------------------------------------------------------------------------------------------------------------------------------
def euler(n, seed):
    """A closed walk over 0..n-1 in which every ordered pair (a, b), a = b included, is adjacent exactly once: an Eulerian circuit of the complete
    digraph with loops (Hierholzer, each vertex's successors in an order drawn from the seed).  n * n + 1 entries."""
    rng = random.Random(seed)
    succ = []
    for _ in range(n):
        order = list(range(n))
        rng.shuffle(order)
        succ.append(order)
    start = rng.randrange(n)
    stack, walk = [start], []
    while stack:
        v = stack[-1]
        if succ[v]:
            stack.append(succ[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and walk[0] == walk[-1]
    return walk


def arcs(walk, k):
    """the walk cut into consecutive arcs of at most k calls; each arc begins with the arc before's last entry, so that no adjacent pair is lost"""
    assert k >= 2
    out, i = [], 0
    while i < len(walk) - 1:
        out.append(list(walk[i:i + k]))
        i += k - 1
    return out


def big_then_small(ops):
    """every operation directly after the operation with the largest workspace (Op.work), and again directly after the one with the smallest"""
    work = [o.work for o in ops]
    assert all(w is not None for w in work), "Op.work is not measured"
    big, small = max(range(len(ops)), key=lambda i: (work[i], -i)), min(range(len(ops)), key=lambda i: (work[i], i))
    walk = []
    for i in range(len(ops)):
        walk += [big, i, small, i]
    return walk


def two_handles(walk_a, walk_b):
    """(handle, operation) call by call: a's first, b's first, a's second, ...; the longer walk's rest follows"""
    out = []
    for i in range(max(len(walk_a), len(walk_b))):
        if i < len(walk_a):
            out.append((0, walk_a[i]))
        if i < len(walk_b):
            out.append((1, walk_b[i]))
    return out


def adjacent_pairs(walks):
    return {(a, b) for w in walks for a, b in zip(w, w[1:])}


# ---- comparing ----------------------------------------------------------------------------------------------------------------------------------
def first_difference(base, got, skip=()):
    """None, or (key, index) of the first thing that differs: keys in the baseline's order, arrays by their bytes (shape and dtype first: index None)"""
    keys = [k for k in base if k not in skip]
    extra = [k for k in got if k not in skip and k not in base]
    if extra:
        return extra[0], None
    for k in keys:
        if k not in got:
            return k, None
        a, b = base[k], got[k]
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            a, b = np.asarray(a), np.asarray(b)
            if a.shape != b.shape or a.dtype != b.dtype:
                return k, None
            if a.tobytes() != b.tobytes():
                fa, fb = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
                item = max(a.dtype.itemsize, 1)
                byte = int(np.flatnonzero(fa.view(np.uint8) != fb.view(np.uint8))[0])
                return k, tuple(int(v) for v in np.unravel_index(byte // item, a.shape)) if a.ndim else ()
        elif a != b:
            return k, None
    return None


class Finding:
    def __init__(self, label, position, op, predecessor, key, index):
        self.label, self.position, self.op, self.predecessor, self.key, self.index = label, position, op, predecessor, key, index

    def __repr__(self):
        return "%s call %d: %s after %s differs from its baseline in %r at %s" % (self.label, self.position, self.op, self.predecessor or "nothing", self.key, self.index)


def run_walk(handle, ops, walk, baselines, skip=lambda handle, op: (), label="", predecessor=None):
    """Runs ops[i] for i in walk on the handle; every answer against baselines[i].  Returns the findings (all of them: the walk is not cut short).
    skip(handle, op): the answer keys that are not compared for this call."""
    found = []
    for pos, i in enumerate(walk):
        got = handle.run(ops[i])
        diff = first_difference(baselines[i], got, skip(handle, ops[i]))
        if diff is not None:
            found.append(Finding(label, pos, ops[i].name, predecessor, diff[0], diff[1]))
        predecessor = ops[i].name
    return found


def run_two(handles, ops, calls, baselines, skip=lambda handle, op: (), label=""):
    """two_handles' calls over two handles, each with its own operations and baselines; the predecessor named is the call before, on either handle"""
    found, before = [], None
    for pos, (w, i) in enumerate(calls):
        got = handles[w].run(ops[w][i])
        diff = first_difference(baselines[w][i], got, skip(handles[w], ops[w][i]))
        here = "%s:%s" % (handles[w].name, ops[w][i].name)
        if diff is not None:
            found.append(Finding(label, pos, here, before, diff[0], diff[1]))
        before = here
    return found
