"""Tight gates (tests/test_gpu_tight_gates.py) beyond Cornell's two blocks: the wiring that ships -- fill_editable making the records from loaded OBJ triangles
and writing both halves of the gate table, arena_update making them again after an edit, render_impl picking the half, ray_gate_class<true> evaluating guards,
range and box on the device -- on meshes with oblique faces and with all six direction slots in use, at the eligibility limits as the arena applies them, on
scaled rooms, with a full gate table and one candidate more, through every entry that renders with render_impl, across Scene.update() and with the switch preset
from the environment.  A wrong record or a wrong half of the table crashes nothing: it files a ray gate-free that a triangle accepts and a mesh loses pixels at
its silhouette, so every comparison here is bit equality or an exact integer.

The eligible counts asserted are the ones gatecert_make (fray_amd/csrc/dev_gatecert.hpp) gives on the host for the same files: tests/test_gate_table_host.py
parses each generated room with the product's parser, runs arena_build on the CPU and holds nTightGates, the segment-plane nodes, segCertAll and each record's
direction entries to the figures below.  Rooms are 48 x 48 x 4 spp, the size tests/test_gpu_tight_gates.py uses."""
import math
import os
import re
import sys

import numpy as np
import pytest

import scene_edits
from conftest import ROOT, open_scene, run_in_clean_child
from test_gpu_segment_planes import bits, fan, room
from test_gpu_tight_gates import on_off_counted_oracle

pytestmark = pytest.mark.gpu


# ---- meshes: three-index faces only, so that nothing depends on how the loader cuts polygons ----------------------------------------------------------
def octahedron(c, r):
    """eight faces, every one oblique: the normals (+-1, +-1, +-1), four directions once opposite ones share an entry"""
    cx, cy, cz = c
    vs = [(cx + r, cy, cz), (cx - r, cy, cz), (cx, cy + r, cz), (cx, cy - r, cz), (cx, cy, cz + r), (cx, cy, cz - r)]
    return vs, [(1, 3, 5), (3, 2, 5), (2, 4, 5), (4, 1, 5), (3, 1, 6), (2, 3, 6), (4, 2, 6), (1, 4, 6)]


def pyramid(n, c, r, h, phase=0.3):
    """n side faces and a base of n - 2 triangles in the plane y = c.y: n + 1 normal directions (no two sides are opposite: all lean upwards)"""
    cx, cy, cz = c
    vs = [(cx + r * math.cos(phase + 2 * math.pi * i / n), cy, cz + r * math.sin(phase + 2 * math.pi * i / n)) for i in range(n)] + [(cx, cy + h, cz)]
    return vs, [(1 + i, n + 1, 1 + (i + 1) % n) for i in range(n)] + [(1, 1 + i, 2 + i) for i in range(1, n - 1)]


def rot_y(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return lambda p: (c * p[0] + s * p[2], p[1], -s * p[0] + c * p[2])


def rot_x(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return lambda p: (p[0], c * p[1] - s * p[2], s * p[1] + c * p[2])


def l_prism(c, a, h, turn):
    """tests/native/gatecert_check.cpp's L: the square [-a, a]^2 without its (+, +) quarter, extruded from -h to h along y, turned about y -- not convex; two
    caps of four triangles and six sides of two: 20 triangles, three normal directions (the sides' rounded normals merge within 2^-30)"""
    px, pz = (-1, 1, 1, 0, 0, -1), (-1, -1, 0, 0, 1, 1)
    R = rot_y(turn)
    P = lambda i, y: tuple(p + q for p, q in zip(c, R((a * px[i], y, a * pz[i]))))
    vs = [P(i, -h) for i in range(6)] + [P(i, h) for i in range(6)]
    fs = []
    for o in (0, 6):
        fs += [(o + 1, o + 2, o + 3), (o + 1, o + 3, o + 4), (o + 1, o + 4, o + 5), (o + 1, o + 5, o + 6)]
    for i in range(6):
        j = (i + 1) % 6
        fs += [(1 + i, 1 + j, 7 + j), (1 + i, 7 + j, 7 + i)]
    return vs, fs


def strip_box(c, half, one_more=False):
    """a box turned out of every coordinate plane whose four sides are cut into three strips each and whose top and bottom into two: 16 quads, exactly 32
    triangles (FRAY_GATECERT_MAX_TRIS), three directions whose many rounded copies must merge.  A strip is 2 half / 3 wide and 2 half long: no sliver (nu = 3).
    one_more: the last triangle cut in two at the middle of an edge, 33 triangles."""
    turn = lambda p: rot_y(20.0)(rot_x(15.0)(p))
    vs, fs = [], []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        strips = 2 if axis == 1 else 3
        for sign in (-1.0, 1.0):
            for k in range(strips):
                u0, u1 = -half + 2 * half * k / strips, -half + 2 * half * (k + 1) / strips
                quad = []
                for uu, vv in ((u0, -half), (u1, -half), (u1, half), (u0, half)):
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[u], p[v] = sign * half, uu, vv
                    quad.append(tuple(a + b for a, b in zip(c, turn(p))))
                n = len(vs)
                vs += quad
                fs += [(n + 1, n + 2, n + 3), (n + 1, n + 3, n + 4)]
    if one_more:
        a, b, d = fs.pop()
        vs.append(tuple(0.5 * (p + q) for p, q in zip(vs[b - 1], vs[d - 1])))
        fs += [(a, b, len(vs)), (a, len(vs), d)]
    return vs, fs


OCTA_C, OCTA_R = (300.0, 200.0, 250.0), 80.0
BOX_C, BOX_HALF = (420.0, 400.0, 150.0), 50.0


def without_kd(path, name):
    """`useKDTree false` for one generated mesh: the loader gives a mesh of more than 20 triangles a KD-tree, and only a mesh without one is a gate"""
    text = open(path).read()
    old = "Mesh mesh_%s {\n" % name
    assert old in text
    open(path, "w").write(text.replace(old, old + "\tuseKDTree false\n"))
    return path


# name -> (mesh (name, vertices, faces), triangles, loaded without a KD-tree, eligible gates beyond the blocks' 2, segment-plane nodes beyond the walls' 5,
# certified_segments_eligible: every node is a plane node or exactly gated, tight or not).  All figures from the host's arena_build of the same files.
SHAPES = {
    "an octahedron, every face oblique": (lambda: ("octa",) + octahedron(OCTA_C, OCTA_R), 8, False, 1, 0, 1),
    "a pentagonal pyramid with its base, six directions": (lambda: ("penta",) + pyramid(5, (400.0, 380.0, 350.0), 50.0, 100.0), 8, False, 1, 0, 1),
    "a hexagonal pyramid with its base, seven directions": (lambda: ("hexa",) + pyramid(6, (400.0, 380.0, 350.0), 50.0, 100.0), 10, False, 0, 0, 1),
    "an L-shaped prism turned 30 degrees about y": (lambda: ("lprism",) + l_prism((400.0, 420.0, 200.0), 60.0, 40.0, 30.0), 20, False, 1, 0, 1),
    "a box cut into strips, 32 triangles": (lambda: ("strips",) + strip_box(BOX_C, BOX_HALF), 32, True, 1, 0, 1),
    "the same box with one more cut, 33 triangles": (lambda: ("strips",) + strip_box(BOX_C, BOX_HALF, one_more=True), 33, True, 0, 0, 1),
    # ... and as the loader makes it by default: a KD mesh is no gate, the scene's kernels are the KD variants, which are never handed the table's tight half
    "the box of 32 triangles with its KD-tree": (lambda: ("strips",) + strip_box(BOX_C, BOX_HALF), 32, False, 0, 0, 0),
    "a five-triangle fan, a plane node and no gate": (lambda: ("five",) + fan(380.0, 330.0, 250.0, 90.0, 5), 5, False, 0, 1, 1),
}


def render_room(fray, abi, oracle, path, what):
    s = fray.Scene.parseScene(path)
    s.beginRender()
    return (s,) + on_off_counted_oracle(s, abi, oracle, what)


@pytest.mark.parametrize("what", list(SHAPES), ids=lambda v: v.replace(" ", "_").replace(",", ""))
def test_shapes_render_the_same_bits(fray, abi, oracle, gpu, tmp_path, what):
    make, tris, no_kd, plus, plane_nodes, certifiable = SHAPES[what]
    mesh = make()
    assert len(mesh[2]) == tris and all(len(f) == 3 for f in mesh[2])
    path = room(tmp_path, extra=[mesh])
    s, eligible, (segs, cert), (segs_off, cert_off) = render_room(fray, abi, oracle, without_kd(path, mesh[0]) if no_kd else path, what)
    assert eligible == 2 + plus
    assert s.get_option("segment_plane_nodes") == 5 + plane_nodes
    assert s.get_option("certified_segments_eligible") == certifiable
    if certifiable:
        assert cert > 0 and cert_off > 0
    else:
        assert cert == 0 and cert_off == 0
    s.close()


def steep_pyramid(reverse):
    """a pentagonal pyramid 24 wide and 150 high: six directions again, and long thin sides that put its guard threshold at 6.2e-3 (the host's figure; the
    cap is 2^-6), a thousand times the other meshes' -- here about one direction in a hundred fails each entry's guard, so every entry decides segments"""
    vs, fs = pyramid(5, (420.0, 330.0, 380.0), 12.0, 150.0)
    return "steep", vs, fs[::-1] if reverse else fs


def test_every_direction_slot_decides(fray, abi, oracle, gpu, tmp_path):
    """The guard is a conjunction over the record's direction entries, so the segments certified cannot depend on the slots the directions stand in.  The same
    pyramid with its faces listed forwards (slots: the sides 0 .. 4, then the base) and backwards (the base, then the sides 4 .. 0): every slot holds another
    direction, and a slot that was left out, zeroed or not read on the device would certify other segments in the two rooms.  (With the other meshes' guards
    of 1e-5 a frame holds a handful of segments that a single entry decides; with this one hundreds: a scratch build that dropped the last entry certified
    more segments in one order than in the other, and one that zeroed it none.)"""
    got = []
    for reverse in (False, True):
        d = tmp_path / ("backwards" if reverse else "forwards")
        d.mkdir()
        s, eligible, fig_on, fig_off = render_room(fray, abi, oracle, room(d, extra=[steep_pyramid(reverse)]), "the steep pyramid, faces " + d.name)
        assert eligible == 3 and s.get_option("certified_segments_eligible") == 1
        got.append((fig_on, fig_off))
        s.close()
    (on_a, off_a), (on_b, off_b) = got
    assert on_a[1] > 0 and off_a[1] > 0
    assert on_a == on_b and off_a == off_b


# ---- scale ---------------------------------------------------------------------------------------------------------------------------------------------
# k -> (eligible gates, certified_segments_eligible), both from the host's arena_build of the same files.  A mesh is eligible while the largest |coordinate| of
# its own box, with the margin, stays under 2^24 (FRAY_GATECERT_MAX_COORD): at 3.6e4 the short block's 474 k passes it and keeps its bounding-box gate, the tall
# block (456 k) stays tight, and both gates stay exact (Mf < 1e9); at 1e5 neither is eligible and the switch changes nothing.  From 1e4 on a segment's start,
# 1e-6 off its surface, no longer clears the margin of the surface's own plane (scene_arena.hpp, the last condition of segCertAll): no segment is certified.
SCALES = {1e-2: (2, 1), 1e4: (2, 0), 3.6e4: (1, 0), 1e5: (0, 0)}


@pytest.mark.parametrize("k", list(SCALES), ids=lambda k: "k=%g" % k)
def test_scaled_rooms_render_the_same_bits(fray, abi, oracle, gpu, tmp_path, k):
    want, certifiable = SCALES[k]
    s, eligible, fig_on, fig_off = render_room(fray, abi, oracle, room(tmp_path, k=k), "the room scaled by %g" % k)
    assert eligible == want
    assert s.get_option("certified_segments_eligible") == certifiable
    if certifiable:
        assert fig_on[1] > 0 and fig_off[1] > 0
    else:
        assert fig_on[1] == fig_off[1] == 0
    if want == 0:
        assert fig_on == fig_off                                           # the two halves of the table are the same bytes
    s.close()


# ---- cameras that graze an oblique face -------------------------------------------------------------------------------------------------------------------
FACE_N = np.array([1.0, 1.0, -1.0])                                         # the octahedron's face (+x, +y, -z): its plane is (p - c) . N = r
FACE_T = np.array([1.0, 1.0, 2.0])                                          # a direction in that plane (N . T = 0): the cameras look along it
FACE_G = np.array(OCTA_C) + OCTA_R / 3.0 * FACE_N                           # the face's centroid


def look(front, up):
    """(yaw, pitch, roll) in degrees of the camera whose rotation rotZ(roll) rotX(pitch) rotY(yaw) has the rows right = up x front, up, front"""
    f, u = front / np.linalg.norm(front), up / np.linalg.norm(up)
    r = np.cross(u, f)
    pitch = math.asin(f[1])
    yaw = math.atan2(-f[0], f[2])
    roll = math.atan2(-r[1] / math.cos(pitch), u[1] / math.cos(pitch))
    return math.degrees(yaw), math.degrees(pitch), math.degrees(roll)


def with_camera(path, pos, front, up, fov):
    """the generated room's camera replaced (tests/test_gpu_tight_gates.py at_height moves it the same way)"""
    text = open(path).read()
    yaw, pitch, roll = look(front, up)
    new, n = re.subn(r"position \([^)]*\)\n\tyaw 0\n\tpitch 0\n\troll 0\n\tfov 50\n", "position (%r, %r, %r)\n\tyaw %r\n\tpitch %r\n\troll %r\n\tfov %r\n"
                     % (float(pos[0]), float(pos[1]), float(pos[2]), yaw, pitch, roll, fov), text)
    assert n == 1
    open(path, "w").write(new)
    return path


GRAZE_H, GRAZE_BACK, GRAZE_FOV = 0.5, 300.0, 2.0
# (a) the camera GRAZE_H above the face's plane, GRAZE_BACK behind the face's centroid along the viewing direction, the plane's normal its `up`: the middle row
# of pixels runs parallel to the face (|nf . d| is a rounding error), the rows below it come down onto the face at slopes of k * 5e-4, the rows above leave it.
# (b) the same camera moved 90 (-1, 1, 0) within the plane: its rays pass the box of the octahedron's own triangles, x in [220, 380], y in [120, 280], on the
# side y > 280 - (x - 220), but cross the mesh's bounding box, which the loader's dummy vertex (0, 0, 0) stretches to [0, 380] x [0, 280] x [0, 330] -- the
# rays that the two halves of the gate table treat differently, and among them those that only the guard sends back.
GRAZING = {"grazing the face": np.zeros(3), "beside the face": np.array([-90.0, 90.0, 0.0])}


def slab_hits(lo, hi, o, d):
    """float64 slab test of the lines' forward halves against the box [lo, hi], per ray"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d
    near, far = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
    return far >= np.maximum(near, 0.0)


@pytest.mark.parametrize("what", list(GRAZING), ids=lambda v: v.replace(" ", "_"))
def test_cameras_on_an_oblique_face(fray, abi, oracle, gpu, tmp_path, what):
    n, t = FACE_N / np.linalg.norm(FACE_N), FACE_T / np.linalg.norm(FACE_T)
    pos = FACE_G + GRAZE_H * n - GRAZE_BACK * t + GRAZING[what]
    path = with_camera(room(tmp_path, extra=[("octa",) + octahedron(OCTA_C, OCTA_R)]), pos, t, n, GRAZE_FOV)
    s = fray.Scene.parseScene(path)
    s.beginRender()
    # the census, on the CPU, before the comparison is trusted: r = |nf . d| / |d|_1 of the frame's own camera rays, nf = N / |N|_1.  A guard threshold lies in
    # [2^-18, 2^-6] (Gf = G + 2^-18; eligibility caps it), so rays with r < 2^-19 fail every guard and rays with r in (2^-18, 2^-10) lie around it.
    o, d = s.camera_rays()
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    r = np.abs(d @ (FACE_N / np.abs(FACE_N).sum())) / np.abs(d).sum(axis=1)
    low, mid = r < 2.0 ** -19, (r > 2.0 ** -18) & (r < 2.0 ** -10)
    lo_t, hi_t = np.array(OCTA_C) - OCTA_R, np.array(OCTA_C) + OCTA_R
    in_tight, in_box = slab_hits(lo_t - 1.0, hi_t + 1.0, o, d), slab_hits(np.zeros(3), hi_t, o, d)
    print("%s: %d rays; r < 2^-19: %d, 2^-18 < r < 2^-10: %d; of these %d + %d cross the triangles' box and %d + %d pass it inside the bounding box"
          % (what, len(r), low.sum(), mid.sum(), (low & in_tight).sum(), (mid & in_tight).sum(), (low & ~in_tight & in_box).sum(), (mid & ~in_tight & in_box).sum()))
    assert low.sum() >= 16 and mid.sum() >= 16
    if what == "beside the face":
        assert (low & ~in_tight & in_box).sum() >= 16 and (mid & ~in_tight & in_box).sum() >= 16
    else:
        assert (low & in_tight).sum() >= 16 and (mid & in_tight).sum() >= 16
    eligible, (segs, cert), (segs_off, cert_off) = on_off_counted_oracle(s, abi, oracle, what)
    assert eligible == 3
    assert s.get_option("certified_segments_eligible") == 1 and cert > 0 and cert_off > 0
    s.close()


# ---- the gate table's edge ---------------------------------------------------------------------------------------------------------------------------------
SMALL = [(90.0, 420.0, 120.0), (200.0, 440.0, 90.0), (330.0, 430.0, 110.0), (460.0, 420.0, 130.0), (120.0, 450.0, 480.0), (440.0, 450.0, 470.0), (280.0, 470.0, 430.0)]


def small_octahedra(n):
    """n translated copies of one small octahedron, each its own OBJ file and its own untransformed node"""
    return [("octa%d" % i,) + octahedron(SMALL[i], 25.0) for i in range(n)]


def test_eight_gated_meshes_fill_the_table(fray, abi, oracle, gpu, tmp_path):
    s, eligible, (segs, cert), (segs_off, cert_off) = render_room(fray, abi, oracle, room(tmp_path, extra=small_octahedra(6)), "eight gated meshes")
    assert eligible == 8                                                   # FRAY_MAX_GATES
    assert s.get_option("certified_segments_eligible") == 1 and cert > 0 and cert_off > 0
    s.close()


def test_a_ninth_mesh_gets_no_gate(fray, abi, oracle, gpu, tmp_path):
    """the ninth candidate is neither a plane node nor gated: nothing may be skipped on its account, and no segment is certified"""
    s, eligible, (segs, cert), (segs_off, cert_off) = render_room(fray, abi, oracle, room(tmp_path, extra=small_octahedra(7)), "eight gated meshes and a ninth")
    assert eligible == 8
    assert s.get_option("certified_segments_eligible") == 0
    assert cert == 0 and cert_off == 0
    s.close()


# ---- every way into render_impl ----------------------------------------------------------------------------------------------------------------------------
def samples_cut(s):
    """3 + 5 samples against 8 in one call, the states with their moment channel included"""
    _, st = s.render_samples(3, seed=42)
    rgb, st = s.render_samples(5, st, seed=42)
    whole, st8 = s.render_samples(8, seed=42)
    assert st.samples_done == st8.samples_done == 8 and st.state.shape[-1] >= 4
    assert np.array_equal(bits(rgb), bits(whole)) and st.state.tobytes() == st8.state.tobytes()
    return {"rgb": rgb, "state": st.state}


def components(s):
    direct, indirect, (sd, si) = s.render_components(8, seed=42)
    return {"direct": direct, "indirect": indirect, "state_direct": sd.state, "state_indirect": si.state}


def adaptive(s):
    rgb, spp, err, info = s.render_adaptive(0.05, min_spp=2, seed=42)
    counts = dict(zip(*(v.tolist() for v in np.unique(spp, return_counts=True))))
    print("adaptive: pixels per final sample count", counts)
    assert len(counts) >= 2                                                # pixels stop on at least two rungs
    return {"rgb": rgb, "spp": spp, "err": err, "rungs": np.array(info["rungs"]), "samples": np.array(info["samples"])}


def frame(**kw):
    return lambda s: {"rgb": s.render(seed=42, **kw)[0]}


def lanes_1_and_4(s):
    s.set_option("pt_lanes", 1)
    one, _ = s.render(seed=42)
    s.set_option("pt_lanes", 4)
    four, _ = s.render(seed=42)
    assert np.array_equal(bits(one), bits(four))
    return {"one": one, "four": four}


# name -> (width, height, settings and camera fields, call).  144 x 96 for the bucket subset: a 48 x 48 frame is one bucket, and a share that begins at
# bucket 1 would be empty; six buckets give it buckets 1 and 4.
ENTRIES = {
    "render_samples 3 + 5": (48, 48, dict(numPaths=8), samples_cut),
    "render_components": (48, 48, dict(numPaths=8), components),
    "render_adaptive": (48, 48, dict(numPaths=16), adaptive),
    "stereo": (48, 48, dict(numPaths=8, stereoSeparation=12.0), frame()),
    "maxTraceDepth 20": (48, 48, dict(numPaths=8, maxTraceDepth=20), frame()),
    "pt_lanes 1 against 4": (48, 48, dict(numPaths=8), lanes_1_and_4),
    "spp_chunk 1": (48, 48, dict(numPaths=8), frame(spp_chunk=1)),
    "a bucket subset": (144, 96, dict(numPaths=8), frame(bucket_first=1, bucket_stride=3)),
}


@pytest.mark.parametrize("what", list(ENTRIES), ids=lambda v: v.replace(" ", "_"))
def test_entries_answer_the_same_bits_with_the_switch_off(fray, gpu, what):
    W, H, over, call = ENTRIES[what]
    s = open_scene(fray, "cornell_box.fray", W, H, gi=1, wantAA=0, **over)
    s.beginRender()
    assert s.tight_gates() == (1, 2)
    on = call(s)
    assert s.tight_gates(0) == (0, 2)
    off = call(s)
    assert set(on) == set(off)
    for k in on:
        a, b = np.ascontiguousarray(on[k]), np.ascontiguousarray(off[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)
    assert any(np.asarray(v).dtype == np.float32 and float(np.abs(v).max()) > 0 for v in on.values())          # a picture, not a black frame
    s.close()


CHILD = """import sys
import numpy as np
import fray_amd
s = fray_amd.Scene.parseScene(sys.argv[1])
s.settings.frameWidth, s.settings.frameHeight, s.settings.gi, s.settings.wantAA, s.settings.numPaths = 48, 48, 1, 0, 8
s.beginRender(0)
enabled, eligible = s.tight_gates()
img, _ = s.render(seed=42)
np.save(sys.argv[2], img)
print("tight_gates %d %d" % (enabled, eligible))
s.close()
"""


def test_the_environment_presets_the_switch_off(fray, gpu, tmp_path):
    """FRAYHIP_TIGHT_GATES=0 is read once, when a handle is created: in a fresh child, whose environment it is -- this process's is left alone"""
    scene = os.path.join(ROOT, "scenes", "cornell_box.fray")
    out = str(tmp_path / "child.npy")
    log = run_in_clean_child([sys.executable, "-c", CHILD, scene, out], str(tmp_path / "child.log"), timeout=300, env=dict(os.environ, FRAYHIP_TIGHT_GATES="0"))
    assert "[exit code 0]" in log, log[-3000:]
    assert "tight_gates 0 2" in log, log[-3000:]
    assert "FRAYHIP_TIGHT_GATES" not in os.environ
    s = open_scene(fray, "cornell_box.fray", 48, 48, gi=1, wantAA=0, numPaths=8)
    s.beginRender()
    assert s.tight_gates() == (1, 2)
    mine, _ = s.render(seed=42)
    child = np.load(out)
    assert child.dtype == np.float32 and np.array_equal(bits(child), bits(mine)) and float(mine.max()) > 0
    s.close()


# ---- edits ---------------------------------------------------------------------------------------------------------------------------------------------------
def open_block_case(fray, tmp_path, tokens=()):
    s = fray.Scene.parseScene(scene_edits.scene_path(scene_edits.CASES["cornell-block"], tmp_path))
    s.settings.frameWidth, s.settings.frameHeight, s.settings.gi, s.settings.wantAA, s.settings.numPaths = 48, 48, 1, 0, 4
    if tokens:
        scene_edits.apply(fray, s, tokens)
    s.beginRender()
    return s


def on_and_off(s):
    """((enabled, eligible), certified_segments_eligible, the frame with the switch on, the frame with it off); the switch is left as it was found"""
    was, eligible = s.tight_gates()
    s.tight_gates(1)
    on, _ = s.render(seed=42)
    s.tight_gates(0)
    off, _ = s.render(seed=42)
    s.tight_gates(was)
    return (was, eligible), s.get_option("certified_segments_eligible"), on, off


def test_the_eligible_count_and_the_switch_across_updates(fray, gpu, tmp_path):
    """cornell-block (tests/scene_edits.py): the tall block is translated, put back, and the switch is turned off before another update.  After each step the
    handle is the one created from the edited description: the eligible count, certified_segments_eligible and the frames in both states of the switch."""
    case = scene_edits.CASES["cornell-block"]
    s = open_block_case(fray, tmp_path)
    fresh = on_and_off(s)
    assert fresh[0] == (1, 2) and fresh[1] == 1 and np.array_equal(bits(fresh[2]), bits(fresh[3]))
    # the block moves: a transformed mesh is no exact gate and gets no tight record; with an inexact gate in the scene no node may be skipped on a gate's word
    scene_edits.apply(fray, s, case["edit"])
    s.update()
    moved = on_and_off(s)
    b = open_block_case(fray, tmp_path, case["edit"])
    moved_fresh = on_and_off(b)
    b.close()
    assert moved[0] == moved_fresh[0] == (1, 1) and moved[1] == moved_fresh[1] == 0
    for k in (2, 3):
        assert np.array_equal(bits(moved[k]), bits(moved_fresh[k]))
    assert np.array_equal(bits(moved[2]), bits(moved[3])) and not np.array_equal(bits(moved[2]), bits(fresh[2]))
    # ... and comes back: both figures and both frames are the fresh handle's
    scene_edits.apply(fray, s, case["undo"])
    s.update()
    back = on_and_off(s)
    assert back[0] == fresh[0] and back[1] == fresh[1]
    for k in (2, 3):
        assert np.array_equal(bits(back[k]), bits(fresh[k]))
    # the switch survives an update as an option does
    assert s.tight_gates(0) == (0, 2)
    scene_edits.apply(fray, s, case["edit"])
    s.update()
    assert s.tight_gates() == (0, 1)
    kept = on_and_off(s)
    assert kept[0] == (0, 1) and s.tight_gates() == (0, 1)
    for k in (2, 3):
        assert np.array_equal(bits(kept[k]), bits(moved_fresh[k]))
    s.close()
