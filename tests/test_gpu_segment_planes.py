"""Option "segment_planes" (default 1): k_pt_shadow's timed variants for untransformed scenes skip, per wave, the small tree-less meshes whose triangles'
planes no live next-event segment crosses (fray_amd/csrc/dev_segcert.hpp: the certificate and its proof; tests/test_segcert.py runs it on the host).  A
skipped node is one the reference's arithmetic could not make occlude any of the wave's segments, so no picture may change by a single bit: with the
option on or off, against the counting kernels (which ask every node) and against the oracle."""
import os

import numpy as np
import pytest

from conftest import SCENES, open_scene

pytestmark = pytest.mark.gpu


def bits(img):
    return np.ascontiguousarray(img).view(np.uint32)        # integer views: +0 and -0 differ, NaNs compare by payload


def on_off_counted_oracle(s, abi, oracle, what):
    """Renders the scene with the option on, off, on the counting kernels and on the oracle; asserts the four frames equal by bits, and on against off in
    the contracted arithmetic.  Returns (eligible nodes, nodes skipped with the option on, shadow segments, the counting pass's figures)."""
    assert s.get_option("segment_planes") == 1                                        # the default
    on, _ = s.render(seed=42)
    nodes, skipped, segs = s.get_option("segment_plane_nodes"), s.get_option("shadow_nodes_skipped"), s.get_option("shadow_segments")
    s.set_option("segment_planes", 0)
    assert s.get_option("segment_planes") == 0
    off, _ = s.render(seed=42)
    skipped_off = s.get_option("shadow_nodes_skipped")
    counted_off, st_off = s.render(seed=42, stats=True)
    s.set_option("segment_planes", 1)
    counted, st = s.render(seed=42, stats=True)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    # a wave iteration serves at most 64 segments, so segs / 64 is a lower bound of the iterations: the printed figure is an upper bound of nodes per iteration
    print("%s: %d eligible nodes, shadow_nodes_skipped %d with the option (at most %.2f per wave iteration of 64 segments), %d without; %d shadow segments; mean %g"
          % (what, nodes, skipped, skipped / max(segs / 64.0, 1.0), skipped_off, segs, float(ref.mean())))
    assert skipped_off == 0
    assert np.array_equal(bits(on), bits(off))
    assert np.array_equal(bits(on), bits(counted))
    assert np.array_equal(bits(on), bits(ref))
    # The counting kernels keep asking every node: the option does not reach them, so their figures are the same with it on and off, exactly ...
    assert np.array_equal(bits(counted), bits(counted_off))
    print("   work counters GPU - oracle:", {k: int(st[k]) - int(ost[k]) for k in ("shadow_rays", "node_tests", "tri_tests")})
    for k in ("shadow_rays", "node_tests", "tri_tests"):
        assert st[k] == st_off[k], (k, st[k], st_off[k])
    # ... and the oracle's as far as they ever were (tests/test_gpu_parity.py): rays and node tests exactly; the count of triangle tests moves by a few per
    # million with or without this option, where the device's correctly rounded sin / cos / acos differ from glibc's in a direction's last place and a box
    # test at an edge goes the other way without changing any hit
    for k in ("shadow_rays", "node_tests"):
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert abs(st["tri_tests"] - ost["tri_tests"]) <= 2e-5 * ost["tri_tests"] + 2, (st["tri_tests"], ost["tri_tests"])
    # the kernels built with fused multiply-adds are the same source: on against off, bit for bit
    s.set_option("fp_contract", 1)
    con, _ = s.render(seed=42)
    skipped_con = s.get_option("shadow_nodes_skipped")
    s.set_option("segment_planes", 0)
    coff, _ = s.render(seed=42)
    assert np.array_equal(bits(con), bits(coff))
    s.set_option("segment_planes", 1)
    s.set_option("fp_contract", 0)
    return nodes, skipped, segs, skipped_con


PT = [
    ("cornell_box.fray", 64, 64, dict(numPaths=8), 5),
    ("cornell_box.fray", 60, 60, dict(numPaths=8, stereoSeparation=12.0), 5),         # the right eye continues the left eye's generators
    ("cornell_box.fray", 40, 40, dict(numPaths=8, maxTraceDepth=20), 5),              # the long generators
    ("smallpt.fray", 64, 48, dict(numPaths=8), 0),                                    # no mesh: the feature is absent
    ("boxed.fray", 48, 36, dict(numPaths=8), 0),                                      # KD meshes: the kernel variants without the shortcut
]


@pytest.mark.parametrize("scene,W,H,over,eligible", PT, ids=lambda v: v if isinstance(v, str) else None)
def test_frames_are_the_same_bits_with_and_without_segment_planes(fray, abi, oracle, gpu, scene, W, H, over, eligible):
    s = open_scene(fray, scene, W, H, gi=1, **over)
    s.beginRender()
    nodes, skipped, segs, skipped_con = on_off_counted_oracle(s, abi, oracle, "%s %s" % (scene, over))
    assert nodes == eligible
    if eligible == 0:
        assert skipped == 0 and skipped_con == 0
    s.close()


def test_cornell_box_skips_nodes(fray, abi, oracle, gpu):
    """The shortcut must actually run on the scene it was made for: five eligible nodes (the walls), nodes skipped with the option on, none with it off."""
    s = open_scene(fray, "cornell_box.fray", 128, 128, gi=1, numPaths=8)
    s.beginRender()
    nodes, skipped, segs, skipped_con = on_off_counted_oracle(s, abi, oracle, "cornell_box 128 x 128 x 8 spp")
    assert nodes == 5
    assert skipped > 0 and skipped_con > 0
    s.close()


# ---- generated scenes: the Cornell room's own meshes, scaled / moved / joined by others, written into tmp_path ----

def read_obj(name):
    vs, fs = [], []
    for line in open(os.path.join(SCENES, "cornell", name)).read().replace("f ", "\nf ").splitlines():
        t = line.split()
        if t and t[0] == "v":
            vs.append(tuple(float(x) for x in t[1:4]))
        elif t and t[0] == "f":
            fs.append(tuple(int(x) for x in t[1:]))
    return vs, fs


def write_obj(path, vs, fs):
    with open(path, "w") as f:
        for v in vs:
            f.write("v %r %r %r\n" % v)
        for q in fs:
            f.write("f " + " ".join(str(i) for i in q) + "\n")


WALLS = ["floor", "ceiling", "backwall", "rightwall", "leftwall"]
BLOCKS = ["shortblock", "tallblock"]


def room(tmp_path, k=1.0, extra=(), node_lines=None, light=None, spp=4, size=48):
    """The Cornell box with every coordinate scaled by k; extra: (name, vertices, faces) meshes added as white nodes; node_lines: name -> extra lines of a node."""
    node_lines = node_lines or {}
    text = ["GlobalSettings {\n\tframeWidth %d\n\tframeHeight %d\n\tambientLight (0.15, 0.15, 0.15)\n\tmaxTraceDepth 6\n\tgi 1\n\twantAA false\n\tpathsPerPixel %d\n}" % (size, size, spp),
            "Camera camera {\n\tposition (%r, %r, %r)\n\tyaw 0\n\tpitch 0\n\troll 0\n\tfov 50\n\taspectRatio 1\n}" % (278.0 * k, 273.0 * k, -800.0 * k),
            light or "RectLight {\n\tscale (%r, 1, %r)\n\ttranslate (%r, %r, %r)\n\txSubd 4\n\tySubd 4\n\tcolor (1, 0.85, 0.43)\n\tpower %r\n}"
            % (130.0 * k, 105.0 * k, 278.0 * k, 547.7 * k, 279.5 * k, 27.47 * k * k),
            "Lambert white {\n\tcolor (0.76, 0.75, 0.5)\n}", "Lambert green {\n\tcolor (0.15, 0.48, 0.09)\n}", "Lambert red {\n\tcolor (0.63, 0.06, 0.04)\n}"]
    meshes = []
    for name in WALLS + BLOCKS:
        vs, fs = read_obj(name + ".obj")
        meshes.append((name, [tuple(c * k for c in v) for v in vs], fs))
    meshes += list(extra)
    for name, vs, fs in meshes:
        write_obj(str(tmp_path / (name + ".obj")), vs, fs)
        shader = "green" if name == "rightwall" else "red" if name == "leftwall" else "white"
        text.append("Mesh mesh_%s {\n\tfile \"%s.obj\"\n}" % (name, name))
        text.append("Node %s {\n\tgeometry mesh_%s\n\tshader %s\n%s}" % (name, name, shader, "".join("\t%s\n" % l for l in node_lines.get(name, []))))
    f = tmp_path / "room.fray"
    f.write_text("\n\n".join(text) + "\n")
    return str(f)


def fan(cx, cy, cz, r, n):
    """n triangles around a centre, tilted out of every coordinate plane"""
    vs = [(cx, cy, cz)] + [(cx + r * np.cos(2 * np.pi * i / n), cy + 0.3 * r * np.sin(4 * np.pi * i / n), cz + r * np.sin(2 * np.pi * i / n)) for i in range(n)]
    vs = [tuple(float(c) for c in v) for v in vs]
    return vs, [(1, 2 + i, 2 + (i + 1) % n) for i in range(n)]


def coplanar_scene(tmp_path):
    """Two coplanar disjoint quads with the RectLight in their plane (y = 300): every light sample has sigma_b = 0 against their plane, which therefore never
    certifies; a floor below them receives the light, past and between the quads."""
    quadA = ("quad_a", [(0.0, 300.0, 100.0), (150.0, 300.0, 100.0), (150.0, 300.0, 400.0), (0.0, 300.0, 400.0)], [(1, 2, 3, 4)])
    quadB = ("quad_b", [(400.0, 300.0, 100.0), (550.0, 300.0, 100.0), (550.0, 300.0, 400.0), (400.0, 300.0, 400.0)], [(1, 2, 3, 4)])
    light = "RectLight {\n\tscale (130, 1, 105)\n\ttranslate (278, 300, 250)\n\txSubd 4\n\tySubd 4\n\tcolor (1, 0.85, 0.43)\n\tpower 27.47\n}"
    return room(tmp_path, extra=[quadA, quadB], light=light)


GENERATED = {
    "coplanar quads, the light in their plane": (lambda p: coplanar_scene(p), 7),
    "a one-triangle and a five-triangle mesh": (lambda p: room(p, extra=[("one", [(100.0, 100.0, 300.0), (250.0, 130.0, 320.0), (160.0, 260.0, 280.0)], [(1, 2, 3)]),
                                                                          ("five",) + fan(380.0, 330.0, 250.0, 90.0, 5)]), 7),
    "a non-planar quad": (lambda p: room(p, extra=[("warped", [(100.0, 400.0, 100.0), (300.0, 430.0, 100.0), (300.0, 400.0, 300.0), (100.0, 370.0, 300.0)], [(1, 2, 3, 4)])]), 6),
    "the room scaled by 1e4": (lambda p: room(p, k=1e4), 5),
    "the room scaled by 1e-2": (lambda p: room(p, k=1e-2), 5),
    "one wall with a transform": (lambda p: room(p, node_lines={"backwall": ["translate (0, 0, 3)"]}), 4),
    "a mesh with a degenerate triangle": (lambda p: room(p, extra=[("degenerate", [(100.0, 100.0, 300.0), (250.0, 130.0, 320.0), (160.0, 260.0, 280.0), (175.0, 115.0, 310.0)],
                                                                    [(1, 2, 3), (1, 2, 4)])]), 5),        # (vertex 4 is the midpoint of 1-2: AB x AC = 0)
}


@pytest.mark.parametrize("what", list(GENERATED), ids=lambda v: v.replace(" ", "_").replace(",", ""))
def test_generated_scenes_render_the_same_bits(fray, abi, oracle, gpu, tmp_path, what):
    make, eligible = GENERATED[what]
    s = fray.Scene.parseScene(make(tmp_path))
    s.beginRender()
    nodes, skipped, segs, skipped_con = on_off_counted_oracle(s, abi, oracle, what)
    assert nodes == eligible
    s.close()
