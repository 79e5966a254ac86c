"""frayhip_scene_update on the GPU (include/frayhip.h "scene edits"): a handle whose description was edited and pushed with Scene.update() must be
indistinguishable, bit for bit, from a handle created from the edited description -- pictures, hit records, work counters, read-only figures --
and from the CPU oracle's picture of the edited description, which does not go through frayhip_scene_create at all.  The edit cases are those
of tests/test_scene_update_host.py (tests/scene_edits.py).  Frames are at most 96 x 96 (four buckets) at 4 samples per pixel."""
import os
import sys

import numpy as np
import pytest

import scene_edits
from conftest import ROOT, run_in_clean_child
from scene_edits import CASES

pytestmark = pytest.mark.gpu

SPP = 4
SIZES = {"cornell_box.fray": (96, 96), "../tests/scenes/csg_nested.fray": (96, 72), "boxed.fray": (96, 72), "glossy": (64, 48)}
COUNTERS = ("closest_rays", "shadow_rays", "node_tests", "kd_inner_visits", "leaf_refs", "tri_tests", "prim_tests", "smooth_hits", "samples", "texture_fetches",
            "trace_launches", "shadow_launches", "alg_bytes_trace", "alg_bytes_shadow", "alg_flops_trace", "alg_flops_shadow")


def open_case(fray, name, tmp_path, gi=None, spp=SPP):
    case = CASES[name]
    s = fray.Scene.parseScene(scene_edits.scene_path(case, tmp_path))
    s.settings.frameWidth, s.settings.frameHeight = SIZES[case["scene"]]
    s.settings.wantAA = 0
    if gi is not None:
        s.settings.gi = gi
    s.settings.numPaths = spp
    return s


def updated_and_fresh(fray, name, tmp_path, gi=None):
    """A: created from the original, a frame rendered (so that its workspace, lanes and seed table are warm), then edited and update()d.
    B: created from the edited description."""
    a = open_case(fray, name, tmp_path, gi)
    a.beginRender()
    before, _ = a.render(seed=42)
    scene_edits.apply(fray, a, CASES[name]["edit"])
    a.update()
    b = open_case(fray, name, tmp_path, gi)
    scene_edits.apply(fray, b, CASES[name]["edit"])
    b.beginRender()
    return a, b, before


def figures(s):
    return {k: s.get_option(k) for k in ("segment_plane_nodes", "whitted_path", "shadow_nodes_skipped", "contracted_launches", "shadow_segments",
                                         "fans_filed", "fan_children", "batch_lanes")}


def assert_same_handle(a, b):
    ia, da, _ = a.primary_hits()
    ib, db, _ = b.primary_hits()
    assert np.array_equal(ia, ib) and np.array_equal(da, db)
    fa, _ = a.render(seed=42)
    fb, _ = b.render(seed=42)
    assert np.array_equal(fa, fb) and np.all(np.isfinite(fa))
    assert figures(a) == figures(b)
    sa, sta = a.render(seed=42, stats=True)
    sb, stb = b.render(seed=42, stats=True)
    assert np.array_equal(sa, sb) and np.array_equal(sa, fa)
    assert {k: sta[k] for k in COUNTERS} == {k: stb[k] for k in COUNTERS}
    # the torch device entries: the frame's camera rays with hit records, one visibility batch and one radiance batch
    import torch
    org, dirs = a.camera_rays()
    o, d = torch.from_numpy(org).cuda(), torch.from_numpy(dirs).cuda()
    ra, rb = a.trace_rays(o, d, record=True, stats=True), b.trace_rays(o, d, record=True, stats=True)
    for k in ("hit_id", "hit_dist", "hit_rec"):
        assert torch.equal(ra[k], rb[k]), k
    assert np.array_equal(ra["hit_id"].cpu().numpy(), ia)
    assert {k: ra["stats"][k] for k in COUNTERS} == {k: rb["stats"][k] for k in COUNTERS}
    ends = ra["hit_rec"][..., 1:4].contiguous()                                 # from every pixel's hit point (the origin for a miss) to the eye
    va, _ = a.visible(ends, o)
    vb, _ = b.visible(ends, o)
    assert torch.equal(va, vb)
    ca, cb = a.shade_rays(o, d, spp=2, seed=42), b.shade_rays(o, d, spp=2, seed=42)
    assert torch.equal(ca, cb)
    # ... and the contracted kernels with their figures
    a.set_option("fp_contract", 1)
    b.set_option("fp_contract", 1)
    ga, _ = a.render(seed=42)
    gb, _ = b.render(seed=42)
    assert np.array_equal(ga, gb) and figures(a) == figures(b)
    return fa


CORNELL = ["cornell-block", "cornell-wall", "cornell-shader", "cornell-light"]


@pytest.mark.parametrize("gi", [1, 0])
@pytest.mark.parametrize("name", CORNELL)
def test_updated_cornell_handle_is_the_fresh_one(fray, gpu, tmp_path, name, gi):
    a, b, before = updated_and_fresh(fray, name, tmp_path, gi)
    frame = assert_same_handle(a, b)
    assert not np.array_equal(frame, before)                                    # the edit shows
    if name == "cornell-wall":
        assert a.get_option("segment_plane_nodes") == 4
    a.close(); b.close()


@pytest.mark.parametrize("name", ["csg-nested", "boxed-textured", "glossy-fan", "glossy-rect"])
def test_updated_handle_is_the_fresh_one(fray, gpu, tmp_path, name):
    a, b, before = updated_and_fresh(fray, name, tmp_path)
    frame = assert_same_handle(a, b)
    assert not np.array_equal(frame, before)
    a.close(); b.close()


def test_csg_nested_path_traced_too(fray, gpu, tmp_path):
    a, b, _ = updated_and_fresh(fray, "csg-nested", tmp_path, gi=1)
    assert_same_handle(a, b)
    a.close(); b.close()


def test_render_samples_reads_the_new_scene(fray, gpu, tmp_path):
    """Two render_samples calls with an update() in between; the second, on a fresh Accumulation, is the edited scene's frame."""
    a = open_case(fray, "cornell-block", tmp_path, gi=1)
    a.beginRender()
    first, state = a.render_samples(SPP, None, seed=42)
    scene_edits.apply(fray, a, CASES["cornell-block"]["edit"])
    a.update()
    second, state2 = a.render_samples(SPP, None, seed=42)
    b = open_case(fray, "cornell-block", tmp_path, gi=1)
    scene_edits.apply(fray, b, CASES["cornell-block"]["edit"])
    b.beginRender()
    ref, _ = b.render(seed=42)
    assert state2.samples_done == SPP and np.array_equal(second, ref) and not np.array_equal(first, ref)
    a.close(); b.close()


@pytest.mark.parametrize("name,gi", [("cornell-block", 1), ("csg-nested", None), ("boxed-textured", None)])
def test_updated_handle_against_the_oracle(fray, abi, oracle, gpu, tmp_path, name, gi):
    a = open_case(fray, name, tmp_path, gi)
    a.beginRender()
    a.render(seed=42)
    scene_edits.apply(fray, a, CASES[name]["edit"])
    a.update()
    img, _ = a.render(seed=42)
    ref, _ = oracle.render(a.desc, abi.MODE_RENDER, seed=42)
    ids, dist, _ = a.primary_hits()
    oi, od, _ = oracle.render(a.desc, abi.MODE_PRIMARY_ID)
    same = float((img == ref).all(axis=2).mean())
    print("%s: %.3f %% of the pixels bit-identical to the oracle" % (name, 100 * same))
    assert np.array_equal(ids, oi) and np.array_equal(dist, od)
    assert ref.mean() > 1e-3 and np.array_equal(img, ref)
    a.close()


def test_round_trip_and_twenty_updates(fray, gpu, tmp_path):
    case = CASES["cornell-block"]
    s = open_case(fray, "cornell-block", tmp_path, gi=1)
    s.beginRender()
    original, _ = s.render(seed=42)
    scene_edits.apply(fray, s, case["edit"])
    s.update()
    moved, _ = s.render(seed=42)
    scene_edits.apply(fray, s, case["undo"])
    s.update()
    back, _ = s.render(seed=42)
    assert not np.array_equal(moved, original) and np.array_equal(back, original)
    assert s.get_option("scene_updates") == 2
    for k in range(18):
        scene_edits.apply(fray, s, case["edit"] if k % 2 == 0 else case["undo"])
        s.update()
    assert s.get_option("scene_updates") == 20
    again, _ = s.render(seed=42)
    assert np.array_equal(again, original)
    s.close()


def test_what_an_update_keeps(fray, gpu, tmp_path):
    s = open_case(fray, "cornell-block", tmp_path, gi=1)
    s.beginRender()
    options = {"pt_lanes": 3, "skip_null_segments": 0, "seed_table_mib": 512, "fused_whitted_max": 7, "speculate_fans": 0, "segment_planes": 0, "pt_budget_mib": 2048}
    for k, v in options.items():
        s.set_option(k, v)
    s.render(seed=42)
    table = s.get_option("seed_table_bytes")
    assert s.get_option("seed_launches") > 0 and table > 0
    scene_edits.apply(fray, s, CASES["cornell-block"]["edit"])
    s.update()
    assert s.get_option("seed_table_bytes") == table
    s.render(seed=42)
    assert s.get_option("seed_launches") == 0 and s.get_option("seed_planes_reused") == SPP
    assert s.get_option("seed_table_bytes") == table
    assert {k: s.get_option(k) for k in options} == options
    s.close()


CUBE_OBJ = "".join("v %d %d %d\n" % (x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)) + \
    "f 1 2 4\nf 1 4 3\nf 5 8 6\nf 5 7 8\nf 1 5 6\nf 1 6 2\nf 3 4 8\nf 3 8 7\nf 1 3 7\nf 1 7 5\nf 2 6 8\nf 2 8 4\n"

ONE_MESH = """GlobalSettings {
	frameWidth 64
	frameHeight 48
	ambientLight (0.2, 0.2, 0.2)
	wantAA off
}
Camera camera {
	position (0, 4, -14)
	fov 60
}
PointLight p0 {
	pos (-6, 12, -8)
	power 300
}
Plane ground {
	y -2
	limit 40
}
Mesh thing {
	file "%s"
}
Lambert grey {
	color (0.6, 0.6, 0.6)
}
Node floorNode {
	geometry ground
	shader grey
}
Node thingNode {
	geometry thing
	shader grey
	scale (2, 2, 2)
}
"""


def test_cost_does_not_depend_on_the_mesh(fray, gpu, tmp_path):
    """Two scenes that differ in the mesh a node points to, 12 triangles against teapot_hires.obj: the same transform edit uploads the same bytes,
    and far less than the arena holds for the teapot's triangles."""
    with open(tmp_path / "cube.obj", "w") as f:
        f.write(CUBE_OBJ)
    teapot = os.path.relpath(os.path.join(ROOT, "scenes", "geom", "teapot_hires.obj"), str(tmp_path))
    out = {}
    for tag, mesh in (("cube", "cube.obj"), ("teapot", teapot)):
        path = tmp_path / (tag + ".fray")
        with open(path, "w") as f:
            f.write(ONE_MESH % mesh)
        s = fray.Scene.parseScene(str(path))
        s.beginRender()
        before, _ = s.render(seed=42)
        fray.Transform(s.nodes[1]).rotate(30, 0, 0).translate(1, 0.5, 0).store(s.nodes[1])
        s.update()
        after, _ = s.render(seed=42)
        assert not np.array_equal(before, after)
        m = s.desc.meshes[0]
        # DTri 128 B and DTriAttr 168 B per triangle, DTri 128 B again per leaf reference (fray_amd/csrc/dev_scene.hpp)
        out[tag] = (s.get_option("scene_update_bytes"), s.get_option("arena_bytes"), m.n_triangles * (128 + 168) + m.n_trirefs * 128, m.n_triangles)
        s.close()
    print(out)
    assert out["cube"][3] == 12 and out["teapot"][3] > 1000
    assert out["cube"][0] == out["teapot"][0] > 0
    assert out["teapot"][0] < out["teapot"][1] - out["teapot"][2]
    assert out["teapot"][0] < 65536 < out["teapot"][2]


def test_refusals_leave_the_scene_unedited(fray, abi, gpu, tmp_path):
    s = open_case(fray, "csg-nested", tmp_path)                               # it has every table: CSG operands, a mesh, a texture
    s.beginRender()
    original, _ = s.render(seed=42)
    d = s.desc

    def refused(what):
        with pytest.raises(fray.FrayError) as e:
            s.update()
        assert e.value.code == abi.E_ARG and "frayhip_scene_update" in str(e.value), what
        return str(e.value)

    d.n_nodes -= 1
    assert "count" in refused("count")
    d.n_nodes += 1
    d.geoms[3].index ^= 1
    assert "geoms[]" in refused("geoms")
    d.geoms[3].index ^= 1
    d.csgs[0].op = (d.csgs[0].op + 1) % 3
    assert "csgs[]" in refused("csgs")
    d.csgs[0].op = (d.csgs[0].op + 2) % 3
    d.meshes[0].n_triangles += 1
    assert "meshes[]" in refused("mesh header")
    d.meshes[0].n_triangles -= 1
    d.textures[0].kind = abi.TEX_FRESNEL if hasattr(abi, "TEX_FRESNEL") else 3
    assert "textures[]" in refused("texture kind")
    d.textures[0].kind = 0
    # a sound edit and an unsound one in the same call: neither may land
    keep = bytes(s.nodes[1])
    fray.Transform(s.nodes[1]).translate(0, 3, 0).store(s.nodes[1])
    s.nodes[2].shader = d.n_shaders
    assert "node reference out of range" in refused("shader index")
    s.nodes[2].shader = 2
    assert s.get_option("scene_updates") == 0
    frame, _ = s.render(seed=42)
    assert np.array_equal(frame, original)

    codes = []

    def progress(info):
        try:
            s.update()
            codes.append(0)
        except fray.FrayError as e:
            codes.append(e.code)
        return False
    frame, _ = s.render(seed=42, progress=progress)
    assert codes and all(c == abi.E_ARG for c in codes) and np.array_equal(frame, original) and s.get_option("scene_updates") == 0
    # the same description is accepted once the frame is over, and now the moved node shows
    s.update()
    moved, _ = s.render(seed=42)
    assert s.get_option("scene_updates") == 1 and not np.array_equal(moved, original)
    import ctypes as C
    C.memmove(C.byref(s.nodes[1]), keep, len(keep))
    s.update()
    back, _ = s.render(seed=42)
    assert np.array_equal(back, original)
    s.close()


def test_cli_move(fray, gpu, tmp_path):
    """python -m fray_amd --frames 2 --move 6 10 0 0 in a clean child: frame 1 is the library's frame of the scene with node 6 moved by (10, 0, 0)."""
    out = str(tmp_path / "seq.bmp")
    cmd = [sys.executable, "-m", "fray_amd", os.path.join(ROOT, "scenes", "cornell_box.fray"), "--frames", "2", "--move", "6", "10", "0", "0",
           "--width", "96", "--height", "96", "--spp", str(SPP), "-o", out]
    log = run_in_clean_child(cmd, str(tmp_path / "cli.log"), timeout=300)
    assert "[exit code 0]" in log and "Rendered 2 frames" in log, log[-3000:]
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    s.settings.frameWidth, s.settings.frameHeight, s.settings.numPaths = 96, 96, SPP
    s.beginRender()
    for k in range(2):
        img, _ = s.render(seed=42)
        ref = str(tmp_path / ("ref_%d.bmp" % k))
        assert fray.lib.frayhip_save_bmp(ref.encode(), img.ctypes.data, 96, 96) == 0
        assert open(ref, "rb").read() == open(str(tmp_path / ("seq_%04d.bmp" % k)), "rb").read(), k
        fray.Transform(s.nodes[6]).translate(10, 0, 0).store(s.nodes[6])
        s.update()
    assert open(str(tmp_path / "ref_0.bmp"), "rb").read() != open(str(tmp_path / "ref_1.bmp"), "rb").read()
    s.close()
