"""The first bounce's tile table on the CPU (frayhip_scene_camera_tiles; fray_amd/csrc/dev_camtile.hpp, kernels.hpp k_cam_tiles).

tests/native/camtile_check.cpp runs the tile certificate -- dev_gatecert.hpp's certificate decided from a tile's four corner directions -- against the mesh's triangle
loop restated from the reference, in both arithmetics, on the miss records the product's own arena_build makes of cornell_box and of the generated rooms of
tests/test_gpu_tight_gate_shapes.py, and holds the table's pixel origin to item_pixel and to the bucket numbering of the C ABI."""
import os
import subprocess

import pytest

import scene_edits
import test_gpu_tight_gate_shapes as shapes
from test_gpu_segment_planes import room

ROOT = scene_edits.ROOT
CSRC = os.path.join(ROOT, "fray_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "native", "camtile_check.cpp")] + [os.path.join(CSRC, f) for f in ("host_scene.cpp", "host_loaders.cpp", "host_exr.cpp", "capi_host.cpp")]
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
CLASSES = 7
ZERO = ["-DFRAY_CAMTILE_SCALE=0", "-DFRAY_GATECERT_SCALE=0", "-DFRAY_MISSCERT_SCALE=0"]


def build(exe, flags):
    cmd = ["g++", "-std=c++17", "-ffp-contract=off"] + flags + INC + SRC + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + (r.stdout + r.stderr)[-6000:]
    return exe


@pytest.fixture(scope="module")
def rooms(tmp_path_factory):
    """cornell_box's seven meshes and the generated rooms: oblique faces, five and six directions, 32 triangles, a steep pyramid (guard 6e-3), the room at 1e-2 and 1e4"""
    base = tmp_path_factory.mktemp("camtile_rooms")

    def d(name):
        p = base / name
        p.mkdir()
        return p
    return [os.path.join(ROOT, "scenes", "cornell_box.fray"),
            room(d("octa"), extra=[("octa",) + shapes.octahedron(shapes.OCTA_C, shapes.OCTA_R)]),
            room(d("penta"), extra=[("penta",) + shapes.pyramid(5, (400.0, 380.0, 350.0), 50.0, 100.0)]),
            room(d("lprism"), extra=[("lprism",) + shapes.l_prism((400.0, 420.0, 200.0), 60.0, 40.0, 30.0)]),
            shapes.without_kd(room(d("strips"), extra=[("strips",) + shapes.strip_box(shapes.BOX_C, shapes.BOX_HALF)]), "strips"),
            room(d("steep"), extra=[shapes.steep_pyramid(False)]),
            room(d("small"), k=1e-2),
            room(d("big"), k=1e4)]


def per_class(out):
    """class -> (pairs, certified, refused, contradictions)"""
    got = {}
    for line in out.split("\n"):
        w = line.split()
        if len(w) == 6 and w[0] == "class" and w[1].endswith(":") and w[1][:-1].isdigit():
            got[int(w[1][:-1])] = tuple(int(x) for x in w[2:])
    assert sorted(got) == list(range(CLASSES)), out
    return got


def test_no_ray_of_a_certified_tile_has_a_triangle_accepted(rooms, tmp_path):
    """Random cameras and tiles; corner rays past edges and corners at 1e-4 .. 1e-9; tiles that straddle a silhouette; a camera in the plane of a face; a camera inside a
    mesh's box; directions at the guard threshold and far below it; ragged frames.  Every class certifies some (tile, record) pairs and refuses some, and no ray of a
    certified pair -- the rectangle's corners, jitter 0 and 0x1.fffffep-1f among them -- is accepted by a triangle of the mesh, in either arithmetic."""
    exe = build(str(tmp_path / "camtile_check"), ["-O2"])
    r = subprocess.run([exe, "1500000"] + rooms, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "contradictions 0" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    got = per_class(r.stdout)
    for c, (pairs, certified, refused, bad) in got.items():
        assert pairs > 100000 and certified > 1000 and refused > 1000 and bad == 0, (c, got[c])
    assert r.stdout.count(" records") == len(rooms) and "cornell_box.fray: 7 records" in r.stdout


def test_without_the_margins_the_harness_finds_contradictions(rooms, tmp_path):
    """The second build: no margins, no guard (the three scales 0), and the records' half extents no longer rounded up.  2 000 000 tiles on the same rooms: 39 789
    contradictions -- 1 585 among the corner rays past edges, 2 508 with the camera in the plane of a face, 35 118 with the camera inside a box, 578 among the
    directions below the guard; none among the random, straddling and ragged tiles, whose rays pass no outline by less than the margins.  (The three scales alone leave
    the round-up of the records' half extents, half a float ulp at least, which an FP64 evaluation never uses up: with it the second build found nothing in 3 000 000
    tiles.)"""
    exe = build(str(tmp_path / "camtile_check0"), ["-O2"] + ZERO)
    r = subprocess.run([exe, "1000000"] + rooms, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    got = per_class(r.stdout)
    bad = [got[c][3] for c in range(CLASSES)]
    print("contradictions per class:", bad)
    assert r.returncode == 1 and sum(bad) > 1000 and bad[1] > 0 and bad[3] > 0 and bad[4] > 0, r.stdout[-3000:]


def test_the_harness_is_clean_under_the_sanitizers(rooms, tmp_path):
    """the same program, stand-alone, built with AddressSanitizer and UndefinedBehaviorSanitizer: a shorter run, and the table's origin"""
    exe = build(str(tmp_path / "camtile_check_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "150000"] + rooms, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "contradictions 0" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    r = subprocess.run([exe, "--origin"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]


def test_the_tables_origin_is_item_pixels(tmp_path):
    """x0, y0 and the live mask a first-bounce lane takes from its tile's entry equal item_pixel for every item: 64 x 64, 50 x 44 and 200 x 120 as shares (0, 1), (1, 3)
    and (2, 3) -- the last of 50 x 44 owns no bucket: an empty table -- and 1920 x 1080 as (0, 1) and (3, 8); every pixel of a share once; the origin is the bucket's tile by
    frayhip_bucket_xy and fits the entry's 16 bits."""
    exe = build(str(tmp_path / "camtile_origin"), ["-O2"])
    r = subprocess.run([exe, "--origin"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.count("origin ") == 11 and "origin 1920x1080 first 0 stride 1: 33120 tiles" in r.stdout and "origin 50x44 first 2 stride 3: 0 tiles" in r.stdout
