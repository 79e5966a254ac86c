"""The first bounce's miss records on the CPU (frayhip_scene_camera_skip; fray_amd/csrc/dev_scene.hpp DCamSkip, dev_trace.hpp camera_skip_nodes).

tests/native/camskip_check.cpp runs the certificate of fray_amd/csrc/dev_gatecert.hpp on flat two-triangle quads -- the Cornell walls and generated ones -- whose
boxes have no extent in one axis, against the triangle test and the mesh loop restated from the reference, in both arithmetics.
tests/native/camskip_table_check.cpp parses scene files with the product's parser, runs arena_build and holds the record table to gatecert_make run on each node's
own triangles; the counts asserted here are the ones tests/test_gpu_camera_skip.py reads from the device."""
import os
import subprocess

import pytest

import scene_edits
import test_gpu_tight_gate_shapes as shapes
from test_gpu_segment_planes import room

ROOT = scene_edits.ROOT
CSRC = os.path.join(ROOT, "fray_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "camskip_check.cpp")
INC = "-I" + CSRC
MODES = 7


def _per_mode(out, title, n=MODES):
    words = out.split(title)[1].split("\n")[0].split()
    return [int(words[2 * k + 1].split("/")[0]) for k in range(n)]


def test_a_certified_ray_has_no_triangle_of_a_quad_accepted(tmp_path):
    """No certified ray has a triangle accepted, on the five walls (either diagonal) and on generated rectangles, parallelograms and other planar quads, for random
    rays, rays through edges and corners at offsets down to 1e-9 and to a rounding error, rays nearly parallel to the plane around the guard threshold, starts on
    the plane, exact zeros in the direction and the camera's rays; every wall gets a record; every kind of ray and of mesh is certified sometimes and the guard
    does send rays back.  Built without the margins and the guard the same harness finds contradictions, among the rays through edges and the starts on the
    plane."""
    exe = str(tmp_path / "camskip_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "6000000"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "contradictions 0" in r.stdout, r.stdout + r.stderr
    assert "refused wrongly 0" in r.stdout and r.stdout.count("direction(s)") == 10, r.stdout
    cases = int(r.stdout.split("cases")[1].split(",")[0])
    certified = int(r.stdout.split("certified")[1].split()[0])
    hit = int(r.stdout.split("hit")[1].split(",")[0])
    assert cases > 5000000 and certified > 0.2 * cases and hit > 0.1 * cases, r.stdout
    assert all(c > 0 for c in _per_mode(r.stdout, "certified per mode:")), r.stdout
    kinds = r.stdout.split("no parallelogram):")[1].split("\n")[0].split()
    assert len(kinds) == 4 and all(int(k.split("/")[0]) > 0 for k in kinds), r.stdout
    assert int(r.stdout.split("the guard sent back")[1].split(";")[0]) > 1000, r.stdout
    exe0 = str(tmp_path / "camskip_check0")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DFRAY_GATECERT_SCALE=0", "-DFRAY_MISSCERT_SCALE=0", INC, SRC, "-o", exe0], check=True)
    r0 = subprocess.run([exe0, "1000000"], capture_output=True, text=True, timeout=600)
    print(r0.stdout)
    words = r0.stdout.split("contradictions per mode:")[1].split("\n")[0].split()
    bad = [int(words[2 * k + 1]) for k in range(MODES)]
    assert r0.returncode == 1 and sum(bad) > 100 and bad[1] > 0 and bad[3] > 0, r0.stdout


def test_the_harness_is_clean_under_the_sanitizers(tmp_path):
    """the same program, stand-alone, built with AddressSanitizer and UndefinedBehaviorSanitizer, a shorter run"""
    exe = str(tmp_path / "camskip_check_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "300000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "contradictions 0" in r.stdout, r.stdout + r.stderr


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("camskip_table") / "camskip_table_check")
    src = [os.path.join(ROOT, "tests", "native", "camskip_table_check.cpp")] + [os.path.join(CSRC, f) for f in ("host_scene.cpp", "host_loaders.cpp", "host_exr.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + src + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + (r.stdout + r.stderr)[-6000:]
    return exe


def run(harness, args):
    """path -> (records, their nodes, their guards, their direction counts); the harness itself holds every record to gatecert_make's, entry for entry"""
    r = subprocess.run([harness] + list(args), capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    out, updated = {}, []
    for line in r.stdout.split("\n"):
        w = line.split()
        if w and w[0] == "camskip":
            kv = dict(x.split("=") for x in w[2:])
            lst = lambda v, f: [f(x) for x in v.split(",") if x]
            out[w[1]] = (int(kv["n"]), lst(kv["nodes"], int), lst(kv["guards"], float), lst(kv["dirs"], int))
        elif w and w[0] == "updated":
            updated.append((w[1], int(w[2].split("=")[1])))
    return out, updated


CORNELL = os.path.join(ROOT, "scenes", "cornell_box.fray")


def many_octahedra(n):
    """n small octahedra under the ceiling, each its own OBJ file and node"""
    return [("octa%02d" % i,) + shapes.octahedron((60.0 + 48.0 * (i % 10), 500.0 - 60.0 * (i // 10), 60.0 + 45.0 * (i % 10)), 15.0) for i in range(n)]


def test_the_records_are_gatecert_makes(harness, tmp_path):
    def d(name):
        p = tmp_path / name
        p.mkdir()
        return p
    strips = lambda one_more=False: ("strips",) + shapes.strip_box(shapes.BOX_C, shapes.BOX_HALF, one_more=one_more)
    # name -> (path, records, their nodes).  The room's nodes: floor 0, ceiling 1, back wall 2, right wall 3, left wall 4, short block 5, tall block 6, extras from 7
    rooms = {
        "cornell_box": (CORNELL, 7, list(range(7))),
        "the generated room": (room(d("plain")), 7, list(range(7))),
        "a block with a transform": (room(d("moved"), node_lines={"shortblock": ["translate (0, 0, 3)"]}), 6, [0, 1, 2, 3, 4, 6]),
        "a wall with a transform": (room(d("wall"), node_lines={"ceiling": ["translate (0, 2, 0)"]}), 6, [0, 2, 3, 4, 5, 6]),
        "a KD mesh": (room(d("kd"), extra=[strips()]), 7, list(range(7))),
        "the same mesh without its tree, 32 triangles": (shapes.without_kd(room(d("nokd"), extra=[strips()]), "strips"), 8, list(range(8))),
        "33 triangles": (shapes.without_kd(room(d("nokd33"), extra=[strips(True)]), "strips"), 7, list(range(7))),
        "a hexagonal pyramid, seven directions": (room(d("hexa"), extra=[("hexa",) + shapes.pyramid(6, (400.0, 380.0, 350.0), 50.0, 100.0)]), 7, list(range(7))),
        "a five-triangle fan": (room(d("fan"), extra=[("five",) + shapes.fan(380.0, 330.0, 250.0, 90.0, 5)]), 8, list(range(8))),
        # FRAY_CAMSKIP_MAX = 16: seven and nine more fill the table, the tenth gets none
        "sixteen eligible nodes": (room(d("sixteen"), extra=many_octahedra(9)), 16, list(range(16))),
        "a seventeenth eligible node": (room(d("seventeen"), extra=many_octahedra(10)), 16, list(range(16))),
        # nodes 7 .. 31 are transformed and get none; node 32 is eligible but a 32-bit word does not hold its index, node 31 beside it is held
        "an eligible node of index 32": (room(d("index32"), extra=many_octahedra(26), node_lines={"octa%02d" % i: ["translate (0, 1, 0)"] for i in range(25)}), 7, list(range(7))),
        "an eligible node of index 31": (room(d("index31"), extra=many_octahedra(25), node_lines={"octa%02d" % i: ["translate (0, 1, 0)"] for i in range(24)}), 8, list(range(7)) + [31]),
    }
    got, _ = run(harness, [v[0] for v in rooms.values()])
    for what, (path, n, nodes) in rooms.items():
        count, at, guards, dirs = got[path]
        assert (count, at) == (n, nodes), what
        # Gf = G + 2^-18, and eligibility caps it at 2^-6
        assert all(2.0 ** -18 <= g <= 2.0 ** -6 for g in guards) and all(1 <= k <= 6 for k in dirs), what
    # the walls' guards, about 4e-5; the left wall is not planar (two directions); the blocks have five
    _, _, guards, dirs = got[CORNELL]
    assert all(3e-5 < g < 5e-5 for g in guards[:5]) and dirs == [1, 1, 1, 1, 2, 5, 5], (guards, dirs)


@pytest.mark.parametrize("case", ["cornell-wall", "cornell-block"])
def test_an_updated_arena_has_the_fresh_ones_records(harness, tmp_path, case):
    """a node that an edit moves loses its record, one moved back regains it; byte for byte the arena arena_build makes of the edited file, and of the original"""
    c = scene_edits.CASES[case]
    original = scene_edits.scene_path(c, tmp_path)
    edited = str(tmp_path / (case + ".fray"))
    with open(edited, "w") as f:
        f.write(scene_edits.edited_text(c, original, tmp_path))
    got, updated = run(harness, ["--update", original, edited])
    moved = 3 if case == "cornell-wall" else 6
    assert got[original][:2] == (7, list(range(7)))
    assert got[edited][:2] == (6, [i for i in range(7) if i != moved])
    assert updated == [(edited, 6), (original, 7)]
