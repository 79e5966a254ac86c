"""The gate table on the CPU: what arena_build (fray_amd/csrc/scene_arena.hpp fill_editable) makes of the rooms that tests/test_gpu_tight_gate_shapes.py renders.

tests/native/gate_table_check.cpp parses each room with the product's parser, builds its arena and checks every tight entry against gatecert_make
(fray_amd/csrc/dev_gatecert.hpp) run on the mesh's own triangles: the record's bytes, and every triangle's direction among the entries.  The test holds the
figures that the GPU module asserts -- eligible gates, segment-plane nodes, certified_segments_eligible -- and the direction entries of each added mesh to the
arena's, so every count asserted on the GPU is one the host gives for the same file."""
import os
import subprocess

import pytest

import scene_edits
import test_gpu_tight_gate_shapes as shapes
from test_gpu_segment_planes import room

ROOT = scene_edits.ROOT
CSRC = os.path.join(ROOT, "fray_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gate_table") / "gate_table_check")
    src = [os.path.join(ROOT, "tests", "native", "gate_table_check.cpp")] + [os.path.join(CSRC, f) for f in ("host_scene.cpp", "host_loaders.cpp", "host_exr.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + src + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + (r.stdout + r.stderr)[-6000:]
    return exe


def run(harness, paths):
    """path -> (facts, direction entries per gate's tight entry, its guards, direction entries in the plain half, tight entries that are plain copies)"""
    r = subprocess.run([harness] + list(paths), capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.split("\n"):
        w = line.split()
        if w and w[0] == "facts":
            out[w[1]] = [{k: int(v) for k, v in (kv.split("=") for kv in w[2:])}]
        elif w and w[0] == "tight":
            gates = [x.split(":") for x in w[2:] if ":" in x]
            rest = dict(x.split("=") for x in w[2:] if "=" in x)
            out[w[1]] += [[int(g[0]) for g in gates], [float(g[1]) for g in gates], int(rest["plainDirs"]), int(rest["copies"])]
    return out


def generated_rooms(tmp_path):
    """name -> (path, eligible gates, segment-plane nodes, certified_segments_eligible, the direction entries of the added meshes' tight entries or None)"""
    def d(name):
        p = tmp_path / name
        p.mkdir()
        return p
    rooms = {}
    dirs = {"octa": 4, "penta": 6, "lprism": 3, "strips": 3}
    for i, (what, (make, tris, no_kd, plus, plane_nodes, certifiable)) in enumerate(shapes.SHAPES.items()):
        mesh = make()
        path = room(d("shape%d" % i), extra=[mesh])
        gated = tris >= 6 and (no_kd or tris <= 20)              # FRAY_GATE_MIN_TRIS; the loader gives a mesh of more than 20 triangles a KD-tree
        rooms[what] = (shapes.without_kd(path, mesh[0]) if no_kd else path, 2 + plus, 5 + plane_nodes, certifiable, ([dirs[mesh[0]] if plus else 0] if gated else []))
    for k, (eligible, certifiable) in shapes.SCALES.items():
        rooms["k=%g" % k] = (room(d("scale%g" % k), k=k), eligible, 5, certifiable, None)
    for reverse in (False, True):
        rooms["steep %d" % reverse] = (room(d("steep%d" % reverse), extra=[shapes.steep_pyramid(reverse)]), 3, 5, 1, [6])
    rooms["eight"] = (room(d("eight"), extra=shapes.small_octahedra(6)), 8, 5, 1, [4] * 6)
    rooms["nine"] = (room(d("nine"), extra=shapes.small_octahedra(7)), 8, 5, 0, [4] * 6)
    return rooms


def test_the_generated_rooms_figures_are_the_arenas(harness, tmp_path):
    rooms = generated_rooms(tmp_path)
    got = run(harness, [v[0] for v in rooms.values()])
    guards = {}
    for what, (path, eligible, plane_nodes, certifiable, dirs) in rooms.items():
        facts, entries, guard, plain, copies = got[path]
        assert facts["gatesExact"] == 1, what
        assert (facts["nTightGates"], facts["nSegNodes"], facts["segCertAll"]) == (eligible, plane_nodes, certifiable), what
        assert sum(1 for n in entries if n) == eligible and plain == 0 and copies == facts["nGates"] - eligible, what
        # Gf = G + 2^-18, and eligibility caps it at 2^-6: the bounds the grazing cameras' census rests on
        assert all(2.0 ** -18 <= g <= 2.0 ** -6 for g, n in zip(guard, entries) if n) and all(g == 0 for g, n in zip(guard, entries) if not n), what
        if dirs is not None:
            assert entries == [5, 5] + dirs, what                                  # the blocks, then the added meshes in node order
        guards[what] = guard
    assert guards["steep 0"] == guards["steep 1"] and 5e-3 < guards["steep 0"][2] < 2.0 ** -6       # the record that makes every entry decide


def test_moving_the_tall_block_takes_its_tight_record(harness, tmp_path):
    """cornell-block (tests/scene_edits.py) as two files: eligible 2, and 1 with the tall block moved -- the counts tests/test_gpu_tight_gate_shapes.py reads
    across Scene.update() (that arena_update leaves the fresh build's arena and facts, byte for byte, is tests/test_scene_update_host.py's)"""
    case = scene_edits.CASES["cornell-block"]
    original = scene_edits.scene_path(case, tmp_path)
    edited = str(tmp_path / "cornell-block.fray")
    with open(edited, "w") as f:
        f.write(scene_edits.edited_text(case, original, tmp_path))
    got = run(harness, [original, edited])
    assert (got[original][0]["nTightGates"], got[original][0]["segCertAll"], got[original][1]) == (2, 1, [5, 5])
    assert (got[edited][0]["nTightGates"], got[edited][0]["segCertAll"], got[edited][0]["gatesExact"], got[edited][1]) == (1, 0, 0, [5, 0])
