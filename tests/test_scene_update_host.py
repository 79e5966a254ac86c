"""frayhip_scene_update on the CPU: arena_update (fray_amd/csrc/scene_arena.hpp) must leave the arena, byte for byte, that arena_build makes of the
edited description, and the C helpers (frayhip_transform_*, frayhip_light_begin_frame, frayhip_shader_begin_frame) must be the parser's arithmetic.

tests/native/arena_update_check.cpp does the work, built with AddressSanitizer + UndefinedBehaviorSanitizer (as arena_dump is): it parses the
original scene, builds its arena (twice: two fresh builds are byte-identical, no table needs a field-by-field comparison), edits the description
through the helpers, frees the mesh arrays and the texel pool the description points to, runs arena_update, parses the edited scene written out as
text and compares -- description tables, table list, every table's bytes, ArenaFacts.  Each case asserts the facts before and after, so that it
provably flips what it is there to flip."""
import ctypes as C
import os
import subprocess

import pytest

import scene_edits
from scene_edits import CASES

ROOT = scene_edits.ROOT
CSRC = os.path.join(ROOT, "fray_amd", "csrc")
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("arena_update") / "arena_update_check")
    src = [os.path.join(ROOT, "tests", "native", "arena_update_check.cpp")] + [os.path.join(CSRC, f) for f in ("host_scene.cpp", "host_loaders.cpp", "host_exr.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + src + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + (r.stdout + r.stderr)[-6000:]
    return exe


def run(harness, original, edited, tokens):
    r = subprocess.run([harness, original, edited] + list(tokens), capture_output=True, text=True, timeout=300, env=dict(os.environ, **SAN_ENV))
    print(r.stdout[-4000:])
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.split("\n"):
        tag = line.split(" ", 1)[0]
        if tag in ("before", "after", "fresh", "undone"):
            out[tag] = {k: (int(v) if not k.startswith("h_") else v) for k, v in (kv.split("=") for kv in line.split()[1:])}
        elif tag.endswith("_light0"):
            out[tag] = dict(kv.split("=") for kv in line.split()[1:])
    out["text"] = r.stdout
    return out


def run_case(harness, tmp_path, name):
    case = CASES[name]
    original = scene_edits.scene_path(case, tmp_path)
    edited = str(tmp_path / (name + ".fray"))
    with open(edited, "w") as f:
        f.write(scene_edits.edited_text(case, original, tmp_path))
    tokens = list(case["edit"]) + (["--undo"] + list(case["undo"]) if case["undo"] else [])
    r = run(harness, original, edited, tokens)
    for line in ("fresh_builds identical", "desc_vs_parser identical", "update_vs_fresh identical"):
        assert line in r["text"], line
    assert r["after"] == r["fresh"]
    if case["undo"]:
        assert "undo_vs_original identical" in r["text"] and r["undone"] == r["before"]
    return r


def changed(r, *tables):
    return all(r["before"]["h_" + t] != r["after"]["h_" + t] for t in tables)


def unchanged(r, *tables):
    return all(r["before"]["h_" + t] == r["after"]["h_" + t] for t in tables)


def test_moving_the_tall_block_withdraws_every_gate_certificate(harness, tmp_path):
    r = run_case(harness, tmp_path, "cornell-block")
    b, a = r["before"], r["after"]
    assert (b["nGates"], b["gatesExact"], b["gatedNodes"]) == (2, 1, 2)             # the two blocks: ten or more triangles, untransformed, no KD-tree
    assert (a["nGates"], a["gatesExact"], a["gatedNodes"]) == (2, 0, 0)             # one gate inexact: no node may be skipped on a gate's word
    assert b["identityNodes"] == 7 and a["identityNodes"] == 6
    assert changed(r, "nodes", "gates") and unchanged(r, "segPlanes", "segMasks", "lights", "shaders")


def test_moving_a_wall_takes_its_planes_out_of_the_segment_tables(harness, tmp_path):
    r = run_case(harness, tmp_path, "cornell-wall")
    b, a = r["before"], r["after"]
    assert b["nSegNodes"] == 5 and b["segNodeFlags"] == 5                            # floor, ceiling and three walls
    assert a["nSegNodes"] == 4 and a["segNodeFlags"] == 4 and a["nSegPlanes"] < b["nSegPlanes"]
    assert changed(r, "nodes", "segPlanes", "segMasks") and (a["nGates"], a["gatesExact"]) == (2, 1)


def test_switching_the_mirror_to_white_ends_the_recursion(harness, tmp_path):
    r = run_case(harness, tmp_path, "cornell-shader")
    assert r["before"]["whittedNeedsRecursion"] == 1 and r["after"]["whittedNeedsRecursion"] == 0
    assert changed(r, "nodes") and unchanged(r, "shaders", "gates", "segPlanes")


def test_changing_the_light_changes_its_sample_count_centre_and_area(harness, tmp_path):
    r = run_case(harness, tmp_path, "cornell-light")
    assert r["before"]["lightSampleCount"] == 16 and r["after"]["lightSampleCount"] == 4
    lb, la = r["before_light0"], r["after_light0"]
    assert (lb["xSubd"], lb["ySubd"], la["xSubd"], la["ySubd"]) == ("4", "4", "2", "2")
    assert lb["center"] == "278,547.70000000000005,279.5" and la["center"] == "250,540,279.5"
    assert float(lb["area"]) == 130.0 * 105.0 and float(la["area"]) == 100.0 * 120.0
    assert changed(r, "lights") and unchanged(r, "nodes", "gates")


def test_moving_a_csg_node_and_resizing_its_operands(harness, tmp_path):
    r = run_case(harness, tmp_path, "csg-nested")
    assert r["before"]["extGeometry"] == 1 and r["after"]["extGeometry"] == 1 and r["before"]["nGates"] > 0
    assert changed(r, "nodes", "nodesX", "gates", "spheres", "cubes")                # the DNodeX box of (box & ball) - small, and the gates made from it


def test_texture_parameters_a_bump_reference_and_a_kd_mesh_node(harness, tmp_path):
    r = run_case(harness, tmp_path, "boxed-textured")
    assert changed(r, "textures", "nodes") and unchanged(r, "shaders", "lights", "planes")


def test_a_short_fan_is_not_drawn_ahead(harness, tmp_path):
    r = run_case(harness, tmp_path, "glossy-fan")
    assert (r["before"]["specFanMax"], r["before"]["lightDraws"]) == (16, 0)
    assert (r["after"]["specFanMax"], r["after"]["lightDraws"]) == (0, 0)
    assert changed(r, "shaders")                                                     # numSamples, glossiness and the deflectionScaling made from it


def test_a_rect_light_in_place_of_a_point_light_draws(harness, tmp_path):
    r = run_case(harness, tmp_path, "glossy-rect")
    assert (r["before"]["lightDraws"], r["before"]["lightSampleCount"], r["before"]["specFanMax"]) == (0, 2, 16)
    assert (r["after"]["lightDraws"], r["after"]["lightSampleCount"], r["after"]["specFanMax"]) == (1, 5, 0)
    assert changed(r, "lights")


@pytest.mark.parametrize("name", ["cornell-block", "csg-nested", "boxed-textured", "glossy-fan"])          # one case per scene file
def test_helpers_rebuild_the_parsers_bytes_from_the_files_numbers(harness, tmp_path, name):
    """Every node's and every light's T rebuilt from the identity with the file's own scale / rotate / translate lines, every light's center and
    area and every shader's deflectionScaling re-derived: the description must stay the parser's, byte for byte (and so must the arena)."""
    original = scene_edits.scene_path(CASES[name], tmp_path)
    with open(original) as f:
        tokens = scene_edits.file_transforms(f.read())
    assert tokens.count("reset") >= 2
    r = run(harness, original, original, tokens)
    assert "desc_vs_parser identical" in r["text"] and "update_vs_fresh identical" in r["text"] and r["after"] == r["before"]


def test_the_abi_has_the_entry_points(fray, abi):
    for name in ("frayhip_scene_update", "frayhip_transform_identity", "frayhip_transform_scale", "frayhip_transform_rotate", "frayhip_transform_translate",
                 "frayhip_light_begin_frame", "frayhip_shader_begin_frame"):
        assert hasattr(fray.lib, name) and name in abi.SYMBOLS, name
    desc = abi.SceneDesc(abi_version=abi.ABI_VERSION)
    assert fray.lib.frayhip_scene_update(None, C.byref(desc)) == abi.E_ARG and b"frayhip_scene_update" in fray.lib.frayhip_last_error()
    assert fray.lib.frayhip_transform_scale(None, 1.0, 1.0, 1.0) == abi.E_ARG
    assert fray.lib.frayhip_abi_version() == 3                                       # additions only


def test_transform_wrapper_is_the_parsers_transform(fray, abi):
    """fray_amd.Transform over the helpers against the parser, without a device: boxed.fray's teapot node is translate, rotate, scale in the file."""
    s = fray.Scene.parseScene(os.path.join(scene_edits.SCENES, "boxed.fray"))
    T = fray.Transform().translate(0, 16, 0).rotate(120.3, 0, 0).scale(7.5, 7.5, 7.5)
    assert bytes(T.T) == bytes(s.nodes[7].T) and len(s.nodes) == s.desc.n_nodes == 9
    keep = bytes(s.lights[0])
    s.lights[0].area, s.lights[0].center[1] = -1.0, 99.0
    fray.light_begin_frame(s.lights[0])
    assert bytes(s.lights[0]) == keep
    s.nodes[7].shader = 0                                                            # the views are the description's own arrays
    assert s.desc.nodes[7].shader == 0
    s.close()
