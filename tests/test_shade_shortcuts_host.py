"""The shade shortcuts on the CPU (frayhip_scene_shade_shortcuts; fray_amd/csrc/dev_shade.hpp finalize_hit, light_nth_sample; dev_trace.hpp light_intersect;
scene_arena.hpp fill_editable).

tests/native/shade_shortcut_check.cpp includes the device headers as plain C++ (one lane of a wave, -ffp-contract=off), parses cornell_box.fray with the product's
parser, builds its arena and runs the general and the shortcut form of the three functions side by side, every output compared by bit pattern: random rays, operands
that are +0, -0, subnormal and 2^+-500, hits exactly on x = 0, shade points in the light's plane; then the eligibility of edited lights, the world-normal table
against the general form's normals, and the flags and the table across arena_update.  It is stand-alone and runs under AddressSanitizer and
UndefinedBehaviorSanitizer.  Built without the final + (+0.0), or with the rule against zero offset components switched off, the same program reports contradictions."""
import os
import subprocess

import pytest

import scene_edits

ROOT = scene_edits.ROOT
CSRC = os.path.join(ROOT, "fray_amd", "csrc")
CORNELL = os.path.join(ROOT, "scenes", "cornell_box.fray")
SRC = [os.path.join(ROOT, "tests", "native", "shade_shortcut_check.cpp")] + [os.path.join(CSRC, f) for f in ("host_scene.cpp", "host_loaders.cpp", "host_exr.cpp")]
INC = ["-I" + os.path.join(ROOT, "tests", "native", "hostlane"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def build(tmp, name, flags):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-ffp-contract=off"] + flags + INC + SRC + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + (r.stdout + r.stderr)[-6000:]
    return exe


def per_mode(out, title):
    return [int(w) for w in out.split(title)[1].split("\n")[0].split()]


def run(exe, args, timeout=600):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:])
    return r


def test_both_forms_give_the_same_bits(tmp_path):
    """3 000 000 random rays from inside the room and 4 500 000 adversarial cases: no output differs; every mode runs, mesh and light hits and shade points in the
    light's plane occur; the only cases set aside are those outside the proofs' precondition (a non-finite direction or hit point, made of 2^-500 and subnormal
    directions), all in the adversarial mode."""
    exe = build(tmp_path, "shade_shortcut_check", ["-O2"])
    r = run(exe, [CORNELL, "3000000"])
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "flags: shadeIdentity 1 lightsDiagonal 1 normStride 32 nodes 7 lights 1 xShift 2" in r.stdout
    assert "table: 30 entries equal" in r.stdout
    cases, outside, bad = (per_mode(r.stdout, t) for t in ("cases per mode:", "outside the precondition per mode:", "contradictions per mode:"))
    assert bad == [0, 0, 0] and all(c > 1000000 for c in cases), r.stdout
    assert outside[0] == 0 and outside[2] == 0 and outside[1] < 0.01 * cases[1], r.stdout
    tail = r.stdout.split("mesh hits")[1]
    mesh, light = int(tail.split(",")[0]), int(tail.split("light hits")[1].split(";")[0])
    plane = int(tail.split("light's plane")[1].split(",")[0])
    assert mesh > 1000000 and light > 100000 and plane > 100000, r.stdout


def test_the_harness_is_clean_under_the_sanitizers(tmp_path):
    """the same program, stand-alone, built with AddressSanitizer and UndefinedBehaviorSanitizer, a shorter run; and the flags and the table across arena_update:
    cornell-wall (tests/scene_edits.py) moves the right wall -- bit 0 goes, the lights' bit stays -- and back: the arenas equal the fresh ones byte for byte"""
    exe = build(tmp_path, "shade_shortcut_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    case = scene_edits.CASES["cornell-wall"]
    original = scene_edits.scene_path(case, tmp_path)
    edited = str(tmp_path / "cornell-wall.fray")
    with open(edited, "w") as f:
        f.write(scene_edits.edited_text(case, original, tmp_path))
    r = run(exe, [CORNELL, "200000", "--update", original, edited])
    assert r.returncode == 0 and "FAIL" not in r.stdout and "contradictions 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "updated: shadeIdentity 1 -> 0, lightsDiagonal 1 -> 1" in r.stdout and "updated back: shadeIdentity 1, lightsDiagonal 1" in r.stdout, r.stdout


@pytest.mark.parametrize("flag,mode", [("-DFRAY_SHADE_PLUS_ZERO=0", 1), ("-DFRAY_LIGHT_ZERO_OFFSET_OK=1", 2)])
def test_the_harness_can_fail(tmp_path, flag, mode):
    """Without finalize_hit's final + (+0.0) the adversarial mode finds hit points whose zero has the wrong sign (51 438 of 3 003 000 at N = 2 000 000); with the rule
    against zero offset components switched off, a mirrored light with a -0 offset component passes as eligible and its samples differ (334 261 of 7 515 000)."""
    exe = build(tmp_path, "shade_shortcut_check_bad", ["-O2", flag])
    r = run(exe, [CORNELL, "500000"])
    bad = per_mode(r.stdout, "contradictions per mode:")
    assert r.returncode == 1 and bad[mode] > 1000 and sum(bad) == bad[mode], r.stdout
