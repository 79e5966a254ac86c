"""Shade shortcuts (frayhip_scene_shade_shortcuts / Scene.shade_shortcuts, on by default): in a scene whose nodes are all untransformed flat meshes the path
tracer's timed kernels shade a hit without the node's transform and with a stored world normal; lights that are scaled along the axes and translated are
intersected and sampled by the three diagonal products, and a sample's cell is found by mask and shift when xSubd is a power of two (fray_amd/csrc/dev_shade.hpp
finalize_hit, light_nth_sample; dev_trace.hpp light_intersect, where the proofs stand; tests/test_shade_shortcuts_host.py runs both forms side by side on the
host).  Every value that leaves the changed functions is the same bit for bit, so no picture may change by a single bit -- on against off, against the counting
kernels (which take the general forms) and against the oracle.

Frames are 64 x 64 at 8 spp, one ragged frame is 50 x 44.  eligible: bit 0 the nodes, bit 1 the lights."""
import os
import sys

import numpy as np
import pytest

import scene_edits
import test_gpu_tight_gate_shapes as shapes
from conftest import ROOT, open_scene, run_in_clean_child
from test_gpu_contract import RMS_TOL
from test_gpu_segment_planes import bits, room

pytestmark = pytest.mark.gpu


def four_frames(s, abi, oracle, what, eligible, lit=True):
    """The frame with the switch on, with it off, the counting kernels' frame and the oracle's: equal by bits.  Returns the frame."""
    assert s.shade_shortcuts() == (1, eligible), what                      # on by default
    on, _ = s.render(seed=42)
    counted, _ = s.render(seed=42, stats=True)
    assert s.shade_shortcuts(0) == (0, eligible)
    off, _ = s.render(seed=42)
    assert s.shade_shortcuts(1) == (1, eligible)
    ref, _ = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    differ = lambda a, b: int((bits(a) != bits(b)).any(axis=-1).sum())
    print("%s: eligible %d; pixels that differ: on/off %d, on/counted %d, on/oracle %d" % (what, eligible, differ(on, off), differ(on, counted), differ(on, ref)))
    assert np.array_equal(bits(on), bits(off)), what
    assert np.array_equal(bits(on), bits(counted)), what
    assert np.array_equal(bits(on), bits(ref)), what
    if lit:
        assert float(np.asarray(on).max()) > 0, what                       # a picture, not a black frame
    return on


def test_cornell_box_is_the_same_bits(fray, abi, oracle, gpu):
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, numPaths=8)
    s.beginRender()
    four_frames(s, abi, oracle, "cornell_box 64 x 64 x 8 spp", 3)
    s.close()


def test_a_ragged_frame_is_the_same_bits(fray, abi, oracle, gpu):
    s = open_scene(fray, "cornell_box.fray", 50, 44, gi=1, numPaths=8)
    s.beginRender()
    four_frames(s, abi, oracle, "cornell_box 50 x 44 x 8 spp", 3)
    s.close()


# Views whose rays have exact zero components, where the sign of a zero could show: x = 0 is the left wall's plane and the camera's column; from inside the
# room the central row and column run along the axes.
VIEWS = {"the camera at (0, 273, -800)": (0.0, 273.0, -800.0), "the camera inside the room at (0, 100, 100)": (0.0, 100.0, 100.0)}


@pytest.mark.parametrize("what", list(VIEWS), ids=lambda v: v.replace(" ", "_").replace(",", ""))
def test_views_with_exact_zero_components_are_the_same_bits(fray, abi, oracle, gpu, tmp_path, what):
    path = shapes.with_camera(room(tmp_path, spp=8, size=64), np.array(VIEWS[what]), np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0]), 50.0)
    s = fray.Scene.parseScene(path)
    s.beginRender()
    four_frames(s, abi, oracle, what, 3)
    s.close()


LIGHT = "RectLight {\n\tscale (130, 1, 105)\n%s\ttranslate (278, 547.7, 279.5)\n\txSubd %d\n\tySubd %d\n\tcolor (1, 0.85, 0.43)\n\tpower 27.47\n}"
# name -> (the room, eligible, lit)
ROOMS = {
    "one wall translated": (lambda p: room(p, spp=8, size=64, node_lines={"backwall": ["translate (0, 0, 3)"]}), 2, True),
    "a rotated light": (lambda p: room(p, spp=8, size=64, light=LIGHT % ("\trotate (0, 20, 0)\n", 4, 4)), 1, True),
    # eligible, but xSubd is no power of two: the cell by the division
    "a light with xSubd 3 ySubd 5": (lambda p: room(p, spp=8, size=64, light=LIGHT % ("", 3, 5)), 3, True),
    # (the reference's path tracer gathers nothing from a point light: a black frame on every side)
    "a point light": (lambda p: room(p, spp=8, size=64, light="PointLight {\n\tpos (278, 500, 279.5)\n\tpower 130000\n\tcolor (1, 1, 1)\n}"), 1, False),
}


@pytest.mark.parametrize("what", list(ROOMS), ids=lambda v: v.replace(" ", "_"))
def test_generated_rooms_are_the_same_bits(fray, abi, oracle, gpu, tmp_path, what):
    make, eligible, lit = ROOMS[what]
    s = fray.Scene.parseScene(make(tmp_path))
    s.beginRender()
    four_frames(s, abi, oracle, what, eligible, lit)
    s.close()


def test_eligibility_follows_an_update(fray, abi, oracle, gpu):
    """cornell-wall (tests/scene_edits.py): the right wall is translated through Scene.update() and put back; bit 0 goes and returns, the frames are the oracle's
    of the edited description and the fresh handle's."""
    case = scene_edits.CASES["cornell-wall"]
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, wantAA=0, numPaths=8)
    s.beginRender()
    first = four_frames(s, abi, oracle, "cornell_box", 3)
    scene_edits.apply(fray, s, case["edit"])
    s.update()
    other = four_frames(s, abi, oracle, "the right wall moved", 2)
    assert not np.array_equal(bits(other), bits(first))
    scene_edits.apply(fray, s, case["undo"])
    s.update()
    again = four_frames(s, abi, oracle, "the right wall back", 3)
    assert np.array_equal(bits(again), bits(first))
    # the switch survives an update as an option does
    assert s.shade_shortcuts(0) == (0, 3)
    scene_edits.apply(fray, s, case["edit"])
    s.update()
    assert s.shade_shortcuts() == (0, 2)
    s.close()


def test_the_contracted_frame_stays_within_its_bound(fray, abi, oracle, gpu):
    """option "fp_contract" with the switch on: the contracted kernels take the table's normal, which is more exact than their own -- within the bound
    tests/test_gpu_contract.py holds contracted frames to, RMS_TOL per channel against the oracle."""
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, numPaths=8)
    s.beginRender()
    assert s.shade_shortcuts() == (1, 3)
    s.set_option("fp_contract", 1)
    img, _ = s.render(seed=42)
    assert s.get_option("contracted_launches") > 0
    ref, _ = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    r = np.sqrt(((img.astype(np.float64) - ref) ** 2).mean(axis=(0, 1)))
    print("contracted, switch on: rms per channel %s" % r)
    assert np.all(np.isfinite(img)) and np.all(r <= RMS_TOL), r
    s.close()


# ---- every way into render_impl -----------------------------------------------------------------------------------------------------------------------------
def progressive(s):
    seen = []
    rgb, st = s.render(seed=42, spp_chunk=2, progress=lambda info: seen.append(info["samples_done"]) and None, preview_ms=0)
    assert st["samples_done"] == 8 and not st["cancelled"] and len(seen) >= 2
    return {"rgb": rgb}


def samples_map(s):
    H, W = s.settings.frameHeight, s.settings.frameWidth
    add = (1 + (np.arange(H)[:, None] + np.arange(W)[None, :]) % 5).astype(np.int32)
    rgb, _ = s.render_samples_map(add)
    return {"rgb": rgb}


ENTRIES = {k: shapes.ENTRIES[k] for k in ("render_samples 3 + 5", "render_components", "render_adaptive")}
ENTRIES["progressive"] = (48, 48, dict(numPaths=8), progressive)
ENTRIES["render_samples_map"] = (48, 48, dict(numPaths=8), samples_map)


@pytest.mark.parametrize("what", list(ENTRIES), ids=lambda v: v.replace(" ", "_"))
def test_entries_answer_the_same_bits_with_the_switch_off(fray, gpu, what):
    W, H, over, call = ENTRIES[what]
    s = open_scene(fray, "cornell_box.fray", W, H, gi=1, wantAA=0, **over)
    s.beginRender()
    assert s.shade_shortcuts() == (1, 3)
    on = call(s)
    assert s.shade_shortcuts(0) == (0, 3)
    off = call(s)
    assert set(on) == set(off)
    for k in on:
        a, b = np.ascontiguousarray(on[k]), np.ascontiguousarray(off[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)
    assert any(np.asarray(v).dtype == np.float32 and float(np.abs(v).max()) > 0 for v in on.values())          # a picture, not a black frame
    s.close()


CHILD = """import sys
import fray_amd
s = fray_amd.Scene.parseScene(sys.argv[1])
s.settings.frameWidth, s.settings.frameHeight = 48, 48
s.beginRender(0)
print("shade_shortcuts %d %d" % s.shade_shortcuts())
s.close()
"""


def test_the_environment_presets_the_switch_off(fray, gpu, tmp_path):
    """FRAYHIP_SHADE_SHORTCUTS=0 is read once, when a handle is created: in a fresh child, whose environment it is -- this process's is left alone"""
    scene = os.path.join(ROOT, "scenes", "cornell_box.fray")
    log = run_in_clean_child([sys.executable, "-c", CHILD, scene], str(tmp_path / "child.log"), timeout=300, env=dict(os.environ, FRAYHIP_SHADE_SHORTCUTS="0"))
    assert "[exit code 0]" in log, log[-3000:]
    assert "shade_shortcuts 0 3" in log, log[-3000:]
    assert "FRAYHIP_SHADE_SHORTCUTS" not in os.environ


def test_the_switch_is_refused_while_a_frame_renders(fray, abi, gpu):
    s = open_scene(fray, "cornell_box.fray", 48, 48, gi=1, wantAA=0, numPaths=4)
    s.beginRender()
    seen = []

    def cb(info):
        try:
            s.shade_shortcuts(0)
        except fray.FrayError as e:
            seen.append((e.code, str(e)))
        seen.append(s.shade_shortcuts())                                   # reading is allowed
        return None

    s.render(seed=42, spp_chunk=2, progress=cb, preview_ms=-1)
    assert seen and seen[0][0] == abi.E_ARG and "rendering" in seen[0][1] and seen[1] == (1, 3), seen
    assert fray.lib.frayhip_scene_shade_shortcuts(s._dev, 2, None, None) == abi.E_ARG                 # enable is -1, 0 or 1
    assert fray.lib.frayhip_scene_shade_shortcuts(None, -1, None, None) == abi.E_ARG
    assert s.shade_shortcuts() == (1, 3)
    s.close()
