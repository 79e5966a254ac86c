"""Camera skip (frayhip_scene_camera_skip / Scene.camera_skip, on by default): a first-bounce wave of the path tracer -- one 8x8 pixel tile at one sample index --
leaves out every eligible mesh that all its camera rays provably miss (fray_amd/csrc/dev_trace.hpp camera_skip_nodes, the miss records of dev_scene.hpp DCamSkip,
the certificate of dev_gatecert.hpp; tests/test_camera_skip_host.py runs the certificate and the record table on the host).  A certified ray is one that no
triangle of the mesh accepts as the reference's arithmetic computes it, so the switch changes which nodes a wave asks and never a hit: no picture may change by a
single bit -- on against off, against the counting kernels (which ask every node) and against the oracle.  A wrong record crashes nothing: a wall loses pixels.

Frames are 64 x 64 (or smaller), 4 or 8 spp.  The record counts asserted are the host's for the same files (tests/test_camera_skip_host.py)."""
import os
import sys

import numpy as np
import pytest

import scene_edits
import test_gpu_tight_gate_shapes as shapes
from conftest import ROOT, open_scene, run_in_clean_child
from test_gpu_segment_planes import bits, room

pytestmark = pytest.mark.gpu

COUNTERS = ("closest_rays", "shadow_rays", "node_tests", "prim_tests", "samples")


def tiles(W, H):
    """first-bounce wave iterations with a ray in the frame, per sample: the 8x8 tiles of the 48x48 buckets that reach into the frame (kernels.hpp item_pixel)"""
    per_axis = lambda n: sum(-(-min(48, n - b) // 8) for b in range(0, n, 48))
    return per_axis(W) * per_axis(H)


def on_off_counted_oracle(s, abi, oracle, what):
    """Four frames equal by bits: the switch on, off, the counting kernels, the oracle; the counting kernels' rays, node and primitive tests and samples are the
    oracle's (they take no skip word).  Returns (records, skipped (wave, node) pairs with the switch on, first-bounce wave iterations)."""
    enabled, eligible, _, _ = s.camera_skip()
    assert enabled == 1                                                    # the default
    on, _ = s.render(seed=42)
    _, _, skipped, waves = s.camera_skip()
    counted, st = s.render(seed=42, stats=True)
    assert s.camera_skip()[2:] == (0, 0)                                   # the counting variants ask every node
    assert s.camera_skip(0)[:2] == (0, eligible)
    off, _ = s.render(seed=42)
    assert s.camera_skip() == (0, eligible, 0, 0)                          # switched off the kernel gets no record
    assert s.camera_skip(1)[:2] == (1, eligible)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    print("%s: %d records; %d (wave, node) pairs skipped in %d first-bounce wave iterations: %.3f of %d nodes per iteration"
          % (what, eligible, skipped, waves, skipped / max(waves, 1), s.desc.n_nodes))
    assert np.array_equal(bits(on), bits(off))
    assert np.array_equal(bits(on), bits(counted))
    assert np.array_equal(bits(on), bits(ref))
    assert float(np.asarray(on).max()) > 0                                 # a picture, not a black frame
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert 0 <= skipped <= eligible * waves
    return eligible, skipped, waves


def test_cornell_box_is_the_same_bits_and_skips_most_meshes(fray, abi, oracle, gpu):
    """cornell_box 64 x 64 x 8 spp: all seven meshes have a record; a float64 slab test of every tile's corner rays against the boxes of the meshes' own triangles
    gives 4.97 skipped of 7 per wave iteration at this frame size, and the certificate's margins cost a few 1e-3 units against tiles 50 units wide: at least 4.0."""
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, numPaths=8)
    s.beginRender()
    eligible, skipped, waves = on_off_counted_oracle(s, abi, oracle, "cornell_box 64 x 64 x 8 spp")
    assert eligible == 7
    assert waves == tiles(64, 64) * 8 == 512
    assert skipped / waves >= 4.0
    s.close()


def camera(path, pos, front=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=50.0):
    return shapes.with_camera(path, np.array(pos, float), np.array(front, float), np.array(up, float), fov)


def dof(s):
    s.camera.dof, s.camera.numDOFSamples, s.camera.fNumber, s.camera.focalPlaneDist = 1, 4, 2.0, 1000.0


# name -> (scene file, frame size, what to set on the parsed scene, the most that may be skipped per wave iteration or None).  The boxes are those of the
# meshes' own triangles: a wall's is flat, so a camera inside the room stands in no wall's box, and what it cannot skip is what its tiles look at.
LITTLE = {
    # the walls ahead are asked by the tiles that see them; what lies behind the start goes by the box part's first condition
    "the camera inside the room": (lambda p: camera(room(p, size=64), (278.0, 273.0, 100.0)), (64, 64), None, None),
    # the start inside a record's box: the box part fails for every ray, the tall block is asked by every wave
    "the camera inside the tall block's box": (lambda p: camera(room(p, size=64), (185.0, 200.0, 350.0), front=(0.3, 0.1, -1.0)), (64, 64), None, 6.0),
    # the middle rows run in the floor's plane, y = 0, on either side of it: the guard's rays, and starts on the plane
    "the camera in the floor's plane": (lambda p: camera(room(p, size=64), (278.0, 0.0, -800.0)), (64, 64), None, None),
    "the camera in the ceiling's plane": (lambda p: camera(room(p, size=64), (278.0, 548.8, -800.0)), (64, 64), None, None),
    # the central columns run parallel to the right wall, x = 556, within its guard of 4e-5 |d|_1 (a pixel is 1.5e-2 wide in d.x and every sample is jittered)
    "the central column along the right wall": (lambda p: camera(room(p, size=64), (556.0, 273.0, -800.0)), (64, 64), None, None),
    "the central column beside the right wall": (lambda p: camera(room(p, size=64), (555.999, 273.0, -300.0), fov=20.0), (64, 64), None, None),
    # per-lane origins on the lens
    "a DOF camera": (lambda p: room(p, size=64), (64, 64), dof, None),
    # 50 x 44: two buckets across, tiles cut at the frame's right and lower edge -- dead lanes vote -- and whole tiles outside it
    "a ragged edge bucket": (lambda p: room(p, size=64), (50, 44), None, None),
}


@pytest.mark.parametrize("what", list(LITTLE), ids=lambda v: v.replace(" ", "_").replace("'", ""))
def test_awkward_cameras_render_the_same_bits(fray, abi, oracle, gpu, tmp_path, what):
    make, (W, H), prepare, most = LITTLE[what]
    s = fray.Scene.parseScene(make(tmp_path))
    s.settings.frameWidth, s.settings.frameHeight = W, H
    if prepare:
        prepare(s)
    s.beginRender()
    eligible, skipped, waves = on_off_counted_oracle(s, abi, oracle, what)
    assert eligible == 7
    assert waves == tiles(W, H) * 4
    if most is not None:
        assert skipped <= most * waves
    s.close()


# ---- edits -------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_moved_wall_loses_its_record_and_regains_it(fray, abi, oracle, gpu, tmp_path):
    """cornell-wall (tests/scene_edits.py): the right wall is translated through Scene.update() and put back.  Moved, it has no record and the frame is the
    oracle's of the edited description; back, the record and the frame are the fresh handle's."""
    case = scene_edits.CASES["cornell-wall"]
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, wantAA=0, numPaths=4)
    s.beginRender()
    fresh = on_off_counted_oracle(s, abi, oracle, "cornell_box")
    first, _ = s.render(seed=42)
    assert fresh[0] == 7
    scene_edits.apply(fray, s, case["edit"])
    s.update()
    moved = on_off_counted_oracle(s, abi, oracle, "the right wall moved")
    assert moved[0] == 6 and moved[1] < fresh[1]                           # one record less, and no wave leaves the right wall out
    other, _ = s.render(seed=42)
    assert not np.array_equal(bits(other), bits(first))
    scene_edits.apply(fray, s, case["undo"])
    s.update()
    back = on_off_counted_oracle(s, abi, oracle, "the right wall back")
    assert back == fresh
    again, _ = s.render(seed=42)
    assert np.array_equal(bits(again), bits(first))
    # the switch survives an update as an option does
    assert s.camera_skip(0)[:2] == (0, 7)
    scene_edits.apply(fray, s, case["edit"])
    s.update()
    assert s.camera_skip()[:2] == (0, 6)
    s.close()


# ---- every way into render_impl that runs a first bounce ------------------------------------------------------------------------------------------------------
def progressive(s):
    seen = []
    rgb, st = s.render(seed=42, spp_chunk=2, progress=lambda info: seen.append(info["samples_done"]) and None, preview_ms=0)
    assert st["samples_done"] == 8 and not st["cancelled"] and len(seen) >= 2
    return {"rgb": rgb}


def contracted(s):
    s.set_option("fp_contract", 1)
    rgb, _ = s.render(seed=42)
    assert s.get_option("contracted_launches") > 0
    s.set_option("fp_contract", 0)
    return {"rgb": rgb}


ENTRIES = dict(shapes.ENTRIES)
ENTRIES["progressive"] = (48, 48, dict(numPaths=8), progressive)
ENTRIES["fp_contract"] = (48, 48, dict(numPaths=8), contracted)


@pytest.mark.parametrize("what", list(ENTRIES), ids=lambda v: v.replace(" ", "_"))
def test_entries_answer_the_same_bits_with_the_switch_off(fray, gpu, what):
    """resumable, component, adaptive and progressive frames, the contracted frame (its first bounce runs the exact kernel), one batch lane against four, one
    sample per batch, a bucket subset; and the stereo and long-generator frames, which start from k_pt_init and take no skip word: on = off by bits in all."""
    W, H, over, call = ENTRIES[what]
    s = open_scene(fray, "cornell_box.fray", W, H, gi=1, wantAA=0, **over)
    s.beginRender()
    assert s.camera_skip()[:2] == (1, 7)
    on = call(s)
    skipped = s.camera_skip()[2]
    assert s.camera_skip(0)[:2] == (0, 7)
    off = call(s)
    assert s.camera_skip()[2] == 0
    print("%s: %d pairs skipped in the last frame with the switch on" % (what, skipped))
    if what in ("stereo", "maxTraceDepth 20"):
        assert skipped == 0
    elif what != "render_adaptive":                                        # (an adaptive call's last frame is its last rung's)
        assert skipped > 0
    assert set(on) == set(off)
    for k in on:
        a, b = np.ascontiguousarray(on[k]), np.ascontiguousarray(off[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, k)
    assert any(np.asarray(v).dtype == np.float32 and float(np.abs(v).max()) > 0 for v in on.values())
    s.close()


CHILD = """import sys
import numpy as np
import fray_amd
s = fray_amd.Scene.parseScene(sys.argv[1])
s.settings.frameWidth, s.settings.frameHeight, s.settings.gi, s.settings.wantAA, s.settings.numPaths = 48, 48, 1, 0, 8
s.beginRender(0)
enabled, eligible, _, _ = s.camera_skip()
img, _ = s.render(seed=42)
np.save(sys.argv[2], img)
print("camera_skip %d %d %d" % (enabled, eligible, s.camera_skip()[2]))
s.close()
"""


def test_the_environment_presets_the_switch_off(fray, gpu, tmp_path):
    """FRAYHIP_CAMERA_SKIP=0 is read once, when a handle is created: in a fresh child, whose environment it is -- this process's is left alone"""
    scene = os.path.join(ROOT, "scenes", "cornell_box.fray")
    out = str(tmp_path / "child.npy")
    log = run_in_clean_child([sys.executable, "-c", CHILD, scene, out], str(tmp_path / "child.log"), timeout=300, env=dict(os.environ, FRAYHIP_CAMERA_SKIP="0"))
    assert "[exit code 0]" in log, log[-3000:]
    assert "camera_skip 0 7 0" in log, log[-3000:]
    assert "FRAYHIP_CAMERA_SKIP" not in os.environ
    s = open_scene(fray, "cornell_box.fray", 48, 48, gi=1, wantAA=0, numPaths=8)
    s.beginRender()
    assert s.camera_skip()[:2] == (1, 7)
    mine, _ = s.render(seed=42)
    assert s.camera_skip()[2] > 0
    child = np.load(out)
    assert child.dtype == np.float32 and np.array_equal(bits(child), bits(mine)) and float(mine.max()) > 0
    s.close()


def test_the_switch_is_refused_while_a_frame_renders(fray, abi, gpu):
    s = open_scene(fray, "cornell_box.fray", 48, 48, gi=1, wantAA=0, numPaths=4)
    s.beginRender()
    seen = []

    def cb(info):
        try:
            s.camera_skip(0)
        except fray.FrayError as e:
            seen.append((e.code, str(e)))
        seen.append(s.camera_skip()[:2])                                   # reading is allowed
        return None

    s.render(seed=42, spp_chunk=2, progress=cb, preview_ms=-1)
    assert seen and seen[0][0] == abi.E_ARG and "rendering" in seen[0][1] and seen[1] == (1, 7), seen
    assert fray.lib.frayhip_scene_camera_skip(s._dev, 2, None, None, None, None) == abi.E_ARG                 # enable is -1, 0 or 1
    assert fray.lib.frayhip_scene_camera_skip(None, -1, None, None, None, None) == abi.E_ARG
    assert s.camera_skip()[:2] == (1, 7)
    s.close()
