"""Camera tiles (frayhip_scene_camera_tiles / Scene.camera_tiles, on by default): the first bounce of the path tracer's leanest timed kernel reads what is a property of
its wave's 8x8 pixel tile -- the pixel origin, the meshes no camera ray of the tile can hit -- from a table made once per frame (fray_amd/csrc/dev_camtile.hpp,
kernels.hpp k_cam_tiles), not per lane and per sample; tests/test_camera_tiles_host.py runs the certificate and the origin on the host.  The skipped meshes are ones
no ray of the tile hits as the reference's arithmetic computes it, and the origin is item_pixel's: no picture may change by a single bit -- tiles on against tiles off
(the per-wave test of camera skip), against camera skip off, against the counting kernels (which ask every node) and against the oracle.

Frames are 64 x 64 or smaller (one is 200 x 120 in two shares of a third), 2 to 8 spp."""
import os
import sys

import numpy as np
import pytest

import scene_edits
import test_gpu_camera_skip as skip
from conftest import ROOT, open_scene, run_in_clean_child
from test_gpu_segment_planes import bits, room

pytestmark = pytest.mark.gpu

COUNTERS = ("closest_rays", "shadow_rays", "node_tests", "prim_tests", "samples")


def five_ways(s, abi, oracle, what, **share):
    """Five frames equal by bits: tiles on, tiles off (the per-wave test), camera skip off, the counting kernels, the oracle.  `waves` is the same with tiles on and
    off.  Returns (records, (skipped, waves) with tiles on, (skipped, waves) with tiles off)."""
    assert s.camera_tiles() == 1 and s.camera_skip()[0] == 1               # the defaults
    eligible = s.camera_skip()[1]
    on, _ = s.render(seed=42, **share)
    with_tiles = s.camera_skip()[2:]
    assert s.camera_tiles(0) == 0
    off, _ = s.render(seed=42, **share)
    per_wave = s.camera_skip()[2:]
    assert s.camera_tiles(1) == 1
    assert s.camera_skip(0)[:2] == (0, eligible)
    noskip, _ = s.render(seed=42, **share)                                 # zero skip words; the table still gives the pixel origin
    assert s.camera_skip()[2:] == (0, 0)
    assert s.camera_skip(1)[:2] == (1, eligible)
    counted, st = s.render(seed=42, stats=True, **share)
    assert s.camera_skip()[2:] == (0, 0)                                   # the counting variants ask every node
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42, **share)
    print("%s: %d records; tiles on: %d pairs in %d wave iterations, %.3f per iteration; tiles off (per wave): %d in %d, %.3f"
          % (what, eligible, with_tiles[0], with_tiles[1], with_tiles[0] / max(with_tiles[1], 1), per_wave[0], per_wave[1], per_wave[0] / max(per_wave[1], 1)))
    for name, img in (("tiles off", off), ("camera skip off", noskip), ("the counting kernels", counted), ("the oracle", ref)):
        assert np.array_equal(bits(on), bits(img)), (what, name)
    assert float(np.asarray(on).max()) > 0                                 # a picture, not a black frame
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert with_tiles[1] == per_wave[1]
    assert 0 <= with_tiles[0] <= eligible * with_tiles[1] and 0 <= per_wave[0] <= eligible * per_wave[1]
    return eligible, with_tiles, per_wave


def test_cornell_box_is_the_same_bits_five_ways(fray, abi, oracle, gpu):
    """cornell_box 64 x 64 x 8 spp: 512 first-bounce wave iterations; the per-wave test skips 4.90 of 7 nodes per iteration, and a tile's word holds the nodes that
    stay skipped over the tile's whole rectangle: something, and no more than a table of seven bits can hold"""
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, numPaths=8)
    s.beginRender()
    eligible, (skipped, waves), (skipped_w, _) = five_ways(s, abi, oracle, "cornell_box 64 x 64 x 8 spp")
    assert eligible == 7 and waves == skip.tiles(64, 64) * 8 == 512
    assert skipped > 0 and skipped_w > 0
    s.close()


def test_ragged_tiles_are_the_same_bits(fray, abi, oracle, gpu, tmp_path):
    """50 x 44: two buckets across, tiles cut at the frame's right and lower edge and whole tiles outside it"""
    s = fray.Scene.parseScene(room(tmp_path, size=64))
    s.settings.frameWidth, s.settings.frameHeight = 50, 44
    s.beginRender()
    eligible, (skipped, waves), _ = five_ways(s, abi, oracle, "50 x 44 x 4 spp")
    assert eligible == 7 and waves == skip.tiles(50, 44) * 4 and skipped > 0
    s.close()


@pytest.mark.parametrize("first", [1, 2])
def test_a_share_of_the_buckets_is_the_same_bits(fray, abi, oracle, gpu, first):
    """200 x 120 x 2 spp, 15 buckets, rendered as the shares (1, 3) and (2, 3): the table's entries are the share's tiles in item order"""
    s = open_scene(fray, "cornell_box.fray", 200, 120, gi=1, wantAA=0, numPaths=2)
    s.beginRender()
    eligible, (skipped, waves), _ = five_ways(s, abi, oracle, "200 x 120 x 2 spp, share (%d, 3)" % first, bucket_first=first, bucket_stride=3)
    assert eligible == 7 and waves > 0 and skipped > 0
    s.close()


CAMERAS = {
    "the camera inside the room": (lambda p: skip.camera(room(p, size=64), (278.0, 273.0, 100.0)), None),
    # the start inside a record's box: the box part fails for every tile, the tall block is asked by every wave
    "the camera inside the tall block's box": (lambda p: skip.camera(room(p, size=64), (185.0, 200.0, 350.0), front=(0.3, 0.1, -1.0)), 6.0),
    # the middle rows run in the floor's plane: tiles whose corner directions disagree about the side of the plane, and starts on it
    "the camera in the floor's plane": (lambda p: skip.camera(room(p, size=64), (278.0, 0.0, -800.0)), None),
    # the central columns run along the right wall, x = 556, within its guard
    "the central column along the right wall": (lambda p: skip.camera(room(p, size=64), (556.0, 273.0, -800.0)), None),
}


@pytest.mark.parametrize("what", list(CAMERAS), ids=lambda v: v.replace(" ", "_").replace("'", ""))
def test_awkward_cameras_render_the_same_bits(fray, abi, oracle, gpu, tmp_path, what):
    make, most = CAMERAS[what]
    s = fray.Scene.parseScene(make(tmp_path))
    s.settings.frameWidth, s.settings.frameHeight = 64, 64
    s.beginRender()
    eligible, (skipped, waves), _ = five_ways(s, abi, oracle, what)
    assert eligible == 7 and waves == skip.tiles(64, 64) * 4
    if most is not None:
        assert skipped <= most * waves
    s.close()


def test_a_dof_camera_takes_the_word_from_its_own_rays(fray, abi, oracle, gpu, tmp_path):
    """per-lane starts on the lens: the table's words are zero and the wave evaluates the records on its rays, with tiles on as with tiles off"""
    s = fray.Scene.parseScene(room(tmp_path, size=64))
    s.settings.frameWidth, s.settings.frameHeight = 64, 64
    skip.dof(s)
    s.beginRender()
    eligible, with_tiles, per_wave = five_ways(s, abi, oracle, "a DOF camera")
    assert eligible == 7 and with_tiles[0] > 0
    assert with_tiles == per_wave                                          # the same word from the same rays
    s.close()


def turn(s, degrees):
    s.camera.yaw += degrees


def test_one_handle_across_changes_renders_what_a_fresh_one_does(fray, gpu, tmp_path):
    """A frame, the camera turned by 30 degrees, the frame size changed, a wall moved through Scene.update(): the table is made anew by every frame, so each frame
    equals a fresh handle's of the same view and description."""
    case = scene_edits.CASES["cornell-wall"]

    def fresh(W, H, yaw, moved):
        f = open_scene(fray, "cornell_box.fray", W, H, gi=1, wantAA=0, numPaths=4)
        f.camera.yaw += yaw
        if moved:
            scene_edits.apply(fray, f, case["edit"])
        f.beginRender()
        img, _ = f.render(seed=42)
        pairs = f.camera_skip()[2]
        f.close()
        return img, pairs

    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, wantAA=0, numPaths=4)
    s.beginRender()
    seen = []
    for what, change, args in (("the first frame", None, (64, 64, 0.0, False)),
                               ("the camera turned by 30 degrees", lambda: (turn(s, 30.0), s.beginFrame()), (64, 64, 30.0, False)),
                               ("the frame size changed", lambda: (setattr(s.settings, "frameWidth", 56), setattr(s.settings, "frameHeight", 40), s.beginFrame()), (56, 40, 30.0, False)),
                               ("a wall moved", lambda: (scene_edits.apply(fray, s, case["edit"]), s.update()), (56, 40, 30.0, True))):
        if change:
            change()
        img, _ = s.render(seed=42)
        pairs = s.camera_skip()[2]
        want, want_pairs = fresh(*args)
        print("%s: %d pairs skipped (a fresh handle: %d)" % (what, pairs, want_pairs))
        assert img.shape == want.shape and np.array_equal(bits(img), bits(want)), what
        assert pairs == want_pairs and float(img.max()) > 0, what
        seen.append(bits(img).tobytes())
    assert len(set(seen)) == len(seen)                                     # four different pictures
    s.close()


@pytest.mark.parametrize("what", list(skip.ENTRIES), ids=lambda v: v.replace(" ", "_"))
def test_entries_answer_the_same_bits_with_the_switch_off(fray, gpu, what):
    """every way into render_impl that tests/test_gpu_camera_skip.py lists: tiles on = tiles off by bits"""
    W, H, over, call = skip.ENTRIES[what]
    s = open_scene(fray, "cornell_box.fray", W, H, gi=1, wantAA=0, **over)
    s.beginRender()
    assert s.camera_tiles() == 1
    on = call(s)
    skipped = s.camera_skip()[2]
    assert s.camera_tiles(0) == 0
    off = call(s)
    skipped_off = s.camera_skip()[2]
    print("%s: %d pairs skipped in the last frame with tiles on, %d with tiles off" % (what, skipped, skipped_off))
    if what in ("stereo", "maxTraceDepth 20"):
        assert skipped == 0 and skipped_off == 0
    elif what != "render_adaptive":                                        # (an adaptive call's last frame is its last rung's)
        assert skipped > 0 and skipped_off > 0
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
enabled = s.camera_tiles()
img, _ = s.render(seed=42)
np.save(sys.argv[2], img)
print("camera_tiles %d %d" % (enabled, s.camera_skip()[2]))
s.close()
"""


def test_the_environment_presets_the_switch_off(fray, gpu, tmp_path):
    """FRAYHIP_CAMERA_TILES=0 is read once, when a handle is created: in a fresh child, whose environment it is -- this process's is left alone"""
    scene = os.path.join(ROOT, "scenes", "cornell_box.fray")
    out = str(tmp_path / "child.npy")
    log = run_in_clean_child([sys.executable, "-c", CHILD, scene, out], str(tmp_path / "child.log"), timeout=300, env=dict(os.environ, FRAYHIP_CAMERA_TILES="0"))
    assert "[exit code 0]" in log, log[-3000:]
    assert "camera_tiles 0 " in log, log[-3000:]
    child_pairs = int(log.split("camera_tiles 0 ")[1].split()[0])
    assert "FRAYHIP_CAMERA_TILES" not in os.environ
    s = open_scene(fray, "cornell_box.fray", 48, 48, gi=1, wantAA=0, numPaths=8)
    s.beginRender()
    assert s.camera_tiles() == 1
    mine, _ = s.render(seed=42)
    assert s.camera_skip()[2] > 0
    s.camera_tiles(0)
    s.render(seed=42)
    assert s.camera_skip()[2] == child_pairs > 0                           # the child ran the per-wave test
    child = np.load(out)
    assert child.dtype == np.float32 and np.array_equal(bits(child), bits(mine)) and float(mine.max()) > 0
    s.close()


def test_the_switch_is_refused_while_a_frame_renders(fray, abi, gpu):
    s = open_scene(fray, "cornell_box.fray", 48, 48, gi=1, wantAA=0, numPaths=4)
    s.beginRender()
    seen = []

    def cb(info):
        try:
            s.camera_tiles(0)
        except fray.FrayError as e:
            seen.append((e.code, str(e)))
        seen.append(s.camera_tiles())                                      # reading is allowed
        return None

    s.render(seed=42, spp_chunk=2, progress=cb, preview_ms=-1)
    assert seen and seen[0][0] == abi.E_ARG and "rendering" in seen[0][1] and seen[1] == 1, seen
    assert fray.lib.frayhip_scene_camera_tiles(s._dev, 2, None) == abi.E_ARG                 # enable is -1, 0 or 1
    assert fray.lib.frayhip_scene_camera_tiles(None, -1, None) == abi.E_ARG
    assert s.camera_tiles() == 1
    s.close()
