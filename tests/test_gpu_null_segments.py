"""Option "skip_null_segments" (default 1): the timed path-tracing kernels queue no next-event segment whose contribution is +0.0f in all
three channels by bit pattern (fray_amd/csrc/dev_shade.hpp nee_prepare).  k_pt_shadow would have stored three +0 words for such a segment
whatever visible() answered, which is what path_shade stores itself when nothing was queued: so no picture may change by a single bit, with
the option on or off, against the counting kernels (which keep tracing every segment the reference traces) and against the oracle."""
import numpy as np
import pytest

from conftest import open_scene

pytestmark = pytest.mark.gpu


def bits(img):
    return np.ascontiguousarray(img).view(np.uint32)        # integer views: +0 and -0 differ, NaNs compare by payload


PT = [
    ("cornell_box.fray", 64, 64, dict(numPaths=8)),                                   # Lambert hits facing away from the light sample, the mirror block
    ("smallpt.fray", 64, 48, dict(numPaths=8)),                                       # mirror and glass spheres
    ("../tests/scenes/csg_nested.fray", 80, 60, dict(numPaths=8)),                    # the Cube / CSG kernel variants
    ("boxed.fray", 48, 36, dict(numPaths=8)),                                         # KD meshes, Phong under gi (the reference's default red BRDF)
    ("cornell_box.fray", 60, 60, dict(numPaths=8, stereoSeparation=12.0)),            # the right eye continues the left eye's generators
    ("cornell_box.fray", 40, 40, dict(numPaths=8, maxTraceDepth=20)),                 # the long generators (MtPath)
]


@pytest.mark.parametrize("scene,W,H,over", PT, ids=lambda v: v if isinstance(v, str) else None)
def test_frames_are_the_same_bits_with_and_without_null_segments(fray, abi, oracle, gpu, scene, W, H, over):
    s = open_scene(fray, scene, W, H, gi=1, **over)
    s.beginRender()
    assert s.get_option("skip_null_segments") == 1                                    # the default
    on, _ = s.render(seed=42)
    segs_on = s.get_option("shadow_segments")
    s.set_option("skip_null_segments", 0)
    assert s.get_option("skip_null_segments") == 0
    off, _ = s.render(seed=42)
    segs_off = s.get_option("shadow_segments")
    s.set_option("skip_null_segments", 1)
    counted, st = s.render(seed=42, stats=True)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    print("%s %s: shadow segments %d with the option, %d without, the reference's shadow rays %d" % (scene, over, segs_on, segs_off, ost["shadow_rays"]))
    assert ref.mean() > 1e-3
    assert np.array_equal(bits(on), bits(off))
    assert np.array_equal(bits(on), bits(counted))
    assert np.array_equal(bits(on), bits(ref))
    # the counting kernels trace every segment whatever the option says; the timed ones with the option off queue the same segments
    assert st["shadow_rays"] == ost["shadow_rays"]
    assert segs_off == st["shadow_rays"]
    assert 0 < segs_on <= segs_off
    # the kernels built with fused multiply-adds are the same source: on against off, bit for bit
    s.set_option("fp_contract", 1)
    con, _ = s.render(seed=42)
    s.set_option("skip_null_segments", 0)
    coff, _ = s.render(seed=42)
    assert np.array_equal(bits(con), bits(coff))
    s.close()


ALL_MIRRORS = """
GlobalSettings {
	frameWidth 64
	frameHeight 48
	ambientLight (0.1, 0.1, 0.1)
	maxTraceDepth 5
	wantAA off
}
Camera camera {
	position (0, 6, -14)
	pitch -15
	fov 60
}
RectLight l1 {
	translate (0, 14, 0)
	scale (6, 6, 6)
	power 30
	xSubd 2
	ySubd 2
}
Plane floor {
	limit 30
}
Sphere ball {
	R 2
}
Refl mirror {
	multiplier 0.9
}
Refl dim {
	multiplier 0.6
}
Node floorNode {
	geometry floor
	shader dim
}
Node ballA {
	geometry ball
	shader mirror
	translate (-3, 2, 0)
}
Node ballB {
	geometry ball
	shader mirror
	translate (3, 2, 1)
	scale (1, 1.5, 1)
}
"""


def test_a_scene_of_mirrors_queues_no_segment_at_all(fray, abi, oracle, gpu, tmp_path):
    """Every surface is a Refl shader (Reflection::eval is zero by construction): every next-event sample is null."""
    f = tmp_path / "mirrors.fray"
    f.write_text(ALL_MIRRORS)
    s = fray.Scene.parseScene(str(f))
    s.settings.gi, s.settings.numPaths = 1, 8
    assert s.samples_per_pixel() == 8
    s.beginRender()
    on, _ = s.render(seed=42)
    segs_on = s.get_option("shadow_segments")
    s.set_option("skip_null_segments", 0)
    off, _ = s.render(seed=42)
    segs_off = s.get_option("shadow_segments")
    counted, st = s.render(seed=42, stats=True)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    print("mirrors: shadow segments %d with the option, %d without; shadow rays of the counting pass %d, of the oracle %d; mean of the frame %g"
          % (segs_on, segs_off, st["shadow_rays"], ost["shadow_rays"], ref.mean()))
    assert ref.mean() > 1e-3                                  # the light itself, seen in the mirrors
    assert np.array_equal(bits(on), bits(ref)) and np.array_equal(bits(off), bits(ref)) and np.array_equal(bits(counted), bits(ref))
    assert st["shadow_rays"] == ost["shadow_rays"] > 0
    assert segs_on == 0
    assert segs_off == st["shadow_rays"]
    s.close()


def test_cornell_box_share_of_segments_kept(fray, gpu):
    """A sanity band, not a measurement: 86.0 % of cornell_box's next-event segments are lit on a CPU count of the 1920 x 1080 x 64 spp frame (every 23rd
    bucket); the option must skip the others and must not eat lit ones."""
    s = open_scene(fray, "cornell_box.fray", 400, 400, gi=1, numPaths=8)
    s.beginRender()
    s.render(seed=42)
    kept = s.get_option("shadow_segments")
    _, st = s.render(seed=42, stats=True)
    share = kept / st["shadow_rays"]
    print("cornell_box 400 x 400 x 8 spp: %d of %d next-event segments queued: %.4f" % (kept, st["shadow_rays"], share))
    assert 0.80 <= share <= 0.92, share
    s.close()
