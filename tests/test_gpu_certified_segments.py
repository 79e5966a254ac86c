"""Option "certified_segments" (default 1): in a scene whose nodes are all segment-plane nodes or exactly gated ones, k_pt_bounce's timed variant of flag
word 0 stores the term of a next-event segment itself, with no queue entry and no visible(), when the segment's ray is proven to miss every gate and its
ends lie on one side of every plane entry (DESIGN.md "Certified segments"; tests/test_certified_segments_host.py runs the rule on the host).  Such a
segment is one the reference's arithmetic finds unoccluded, so no picture may change by a single bit: with the option on or off, against the counting
kernels (which queue every segment) and against the oracle, and on against off in the contracted arithmetic."""
import numpy as np
import pytest

from conftest import open_scene
from test_certified_segments_host import eligible_by_rule
from test_gpu_segment_planes import GENERATED, bits

pytestmark = pytest.mark.gpu


def figures(s):
    return s.get_option("shadow_segments"), s.get_option("shadow_segments_certified")


def on_off_counted_oracle(s, abi, oracle, what):
    """Renders with the option on, off, on the counting kernels and on the oracle: four frames equal by bits; on against off in the contracted arithmetic; the
    counters as the issue states them.  Returns (eligible, certified with the option on, shadow segments, certified in the contracted arithmetic)."""
    assert s.get_option("certified_segments") == 1 and s.get_option("segment_planes") == 1                # the defaults
    eligible = s.get_option("certified_segments_eligible")
    on, _ = s.render(seed=42)
    segs, cert = figures(s)
    s.set_option("certified_segments", 0)
    assert s.get_option("certified_segments") == 0
    off, _ = s.render(seed=42)
    segs_off, cert_off = figures(s)
    s.set_option("certified_segments", 1)
    s.set_option("segment_planes", 0)                                   # the option has no effect while "segment_planes" is 0
    noplanes, _ = s.render(seed=42)
    segs_np, cert_np = figures(s)
    s.set_option("segment_planes", 1)
    counted, st = s.render(seed=42, stats=True)
    cert_counted = s.get_option("shadow_segments_certified")
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    print("%s: eligible %d; shadow_segments %d, certified %d (%.3f); option off: %d, %d; segment_planes off: %d, %d; counting frame: certified %d, shadow_rays %d"
          % (what, eligible, segs, cert, cert / max(segs, 1), segs_off, cert_off, segs_np, cert_np, cert_counted, st["shadow_rays"]))
    assert np.array_equal(bits(on), bits(off))
    assert np.array_equal(bits(on), bits(noplanes))
    assert np.array_equal(bits(on), bits(counted))
    assert np.array_equal(bits(on), bits(ref))
    assert segs == segs_off == segs_np and 0 <= cert <= segs
    assert cert_off == 0 and cert_np == 0 and cert_counted == 0
    assert st["shadow_rays"] == ost["shadow_rays"]                       # the counting variants keep queueing every segment
    s.set_option("fp_contract", 1)
    con, _ = s.render(seed=42)
    segs_con, cert_con = figures(s)
    s.set_option("certified_segments", 0)
    coff, _ = s.render(seed=42)
    segs_coff, cert_coff = figures(s)
    assert np.array_equal(bits(con), bits(coff))
    assert segs_con == segs_coff and cert_coff == 0
    s.set_option("certified_segments", 1)
    s.set_option("fp_contract", 0)
    return eligible, cert, segs, cert_con


PT = [
    ("cornell_box.fray", 64, 64, dict(numPaths=8), True),
    ("cornell_box.fray", 60, 60, dict(numPaths=8, stereoSeparation=12.0), True),         # the right eye continues the left eye's generators
    ("cornell_box.fray", 40, 40, dict(numPaths=8, maxTraceDepth=20), True),              # the long generators
    ("smallpt.fray", 64, 48, dict(numPaths=8), False),                                   # spheres: the feature is absent
    ("boxed.fray", 48, 36, dict(numPaths=8), False),                                     # KD meshes: the kernel variants without it
]


@pytest.mark.parametrize("scene,W,H,over,eligible", PT, ids=lambda v: v if isinstance(v, str) else None)
def test_frames_are_the_same_bits_with_and_without_certified_segments(fray, abi, oracle, gpu, scene, W, H, over, eligible):
    s = open_scene(fray, scene, W, H, gi=1, **over)
    s.beginRender()
    got, cert, segs, cert_con = on_off_counted_oracle(s, abi, oracle, "%s %s" % (scene, over))
    assert bool(got) == eligible == eligible_by_rule(s.desc)
    if eligible:
        assert cert > 0 and cert_con > 0
    else:
        assert cert == 0 and cert_con == 0
    s.close()


@pytest.mark.parametrize("what", list(GENERATED), ids=lambda v: v.replace(" ", "_").replace(",", ""))
def test_generated_rooms_render_the_same_bits(fray, abi, oracle, gpu, tmp_path, what):
    """Certified > 0 exactly where the scene is eligible.  "coplanar quads, the light in their plane" has plane nodes only, and is not eligible: every light
    sample lies IN the two quads' plane (sigma_b = 0), so that entry passes for no segment and the rule needs every entry -- the scene's flag says so
    (scene_arena.hpp fill_editable) and the bounce kernel does not evaluate a certificate that cannot hold.  Nor is "the room scaled by 1e4": at coordinates
    of 5e6 the margin of a wall's plane is near 1e-4 |N|, and a segment starts 1e-6 off the wall it was sampled on, inside that margin."""
    s = fray.Scene.parseScene(GENERATED[what][0](tmp_path))              # 48 x 48, 4 spp
    s.beginRender()
    got, cert, segs, cert_con = on_off_counted_oracle(s, abi, oracle, what)
    assert bool(got) == eligible_by_rule(s.desc)
    assert (cert > 0) == bool(got) and (cert_con > 0) == bool(got)
    s.close()


def test_a_moved_wall_ends_the_certificates_and_moving_it_back_restores_them(fray, abi, oracle, gpu):
    """frayhip_scene_update recomputes the scene's flag with the tables it follows from: a translated back wall is no plane node, so nothing is certified; with
    the wall back the frame and the counts are the original's."""
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, numPaths=8)
    s.beginRender()
    first, _ = s.render(seed=42)
    segs, cert = figures(s)
    assert s.get_option("certified_segments_eligible") == 1 and cert > 0
    fray.Transform(s.nodes[2]).translate(0, 0, 3).store(s.nodes[2])                       # the back wall
    s.update()
    moved, _ = s.render(seed=42)
    ref, _ = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    assert s.get_option("certified_segments_eligible") == 0 and s.get_option("shadow_segments_certified") == 0
    assert np.array_equal(bits(moved), bits(ref))
    fray.Transform().store(s.nodes[2])
    s.update()
    again, _ = s.render(seed=42)
    assert s.get_option("certified_segments_eligible") == 1
    assert figures(s) == (segs, cert)
    assert np.array_equal(bits(again), bits(first))
    s.close()


def test_share_of_certified_segments_on_cornell_box(fray, gpu):
    """No bound: prints certified / shadow_segments for cornell_box 400 x 400 x 8 spp (profiles/certified_segments/README.md quotes it)."""
    s = open_scene(fray, "cornell_box.fray", 400, 400, gi=1, numPaths=8)
    s.beginRender()
    s.render(seed=42)
    segs, cert = figures(s)
    print("cornell_box 400 x 400 x 8 spp: shadow_segments %d, certified %d, share %.4f" % (segs, cert, cert / segs))
    assert 0 < cert <= segs
    s.close()
