"""Tight gates (frayhip_scene_tight_gates / Scene.tight_gates, on by default): the path tracer's producers test a gate that stands for an eligible mesh by the box of the mesh's own triangles and a
guard against rays nearly parallel to a face (fray_amd/csrc/dev_gatecert.hpp: the certificate and its proof; tests/test_gatecert_host.py runs it on the
host), not by the mesh's bounding box, which for an OBJ mesh also holds the loader's dummy vertex (0, 0, 0).  A certified ray is one that no triangle of
the mesh accepts as the reference's arithmetic computes it: the option changes which rays are filed gate-free and which segments are certified, never a
ray, so no picture may change by a single bit -- on against off, against the counting kernels and against the oracle."""
import numpy as np
import pytest

from conftest import open_scene
from test_gpu_segment_planes import bits, read_obj, room

pytestmark = pytest.mark.gpu

COUNTERS = ("closest_rays", "shadow_rays", "node_tests", "prim_tests", "samples")
ALL_COUNTERS = COUNTERS + ("tri_tests", "kd_inner_visits", "leaf_refs", "smooth_hits", "texture_fetches")


def figures(s):
    return s.get_option("shadow_segments"), s.get_option("shadow_segments_certified")


def on_off_counted_oracle(s, abi, oracle, what):
    """Four frames equal by bits: the option on, off, the counting kernels, the oracle.  The counting kernels still ask every node: their counters are the
    same with the option on and off, every one exactly, and the oracle's -- rays, node and primitive tests and samples exactly; tri_tests within the few
    per million by which it differs from the oracle's in this suite with or without any option (tests/test_gpu_segment_planes.py: the device's
    correctly rounded trigonometry against glibc's moves a box test at an edge).  Returns (eligible gates, (segments, certified) on, the same off)."""
    enabled, eligible = s.tight_gates()
    assert enabled == 1                                                    # the default
    on, _ = s.render(seed=42)
    fig_on = figures(s)
    counted, st = s.render(seed=42, stats=True)
    assert s.tight_gates(0) == (0, eligible)
    off, _ = s.render(seed=42)
    fig_off = figures(s)
    counted_off, st_off = s.render(seed=42, stats=True)
    assert s.tight_gates(1) == (1, eligible)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    print("%s: eligible gates %d; shadow_segments %d, certified %d (%.4f) with the option, %d, %d (%.4f) without"
          % (what, eligible, fig_on[0], fig_on[1], fig_on[1] / max(fig_on[0], 1), fig_off[0], fig_off[1], fig_off[1] / max(fig_off[0], 1)))
    print("   work counters GPU - oracle:", {k: int(st[k]) - int(ost[k]) for k in COUNTERS + ("tri_tests",)})
    assert np.array_equal(bits(on), bits(off))
    assert np.array_equal(bits(on), bits(counted))
    assert np.array_equal(bits(on), bits(counted_off))
    assert np.array_equal(bits(on), bits(ref))
    assert fig_on[0] == fig_off[0]                                         # the segments decided are the same ones; only how
    for k in ALL_COUNTERS:
        assert st[k] == st_off[k], (k, st[k], st_off[k])
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert abs(st["tri_tests"] - ost["tri_tests"]) <= 2e-5 * ost["tri_tests"] + 2, (st["tri_tests"], ost["tri_tests"])
    return eligible, fig_on, fig_off


def test_cornell_box_is_the_same_bits_and_certifies_more_segments(fray, abi, oracle, gpu):
    """cornell_box 64 x 64 x 8 spp: both blocks are eligible; the frames are equal; and the certified share of the next-event segments is above the one
    with the option off in the same run (the gates are smaller, so more segments' rays miss them)."""
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, numPaths=8)
    s.beginRender()
    eligible, (segs, cert), (segs_off, cert_off) = on_off_counted_oracle(s, abi, oracle, "cornell_box 64 x 64 x 8 spp")
    assert eligible == 2
    assert segs == segs_off > 0
    assert cert / segs > cert_off / segs_off > 0
    s.close()


def test_contracted_frames_are_the_same_bits_with_and_without_tight_gates(fray, gpu):
    """fp_contract = 1 has no oracle; the gate changes which rays are filed where, never a ray: on against off, bit for bit."""
    s = open_scene(fray, "cornell_box.fray", 64, 64, gi=1, numPaths=8)
    s.beginRender()
    s.set_option("fp_contract", 1)
    on, _ = s.render(seed=42)
    fig_on = figures(s)
    assert s.get_option("contracted_launches") > 0
    s.tight_gates(0)
    off, _ = s.render(seed=42)
    fig_off = figures(s)
    print("contracted: certified %d of %d with the option, %d of %d without" % (fig_on[1], fig_on[0], fig_off[1], fig_off[0]))
    assert np.array_equal(bits(on), bits(off))
    assert fig_on[0] == fig_off[0] and fig_on[1] >= fig_off[1]
    s.close()


def at_height(path, y):
    """the generated room's camera moved to height y (it looks along +z, pitch 0: the middle rows' rays are nearly horizontal)"""
    text = open(path).read()
    assert "position (278.0, 273.0, -800.0)" in text
    open(path, "w").write(text.replace("position (278.0, 273.0, -800.0)", "position (278.0, %r, -800.0)" % y))
    return path


def sliver_block():
    """a copy of the short block, floating 200 above it, with one more triangle lying a millionth above its top face: a sliver by dev_gatecert.hpp's
    bound (E^2 / |N|_1 = 1e8), so this third gate gets no tight record"""
    vs, fs = read_obj("shortblock.obj")
    vs = [(x, y + 200.0, z) for x, y, z in vs]
    n = len(vs)
    return ("sliverblock", vs + [(300.0, 365.0, 150.0), (400.0, 365.0, 150.0), (350.0, 365.000001, 150.0)], fs + [(n + 1, n + 2, n + 3)])


ROOMS = {
    # the camera in the plane of the short block's top face (y = 165): primary rays of the middle rows, and what bounces off along them, run nearly
    # parallel to that face on either side of it -- the rays the guard exists for; both blocks eligible
    "camera in the plane of a top face": (lambda p: at_height(room(p), 165.0), 2, True),
    # a transformed block is no exact gate, and with an inexact gate in the scene gate-free is a hint again: the other block's record is made but not used
    "a block with a transform": (lambda p: at_height(room(p, node_lines={"shortblock": ["translate (0, 0, 3)"]}), 165.0), 1, False),
    "a third block with a sliver": (lambda p: at_height(room(p, extra=[sliver_block()]), 165.0), 2, True),
}


@pytest.mark.parametrize("what", list(ROOMS), ids=lambda v: v.replace(" ", "_"))
def test_generated_rooms_render_the_same_bits(fray, abi, oracle, gpu, tmp_path, what):
    """48 x 48 x 4 spp.  An ineligible gate keeps the mesh's bounding box, and the picture is the oracle's either way."""
    make, eligible, exact = ROOMS[what]
    s = fray.Scene.parseScene(make(tmp_path))
    s.beginRender()
    got, (segs, cert), (segs_off, cert_off) = on_off_counted_oracle(s, abi, oracle, what)
    assert got == eligible
    if not exact:
        assert cert == cert_off == 0 and s.get_option("certified_segments_eligible") == 0
    else:
        # (no order between the two counts here: with the camera in the plane of a face that the tight and the bounding box share, the two certificates' FP32
        # margins, which follow the boxes' centres, decide a handful of grazing rays differently)
        assert cert > 0 and cert_off > 0
    s.close()
