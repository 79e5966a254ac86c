"""The seed table (option "seed_table_mib"): x[397] of every camera sample's seeding recurrence depends on the contract seed, the frame
size and the bucket share alone, so a scene handle keeps the words k_seed wrote from one frame to the next and launches k_seed only for sample
planes it does not hold.  The kernels read the same words from another address: every comparison here is bit for bit, against a second handle
of the same scene that renders with the table off ("seed_table_mib" 0, which is the behaviour before the table)."""
import numpy as np
import pytest

from conftest import open_scene

pytestmark = pytest.mark.gpu


def pair(fray, name, W, H, over):
    """Two handles of one scene: the table at its default, and off."""
    s = open_scene(fray, name, W, H, **over)
    s.beginRender()
    r = open_scene(fray, name, W, H, **over)
    r.beginRender()
    r.set_option("seed_table_mib", 0)
    return s, r


def figures(s):
    return s.get_option("seed_launches"), s.get_option("seed_planes_reused")


def set_spp(s, field, spp):
    if hasattr(s.settings, field):
        setattr(s.settings, field, spp)
    else:
        setattr(s.camera, field, spp)
    s.beginFrame()


# (id, scene, W, H, overrides, what get_option("whitted_path") must say afterwards, None for path-traced frames)
KINDS = [
    ("pt-mono", "cornell_box.fray", 96, 64, dict(gi=1, numPaths=8, wantAA=0), None),
    ("pt-stereo", "cornell_box.fray", 60, 60, dict(gi=1, numPaths=8, wantAA=0, stereoSeparation=12.0), None),
    ("pt-long-generators", "cornell_box.fray", 40, 40, dict(gi=1, numPaths=8, wantAA=0, maxTraceDepth=20), None),
    ("wavefront-dof", "forest.fray", 96, 72, dict(wantAA=0, dof=1, numDOFSamples=8, interactive=0), 1),
    ("fused-dof", "zaphod.fray", 96, 64, dict(wantAA=0, dof=1, numDOFSamples=8), 2),
    ("k_whitted", "smallpt.fray", 64, 48, dict(gi=0, wantAA=1), 0),
]


@pytest.mark.parametrize("case", KINDS, ids=lambda c: c[0])
@pytest.mark.parametrize("chunk", [0, 3])
def test_the_same_frame_twice_seeds_once(fray, gpu, case, chunk):
    _, name, W, H, over, path = case
    s, r = pair(fray, name, W, H, over)
    spp = s.samples_per_pixel()
    assert s.get_option("seed_table_mib") == 4096 and s.get_option("seed_table_bytes") == 0
    ref, _ = r.render(seed=42, spp_chunk=chunk)
    parent_launches, none = figures(r)
    assert parent_launches == (-(-spp // chunk) if chunk else parent_launches) > 0 and none == 0 and r.get_option("seed_table_bytes") == 0
    a, _ = s.render(seed=42, spp_chunk=chunk)
    la, ra = figures(s)
    print("%s chunk %d: spp %d, first frame %d launches, table-off frame %d, table %d bytes" % (case[0], chunk, spp, la, parent_launches, s.get_option("seed_table_bytes")))
    assert la == parent_launches and ra == 0                      # a miss is the parent's launches, written to another address
    assert s.get_option("seed_table_bytes") >= spp * 4 * W * H
    if path is not None:
        assert s.get_option("whitted_path") == path
    b, _ = s.render(seed=42, spp_chunk=chunk)
    assert figures(s) == (0, spp)
    assert np.array_equal(a, ref) and np.array_equal(b, ref)
    assert ref.mean() > 1e-3
    # the camera is not part of the key
    for t in (s, r):
        t.camera.yaw += 7.0
        t.beginFrame()
    c, _ = s.render(seed=42, spp_chunk=chunk)
    cref, _ = r.render(seed=42, spp_chunk=chunk)
    assert figures(s) == (0, spp)
    assert np.array_equal(c, cref) and not np.array_equal(c, ref)
    s.close()
    r.close()


def test_key_changes_refill_the_table(fray, gpu):
    s, r = pair(fray, "cornell_box.fray", 96, 64, dict(gi=1, numPaths=8, wantAA=0))
    spp = 8

    def both(**kw):
        img, _ = s.render(**kw)
        ref, _ = r.render(**kw)
        assert np.array_equal(img, ref), kw
        return img

    a = both(seed=42)
    assert figures(s)[1] == 0
    both(seed=42)
    assert figures(s) == (0, spp)
    # the seed, and back: the table holds one key
    b = both(seed=43)
    assert figures(s)[0] > 0 and figures(s)[1] == 0 and not np.array_equal(a, b)
    a2 = both(seed=42)
    assert figures(s)[0] > 0 and figures(s)[1] == 0 and np.array_equal(a, a2)
    # the frame size: a larger frame grows the allocation, a smaller one reuses it
    held = s.get_option("seed_table_bytes")
    for W, H in ((144, 100), (50, 50), (144, 100)):
        for t in (s, r):
            t.settings.frameWidth, t.settings.frameHeight = W, H
            t.beginFrame()
        both(seed=42)
        assert figures(s)[0] > 0 and figures(s)[1] == 0, (W, H)
        both(seed=42)
        assert figures(s) == (0, spp), (W, H)
    assert s.get_option("seed_table_bytes") > held
    # two shards rendered alternately through one handle: every change of the bucket share refills
    for rep in range(2):
        for first in (0, 1):
            both(seed=42, bucket_first=first, bucket_stride=2)
            assert figures(s)[0] > 0 and figures(s)[1] == 0, (rep, first)
    both(seed=42, bucket_first=1, bucket_stride=2)
    assert figures(s) == (0, spp)
    both(seed=42, bucket_first=1, bucket_stride=3)
    assert figures(s)[0] > 0 and figures(s)[1] == 0
    s.close()
    r.close()


def test_plan_changes_under_one_key(fray, gpu):
    s, r = pair(fray, "cornell_box.fray", 96, 64, dict(gi=1, numPaths=10, wantAA=0))
    refs = {}

    def ref(spp, seed):
        if (spp, seed) not in refs:
            set_spp(r, "numPaths", spp)
            refs[spp, seed] = r.render(seed=seed)[0]
        return refs[spp, seed]

    # batches of 1, 3 and 5 planes (and the plan's own) over a table that holds planes 0..3: some batches find all, some part, some none of their planes
    for chunk in (0, 1, 3, 5):
        seed = 100 + chunk
        set_spp(s, "numPaths", 4)
        img, _ = s.render(seed=seed)
        assert figures(s)[1] == 0 and np.array_equal(img, ref(4, seed))
        set_spp(s, "numPaths", 10)
        img, _ = s.render(seed=seed, spp_chunk=chunk)
        launches, reused = figures(s)
        print("chunk %d: 4 planes held, 10 asked: %d launches, %d planes reused" % (chunk, launches, reused))
        assert reused == 4 and launches > 0 and np.array_equal(img, ref(10, seed)), chunk
        if chunk:
            assert launches == -(-10 // chunk) - 4 // chunk, chunk          # one launch per batch that lacks a plane: a batch's missing planes are one run
        img, _ = s.render(seed=seed, spp_chunk=chunk)
        assert figures(s) == (0, 10) and np.array_equal(img, ref(10, seed)), chunk
    # batch lanes: planes written on one lane's stream are read on another's in the next frame
    seed = 7
    for lanes_fill, chunk_fill, lanes_hit, chunk_hit in ((1, 2, 4, 3), (4, 2, 1, 0), (4, 1, 4, 4)):
        seed += 1
        s.set_option("pt_lanes", lanes_fill)
        img, _ = s.render(seed=seed, spp_chunk=chunk_fill)
        assert figures(s)[1] == 0 and np.array_equal(img, ref(10, seed))
        s.set_option("pt_lanes", lanes_hit)
        for rep in range(3):
            img, _ = s.render(seed=seed, spp_chunk=chunk_hit)
            assert figures(s) == (0, 10) and np.array_equal(img, ref(10, seed)), (lanes_fill, lanes_hit, rep)
    s.set_option("pt_lanes", 4)
    # spp 8 -> 16 -> 4: the step to 16 seeds planes 8..15 only
    seed = 42
    set_spp(s, "numPaths", 8)
    img, _ = s.render(seed=seed)
    assert figures(s)[1] == 0 and np.array_equal(img, ref(8, seed))
    held = s.get_option("seed_table_bytes")
    set_spp(s, "numPaths", 16)
    img, _ = s.render(seed=seed)
    launches, reused = figures(s)
    assert reused == 8 and launches > 0 and np.array_equal(img, ref(16, seed))
    assert s.get_option("seed_table_bytes") > held > 0
    set_spp(s, "numPaths", 4)
    img, _ = s.render(seed=seed)
    assert figures(s) == (0, 4) and np.array_equal(img, ref(4, seed))
    set_spp(s, "numPaths", 16)
    img, _ = s.render(seed=seed, spp_chunk=5)
    assert figures(s) == (0, 16) and np.array_equal(img, ref(16, seed))
    # a counting frame (one lane, another chunk) fills the table, a timed frame reads it -- and the other way round
    seed = 77
    set_spp(s, "numPaths", 10)
    img, st = s.render(seed=seed, spp_chunk=3, stats=True)
    assert figures(s) == (4, 0) and st["samples"] > 0 and np.array_equal(img, ref(10, seed))
    img, _ = s.render(seed=seed)
    assert figures(s) == (0, 10) and np.array_equal(img, ref(10, seed))
    img, st2 = s.render(seed=seed, spp_chunk=4, stats=True)
    assert figures(s) == (0, 10) and np.array_equal(img, ref(10, seed))
    assert all(st2[k] == st[k] for k in ("closest_rays", "shadow_rays", "samples"))
    s.close()
    r.close()


def test_a_cancelled_progressive_frame_leaves_its_planes(fray, gpu):
    s, r = pair(fray, "cornell_box.fray", 96, 64, dict(gi=1, numPaths=8, wantAA=0))
    for t in (s, r):
        t.set_option("pt_lanes", 1)          # one batch traced ahead of the one reported: the cancel after batch 0 leaves batches 0 and 1 enqueued
    calls = []

    def cancel_at_once(info):
        calls.append(dict(samples_done=info["samples_done"], final=info["final"]))
        return True
    part, st = s.render(seed=42, spp_chunk=2, progress=cancel_at_once)
    assert st["cancelled"] and st["samples_done"] == 4 and calls[0]["samples_done"] == 2
    assert figures(s) == (2, 0)
    rpart, rst = r.render(seed=42, spp_chunk=2, progress=lambda info: True)
    assert rst["cancelled"] and rst["samples_done"] == 4 and np.array_equal(part, rpart)
    full, _ = s.render(seed=42, spp_chunk=3)          # batches 0..2, 3..5, 6..7 over planes 0..3
    assert figures(s) == (2, 4)
    ref, _ = r.render(seed=42)
    assert np.array_equal(full, ref) and not np.array_equal(part, ref)
    # the same through the progressive entry, to the end
    prog, st = s.render(seed=42, spp_chunk=2, progress=lambda info: False, preview_ms=0)
    assert not st["cancelled"] and figures(s) == (0, 8) and np.array_equal(prog, ref)
    s.close()
    r.close()


def test_fp_contract_frames_share_the_table(fray, gpu):
    s, r = pair(fray, "cornell_box.fray", 96, 64, dict(gi=1, numPaths=8, wantAA=0))
    exact, _ = s.render(seed=42)
    assert figures(s)[1] == 0
    for t in (s, r):
        t.set_option("fp_contract", 1)
    con, _ = s.render(seed=42)
    assert figures(s) == (0, 8) and s.get_option("contracted_launches") > 0
    rcon, _ = r.render(seed=42)
    assert np.array_equal(con, rcon)
    for t in (s, r):
        t.set_option("fp_contract", 0)
    again, _ = s.render(seed=42)
    rexact, _ = r.render(seed=42)
    assert figures(s) == (0, 8) and np.array_equal(again, exact) and np.array_equal(exact, rexact)
    s.close()
    r.close()


def test_a_cap_too_small_for_the_frame_renders_as_without_the_table(fray, gpu):
    s, r = pair(fray, "cornell_box.fray", 256, 256, dict(gi=1, numPaths=8, wantAA=0))
    s.set_option("seed_table_mib", 1)                  # 36 buckets x 2304 items x 4 B x 8 planes = 2.5 MiB
    assert s.get_option("seed_table_mib") == 1
    ref, _ = r.render(seed=42, spp_chunk=2)
    for rep in range(2):
        img, _ = s.render(seed=42, spp_chunk=2)
        assert figures(s) == figures(r) == (4, 0) and s.get_option("seed_table_bytes") == 0
        assert np.array_equal(img, ref)
    # ... while a frame of 3 planes fits: the cap is per frame
    for t in (s, r):
        set_spp(t, "numPaths", 3)
    ref3, _ = r.render(seed=42)
    for expect in ((1, 0), (0, 3)):
        img, _ = s.render(seed=42)
        assert figures(s) == expect and 0 < s.get_option("seed_table_bytes") <= 1 << 20 and np.array_equal(img, ref3)
    # lowering the cap below what is held gives the memory back at once; 0 is off
    s.set_option("seed_table_mib", 0)
    assert s.get_option("seed_table_bytes") == 0
    img, _ = s.render(seed=42)
    assert figures(s) == (1, 0) and s.get_option("seed_table_bytes") == 0 and np.array_equal(img, ref3)
    s.close()
    r.close()


def test_a_wavefront_frame_without_draws_launches_no_k_seed(fray, gpu):
    s, r = pair(fray, "zaphod.fray", 96, 64, dict(wantAA=0, dof=0))
    ref, _ = r.render(seed=42)
    assert figures(r) == (0, 0)
    for rep in range(2):
        img, _ = s.render(seed=42)
        assert s.get_option("whitted_path") == 2
        assert figures(s) == (0, 0) and s.get_option("seed_table_bytes") == 0 and np.array_equal(img, ref)
    # the lens draws: seeded, then held
    for t in (s, r):
        t.camera.dof, t.camera.numDOFSamples = 1, 6
        t.beginFrame()
    ref, _ = r.render(seed=42)
    for expect in ((1, 0), (0, 6)):
        img, _ = s.render(seed=42)
        assert figures(s) == expect and np.array_equal(img, ref)
    # and without draws again nothing is launched and nothing is counted as reused
    for t in (s, r):
        t.camera.dof = 0
        t.beginFrame()
    img, _ = s.render(seed=42)
    assert figures(s) == (0, 0)
    s.close()
    r.close()


def test_the_options_by_name(fray, gpu):
    s = open_scene(fray, "cornell_box.fray", 48, 48, gi=1, numPaths=2, wantAA=0)
    s.beginRender()
    assert s.get_option("seed_table_mib") == 4096
    for k in ("seed_table_bytes", "seed_launches", "seed_planes_reused"):
        assert s.get_option(k) == 0
        with pytest.raises(fray.FrayError, match="unknown option"):
            s.set_option(k, 1)                           # figures, not knobs
    with pytest.raises(fray.FrayError, match="seed_table_mib"):
        s.set_option("seed_table_mib", -1)
    with pytest.raises(fray.FrayError, match="seed_table_mib"):
        s.set_option("seed_table_mib", (1 << 20) + 1)
    assert s.get_option("seed_table_mib") == 4096
    s.set_option("seed_table_mib", 7)
    assert s.get_option("seed_table_mib") == 7
    s.set_option("seed_table_mib", 0)
    assert s.get_option("seed_table_mib") == 0
    s.close()
