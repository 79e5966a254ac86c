"""Specular feature frames on every kernel flag word and over the sample loop (include/frayhip.h "specular feature frames"):
1. the chain pinned bit for bit by the numpy walk (tests/specular_ref.py) on the scenes of tests/specular_cases.py -- Cube / CSG, KD and textured
   words, a checker floor, the reflected environment and a rect light as terminals -- under K in (1, 3, 8), with the counting variant's outputs
   and counters; tests/test_specular_ref.py establishes on the CPU what the cases are claimed to show;
2. per word, the walk fed by the ray queries equals the walk fed by the CPU oracle;
3. n > 1: Whitted AA and jittered gi frames equal the walks at the samples' film positions reduced in float32, for k_features_specular and, with
   walks of no step, for k_features;
4. a bump map in a chain, against the Whitted frame of the scene in Const paint."""
import numpy as np
import pytest

import specular_cases as SC
import specular_ref as R
from conftest import open_scene
from test_gpu_shade import jitter, sample_seed

pytestmark = pytest.mark.gpu
F32 = np.float32
KS = (1, 3, 8)


def _assert_pinned(s, ch, K, label):
    """Both outputs of the timed and of the counting variant against the walk ch, every channel of every pixel bit for bit; the counters against
    the walk's segments: `samples` one per pixel, `closest_rays` one search per segment, b + 1 of them per sample."""
    feat, plane = s.render_features_specular(K, 1, bounces=True)
    assert np.array_equal(plane, ch["b"].astype(F32)), label
    assert np.array_equal(feat[..., 0:3], ch["pos"].astype(F32)), label
    assert np.array_equal(feat[..., 9], ch["depth"].astype(F32)), label
    assert np.array_equal(feat[..., 3:6], ch["nrm"].astype(F32)), label
    assert ch["alb_known"].all(), label
    assert np.array_equal(feat[..., 6:9], ch["alb"]), label
    f2, p2, st = s.render_features_specular(K, 1, bounces=True, stats=True)
    assert np.array_equal(f2, feat) and np.array_equal(p2, plane), label
    print("%s: samples %d, closest_rays %d, the walk's segments %d" % (label, st["samples"], st["closest_rays"], int((ch["b"] + 1).sum())))
    assert st["samples"] == ch["b"].size, label
    assert st["closest_rays"] == int((ch["b"].astype(np.int64) + 1).sum()), label
    return feat, plane


def _env_of(s, first):
    """shade_env, checked once where the existing tests pin it: at the primary misses the Whitted colour of the camera ray is the first-hit
    frame's albedo (the environment's colour along the ray)"""
    if not R.has_environment(s.desc):
        return None
    env = R.shade_env(s)
    o, d = s.camera_rays()
    miss = s.trace_rays(o, d)["hit_id"] == -1
    assert miss.sum() > 50 and np.array_equal(env(o[miss], d[miss]), first[miss][:, 6:9]) and np.any(first[miss][:, 6:9] > 0)
    return env


@pytest.mark.parametrize("name", list(SC.CASES))
def test_chain_is_pinned_on_every_word(fray, gpu, tmp_path, name):
    """Wall time on an MI355X: 0.2 s (csg_nested), 0.12 s (forest_mirror), 0.02 s or less for each of the others."""
    build, size, word, claims = SC.CASES[name]
    s = build(fray, tmp_path, *(size or (None, None)))
    desc = s.desc
    assert R.flag_word(desc) == word
    s.beginRender()
    first = s.render_features(1)
    env = _env_of(s, first)
    kinds = np.array([desc.shaders[desc.nodes[i].shader].kind for i in range(desc.n_nodes)])
    for K in KS:
        label = "%s K=%d" % (name, K)
        ch = R.walk_frame(s, K, env=env)
        feat, plane = _assert_pinned(s, ch, K, label)
        # what the case is there for (tests/test_specular_ref.py has the same from the CPU oracle)
        assert (ch["b"] > 0).mean() > 0.05, label
        t = SC.terminals(desc, ch)
        fk = np.where(ch["f_id"] >= 0, kinds[np.where(ch["f_id"] >= 0, ch["f_id"], 0)], -1)
        for claim in claims:
            seen = (fk == 3) if claim == "mir" else (fk == 4) if claim == "glass" else t[claim]
            assert seen.sum() >= (5 if claim in ("mir", "glass") else 10), (label, claim)
        if "light" in claims:                            # the light's row behind a mirror (the floor or the short block): its colour times the mult
            px = t["light"]
            L = desc.lights[-2 - int(ch["t_id"][px][0])]
            mult = np.array([desc.shaders[desc.nodes[int(i)].shader].mult[:] for i in ch["f_id"][px]], F32)
            assert (ch["b"][px] == 1).all() and (fk[px] == 3).all() and (ch["f_id"][px] == SC.CORNELL_FLOOR).sum() >= 10
            assert np.array_equal(feat[px][:, 6:9], mult * np.array(L.color[:], F32))
            assert (feat[px][:, 9] > 0).all() and np.array_equal(feat[px][:, 0:3], ch["pos"][px].astype(F32))
        if "environment" in claims:                      # a reflected miss: zeros but for the albedo, which is not black
            px = t["environment"]
            assert not feat[px][:, 0:6].any() and not feat[px][:, 9].any() and np.any(feat[px][:, 6:9] > 0)
        same = plane == 0
        assert np.array_equal(feat[same], first[same]) and not np.array_equal(feat[~same], first[~same]), label
    s.close()


# ---- 2. the two traces -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_floor_mirror", "csg_nested", "forest_mirror", "generated_f2_s%d" % SC.GENERATED_SEEDS[2][0]])
def test_query_fed_walk_equals_oracle_fed_walk(fray, oracle, gpu, tmp_path, name):
    """One case per even flag word (0, 2, 4, 8), a 32 x 24 grid of film positions between the pixel centres.  Everything but the albedo must be
    equal; an albedo may differ only at a checker-painted Sphere terminal, whose u, v come out of atan2 / asin (the device's against glibc's):
    the number of such rays is printed (0 of 768 in each of the four cases on an MI355X)."""
    build, size, word, _ = SC.CASES[name]
    s = build(fray, tmp_path, *(size or (None, None)))
    desc = s.desc
    W, H = s.frame_size
    gy, gx = np.mgrid[0:24, 0:32]
    xy = np.stack([(gx + 0.37) * (W / 32.0), (gy + 0.61) * (H / 24.0)], axis=-1).astype(np.float64)
    s.beginRender()
    o, d = s.camera_rays(xy)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    so, sd = np.zeros(3), np.zeros(3)
    for i, (x, y) in enumerate(xy.reshape(-1, 2)):       # the camera rays themselves: the oracle's, bit for bit
        oracle.lib.fray_oracle_camera_ray(desc, float(x), float(y), so.ctypes.data, sd.ctypes.data)
        assert np.array_equal(so, o[i]) and np.array_equal(sd, d[i])
    a = R.walk_chain(desc, o, d, 8, R.query_trace(s))
    b = R.walk_chain(desc, o, d, 8, R.oracle_trace(oracle, desc))
    assert (a["b"] > 0).sum() > 20
    for k in a:
        if k not in ("alb", "alb_known"):
            assert np.array_equal(a[k], b[k]), (name, k)
    differ = (a["alb"] != b["alb"]).any(axis=1)
    t = a["t_id"]
    on_sphere = (t >= 0) & np.array([desc.geoms[desc.nodes[i].geom].kind == 1 for i in range(desc.n_nodes)])[np.where(t >= 0, t, 0)]
    print("%s: %d of %d rays differ in albedo (checker u, v of a Sphere terminal)" % (name, int(differ.sum()), len(t)))
    assert not (differ & ~(on_sphere & SC.terminals(desc, a)["checker_paint"])).any()
    s.close()


# ---- 3. the sample loop -------------------------------------------------------------------------------------------------------------------------
def _assert_sample_loop(s, n, seed, positions, K, label):
    """render_features_specular(K, n) and render_features(n) against n walks (of at most K steps, and of none) at the samples' film positions,
    reduced as the kernels reduce: every channel and the plane, bit for bit."""
    W, H = s.frame_size
    xys = [positions(i) for i in range(n)]
    feat, plane, known = R.reduce_walks([R.walk_frame(s, K, xy) for xy in xys])
    assert known.all(), label
    got, got_plane = s.render_features_specular(K, n, seed=seed, bounces=True)
    assert np.array_equal(got_plane, plane), label
    assert np.array_equal(got, feat), (label, np.argwhere((got != feat).any(axis=2))[:5].tolist())
    first, zeros, known = R.reduce_walks([R.walk_frame(s, 0, xy) for xy in xys])
    assert known.all() and not zeros.any()
    got_first = s.render_features(n, seed=seed)
    assert np.array_equal(got_first, first), (label, np.argwhere((got_first != first).any(axis=2))[:5].tolist())
    # the counting variants reduce the same way
    f2, p2, st = s.render_features_specular(K, n, seed=seed, bounces=True, stats=True)
    assert np.array_equal(f2, got) and np.array_equal(p2, plane) and st["samples"] == W * H * n, label
    assert np.array_equal(s.render_features(n, seed=seed, stats=True)[0], first), label
    return got, plane, first


def test_whitted_aa_samples_are_reduced_in_order(fray, gpu):
    """cornell_box, wantAA: five samples at the AA offsets, K = 3.  50 x 38: partial 8 x 8 tiles on both edges."""
    s = open_scene(fray, "cornell_box.fray", 50, 38, gi=0, wantAA=1, dof=0)
    s.beginRender()
    got, plane, first = _assert_sample_loop(s, 5, 42, lambda i: R.aa_positions(50, 38, i), 3, "cornell AA")
    assert (plane > 0).sum() > 100 and (plane != np.floor(plane)).any()          # pixels on the mirror block's outline: some samples on it, some off
    assert not np.array_equal(got, first)
    s.close()


@pytest.mark.parametrize("seed", [9, 42])
@pytest.mark.parametrize("name", ["cornell_box.fray", "smallpt.fray"])
def test_jittered_samples_are_reduced_in_order(fray, gpu, name, seed):
    """gi frames (words 0 and 8): four samples at the jittered positions of sample_seed(seed, p, i), K = 3"""
    W, H = 48, 36
    s = open_scene(fray, name, W, H, gi=1, numPaths=8, wantAA=0, dof=0)
    s.beginRender()
    pos = lambda i: R.jittered_positions(W, H, i, seed, sample_seed, lambda seeds: jitter(fray, seeds))
    got, plane, first = _assert_sample_loop(s, 4, seed, pos, 3, "%s seed %d" % (name, seed))
    assert (plane > 0).sum() > 50 and not np.array_equal(got, first)
    s.close()


def test_jittered_samples_on_the_csg_word(fray, gpu, tmp_path):
    """csg_nested path-traced (word 2, the variant that spills): four jittered samples whose chains differ in length within a pixel --
    tests/test_specular_ref.py finds such pixels with the CPU oracle at this size and seed"""
    W, H = SC.CSG_GI_SIZE
    s = SC.csg_nested(fray, tmp_path, W, H)
    s.settings.gi, s.settings.numPaths = 1, 8
    assert R.flag_word(s.desc) == 2
    s.beginRender()
    pos = lambda i: R.jittered_positions(W, H, i, SC.CSG_GI_SEED, sample_seed, lambda seeds: jitter(fray, seeds))
    got, plane, first = _assert_sample_loop(s, 4, SC.CSG_GI_SEED, pos, 3, "csg_nested gi")
    assert (plane != np.floor(plane)).sum() >= 10 and (plane > 0).mean() > 0.05
    s.close()


# ---- 4. a bump map in a chain ----------------------------------------------------------------------------------------------------------------------
def test_bumped_mirror_against_the_whitted_frame(fray, gpu, tmp_path):
    """forest.fray in Const paint with the teapot a bump-mapped mirror (tests/specular_cases.forest_bumped), K = 8, maxTraceDepth 12.  The walk
    cannot restate a bumped normal; the Whitted renderer applies it and is pinned to the reference.  In a world of Const paint Whitted's colour of
    a pixel is mult * (mult * (... * c)) with c the Const colour or the environment's at the chain's end, and the frame's albedo ((mult * mult) *
    ...) * c: the same b float32 multiplications per channel in opposite association.  b <= 1: one commutative product, equal bit for bit.
    b >= 2: each side is within (1 + 2^-24)^b of the exact product, so they differ by at most 2.5 b 2^-24 relative (2 b 2^-24 to first order).
    Pixels the limit ended (plane == 8) are left out: there the frame stops at a mirror and Whitted goes on."""
    W, H = SC.BUMP_SIZE
    s, teapot = SC.forest_bumped(fray, tmp_path, W, H)
    assert s.settings.maxTraceDepth == 12 and R.flag_word(s.desc) == 4
    s.beginRender()
    feat, plane = s.render_features_specular(8, 1, bounces=True)
    img, _ = s.render(seed=42)
    hid = s.trace_rays(*s.camera_rays())["hit_id"]
    on = hid == teapot
    assert (on & (plane >= 1)).sum() > 200 and np.array_equal(plane >= 1, on)
    left_out = plane == 8
    assert left_out.sum() <= 0.02 * (plane > 0).sum()
    alb, want = feat[..., 6:9].astype(np.float64), img.astype(np.float64)
    exact = plane <= 1
    assert np.array_equal(feat[exact][:, 6:9], img[exact])
    deep = (plane >= 2) & ~left_out
    bound = 2.5 * plane[deep][:, None] * 2.0 ** -24 * np.abs(want[deep])
    err = np.abs(alb[deep] - want[deep])
    print("bumped mirror: %d pixels with b >= 1, %d with b >= 2 (largest error / bound %.3g), %d left out at the limit"
          % (int((plane >= 1).sum()), int(deep.sum()), float((err / np.maximum(bound, 1e-300)).max()) if deep.any() else 0.0, int(left_out.sum())))
    assert (err <= bound).all()
    # the bump is in the frame: the same call without it has other normals on the teapot, and other chains behind them
    s2, _ = SC.forest_bumped(fray, tmp_path, W, H, bump=False)
    s2.beginRender()
    flat = s2.render_features_specular(8, 1)
    assert not np.array_equal(flat[on][:, 3:6], feat[on][:, 3:6]) and np.array_equal(flat[~on], feat[~on])
    s.close()
    s2.close()
