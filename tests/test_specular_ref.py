"""tests/specular_ref.py and tests/specular_cases.py on the CPU: the oracle-fed walk over every case of tests/test_gpu_features_specular_variants.py
at that file's frame sizes, asserting the conditions the GPU tests rely on -- so that they are established here, by the CPU oracle, and not by the kernel
under test -- and the sample reduction against an example worked by hand."""
import numpy as np
import pytest

import hostlane
import specular_cases as SC
import specular_ref as R
from test_gpu_shade import sample_seed

F32 = np.float32


def oracle_jitter(oracle):
    """the first two randfloat()s of the oracle's generator for each seed (what tests/test_gpu_shade.jitter reads from the device's)"""
    def jitter(seeds):
        out, f = np.empty((len(seeds), 2), F32), np.empty(2, F32)
        for i, sd in enumerate(seeds):
            oracle.lib.fray_oracle_rng_stream(int(sd), 2, f.ctypes.data, None, None, 0)
            out[i] = f
        return out
    return jitter


def oracle_rays(oracle, desc, xy):
    """Camera::getScreenRay through film positions xy [n, 2]"""
    o, d = np.zeros((len(xy), 3)), np.zeros((len(xy), 3))
    so, sd = np.zeros(3), np.zeros(3)
    for i, (x, y) in enumerate(xy):
        oracle.lib.fray_oracle_camera_ray(desc, float(x), float(y), so.ctypes.data, sd.ctypes.data)
        o[i], d[i] = so, sd
    return o, d


def _walk(oracle, s, K, xy=None):
    W, H = s.frame_size
    if xy is None:
        o, d = hostlane.camera_rays(oracle, s.desc, W, H)
    else:
        o, d = oracle_rays(oracle, s.desc, xy.reshape(-1, 2))
    return R.walk_chain(s.desc, o, d, K, R.oracle_trace(oracle, s.desc))


def _first_hit_kinds(desc, ch):
    kinds = np.array([desc.shaders[desc.nodes[i].shader].kind for i in range(desc.n_nodes)])
    f = ch["f_id"]
    return np.where(f >= 0, kinds[np.where(f >= 0, f, 0)], -1)


# ---- the cases of part 3 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES))
def test_case_meets_what_the_gpu_test_relies_on(fray, oracle, tmp_path, name):
    build, size, word, claims = SC.CASES[name]
    s = build(fray, tmp_path, *(size or (None, None)))
    desc = s.desc                                            # (at the GPU test's own frame size: the oracle's per-ray loop takes a second at most)
    assert R.flag_word(desc) == word
    assert all(R.restated_shader(desc, desc.nodes[i].shader) for i in range(desc.n_nodes))       # the albedo rule knows every node's shader
    assert not any(desc.shaders[desc.nodes[i].shader].kind == 3 and desc.shaders[desc.nodes[i].shader].glossiness < 1 for i in range(desc.n_nodes))
    for K in (1, 3, 8):
        ch = _walk(oracle, s, K)
        assert (ch["b"] > 0).mean() > 0.05, (K, (ch["b"] > 0).mean())
        assert ch["b"].max() <= K
        # every albedo is known but the reflected environment's, which only a renderer can give
        assert np.array_equal(~ch["alb_known"], (ch["t_id"] == -1)) if R.has_environment(desc) else ch["alb_known"].all()
        t = SC.terminals(desc, ch)
        fk = _first_hit_kinds(desc, ch)
        for claim in claims:
            if claim == "mir":
                assert (fk == 3).sum() >= 5, (K, claim)
            elif claim == "glass":
                assert (fk == 4).sum() >= 5, (K, claim)
            else:
                assert t[claim].sum() >= 10, (K, claim, int(t[claim].sum()))
        if "light" in claims:                                # ... behind the floor itself, not only behind the scene's own mirror block
            assert (t["light"] & (ch["f_id"] == SC.CORNELL_FLOOR)).sum() >= 10
    s.close()


def test_the_words_of_the_untouched_scenes(fray):
    """The scenes of tests/test_gpu_features_specular.py: cornell_box is word 0, and smallpt -- it declares a texture no shader uses -- word 8
    (its pinned chains run k_features_specular<8> already).  With the cases above every even word has a chain."""
    from conftest import open_scene
    for name, word in (("cornell_box.fray", 0), ("smallpt.fray", 8)):
        s = open_scene(fray, name)
        assert R.flag_word(s.desc) == word
        s.close()
    assert {c[2] for c in SC.CASES.values()} == {0, 2, 4, 8}


# ---- the frames of parts 4 and 5 ------------------------------------------------------------------------------------------------------------------
def test_csg_nested_gi_frame_has_pixels_of_mixed_chain_lengths(fray, oracle, tmp_path):
    """the frame of the GPU test, at its size and seed: four jittered samples, K = 3; some pixels' samples take different numbers of steps"""
    s = SC.csg_nested(fray, tmp_path, *SC.CSG_GI_SIZE)
    W, H = s.frame_size
    jit = oracle_jitter(oracle)
    walks = [_walk(oracle, s, 3, R.jittered_positions(W, H, i, SC.CSG_GI_SEED, sample_seed, jit)) for i in range(4)]
    feat, plane, known = R.reduce_walks(walks)
    assert known.all()
    mixed = plane != np.floor(plane)
    assert mixed.sum() >= 10 and (plane > 0).mean() > 0.05
    s.close()


def test_bumped_forest_shows_enough_teapot(fray, oracle, tmp_path):
    """Part 5's frame, at its size: the camera rays whose first hit is the teapot (which the bump does not move: it changes the normal alone) are
    the pixels with b >= 1 on it.  The share of chains the limit of 8 ends is measured on the unbumped scene here -- the walk applies no bump --
    and asserted on the frame itself by the GPU test."""
    s, teapot = SC.forest_bumped(fray, tmp_path, *SC.BUMP_SIZE, bump=False)
    desc = s.desc
    desc.nodes[next(i for i in range(desc.n_nodes) if desc.nodes[i].bump_tex >= 0)].bump_tex = -1      # (the faceted die's, which changes no normal)
    assert R.flag_word(desc) == 4
    ch = _walk(oracle, s, 8)
    assert (ch["f_id"] == teapot).sum() > 200
    assert ((ch["b"] > 0) == (ch["f_id"] == teapot)).all()
    assert ch["limit"].sum() <= 0.02 * (ch["b"] > 0).sum()
    s.close()


# ---- the reduction ----------------------------------------------------------------------------------------------------------------------------------
def test_reduce_samples_by_hand():
    """a = 2^24, b = 1, c = 1 in float32: (a + b) + c = 2^24 (each 1 is half an ulp of 2^24 and ties go to even), a + (b + c) = 2^24 + 2.
    In sample order the sum is 16777216 and the mean 16777216 / 3 rounded to float32 = 5592405.5 (5592405.333... lies between 5592405 and
    5592405.5, nearer the latter); from the other end it would be 16777218 / 3 = 5592406."""
    a, b, c = F32(2.0 ** 24), F32(1), F32(1)
    assert (a + b) + c != a + (b + c)
    got = R.reduce_samples([np.array([2.0 ** 24]), np.array([1.0]), np.array([1.0])])
    assert got.dtype == F32 and got[0] == F32(5592405.5)
    assert R.reduce_samples([np.array([1.0]), np.array([1.0]), np.array([2.0 ** 24])])[0] == F32(5592406.0)
    # each row is rounded to float32 before it is added: 1 + 2^-30 enters as 1
    assert R.reduce_samples([np.array([1.0 + 2.0 ** -30]), np.array([1.0])])[0] == F32(1)
    # the sum starts from sample 0's row, not from zero (0 + -0 would be +0), and one sample is not divided
    one = R.reduce_samples([np.array([-0.0, 0.1])])
    assert np.signbit(one[0]) and one[1] == F32(0.1)
    assert np.signbit(R.reduce_samples([np.array([-0.0]), np.array([-0.0])])[0])
    # one float32 division by float32(n)
    x = F32(0.7)
    assert R.reduce_samples([np.array([x])] * 5)[0] == ((((x + x) + x) + x) + x) / F32(5)


def test_walk_of_zero_steps_is_the_first_hit_rule(fray, oracle, tmp_path):
    """K = 0: no chain; the rows are the hit records, and a mirror's albedo its mult"""
    s = SC.cornell_floor_mirror(fray, tmp_path, 24, 18)
    desc = s.desc
    o, d = hostlane.camera_rays(oracle, desc, 24, 18)
    ch = R.walk_chain(desc, o, d, 0, R.oracle_trace(oracle, desc))
    ids, rec = hostlane.oracle_probe(oracle, desc, o, d)
    hit = ids != -1
    assert not ch["b"].any() and np.array_equal(ch["t_id"], ids) and np.array_equal(ch["f_id"], ids)
    assert np.array_equal(ch["pos"][hit], rec[hit, 1:4]) and np.array_equal(ch["nrm"][hit], rec[hit, 4:7]) and np.array_equal(ch["depth"][hit], rec[hit, 0])
    assert not ch["pos"][~hit].any() and not ch["depth"][~hit].any()
    floor = ids == SC.CORNELL_FLOOR
    mult = np.array(desc.shaders[desc.nodes[SC.CORNELL_FLOOR].shader].mult[:], F32)
    assert floor.sum() > 50 and ch["limit"][floor].all() and np.array_equal(ch["alb"][floor], np.broadcast_to(mult, (floor.sum(), 3)))
    s.close()
