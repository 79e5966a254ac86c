"""Weighted accumulation and history maps on the GPU (include/frayhip.h "weighted accumulation and history maps"), every comparison bit for bit:
1. the weighted entry with a weight of ones and units_in = N against the existing entries (plain, motion, change, motion + change);
2. the weighted entry against tests/temporal_weighted_ref.py with adversarial weights and change values, two chained frames;
3. the history map against tests/history_map_ref.py: first frame, one bin, random units, max_history 1 and 4096, three budgets;
4. the map's held is the weighted entry's own fetch;
5. the map is deterministic, also across streams;
6. Scene.render_sequence(boost=dict(target=1, max_units=1)) is the boost=None sequence;
7. a boosted sequence: counts = spp * weight, raw obeys the sample-map contract, the budget holds and the target is the restatement's;
8. with a moved light and change_samples=1 the pixels whose change is 1 get max_units.
The scene-free tests use the synthetic frames of tests/history_map_cases.py; the sequences cornell_box at 64 x 48, 2 spp, 3 frames."""
import math

import numpy as np
import pytest

import history_map_cases as cases
import history_map_ref
import scene_edits
import temporal_weighted_ref
from conftest import open_scene

pytestmark = pytest.mark.gpu
F = np.float32
MODES = ("plain", "motion", "change", "motion+change")


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _same(what, got, ref):
    """Equal in every bit (NaNs of the same bits included), with the first differing value in the message."""
    got, ref = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(ref))
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    a, b = got.view(np.uint32), ref.view(np.uint32)
    if np.array_equal(a, b):
        return
    bad = np.argwhere(a != b)
    i = tuple(bad[0])
    raise AssertionError("%s: %d of %d values differ, first at %s: library %r, expected %r" % (what, len(bad), got.size, i, got[i], ref[i]))


def _to(dev, *arrays):
    """The arrays as they are (host entry) or as GPU tensors (device entry); None stays None."""
    if not dev:
        return arrays
    import torch
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _inputs(fray, abi, W, H, seed):
    """Two frames of the synthetic world and a history of the first view that is four frames deep (N is not 1 everywhere): a dict."""
    (rgb0, feat0, v0), (rgb1, feat1, v1) = cases.pair(W, H, seed=seed)
    view0 = cases.ctypes_view(abi, v0)
    hist = fray.temporal_accumulate(rgb0, feat0)[0]
    for k in range(3):
        hist = fray.temporal_accumulate(cases.frame(W, H, 0.0, seed=seed + 10 + k)[0], feat0, view0, hist)[0]
    rng = np.random.default_rng(seed + 1)
    chg = rng.choice(np.array([0.0, -0.0, 0.25, 1.0, math.nan], F), (H, W))
    return dict(rgb0=rgb0, feat0=feat0, rgb1=rgb1, feat1=feat1, v0=v0, view0=view0, hist=hist, motion=cases.motion_frame(feat1), change=chg)


def _mode(I, mode):
    return dict(motion=I["motion"] if "motion" in mode else None, change=I["change"] if "change" in mode else None)


# ---- 1. a weight of ones is the existing entries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("W,H", cases.SIZES)
def test_weight_of_ones_is_the_existing_entries(fray, abi, gpu, W, H, dev):
    I = _inputs(fray, abi, W, H, 3)
    ones = np.ones((H, W), F)
    N_in = np.ascontiguousarray(I["hist"][..., 3])
    deep = 0
    for mode in MODES:
        m = _mode(I, mode)
        rgb, feat, hist, units, ones_d, mot, chg = _to(dev, I["rgb1"], I["feat1"], I["hist"], N_in, ones, m["motion"], m["change"])
        want = fray.temporal_accumulate(rgb, feat, I["view0"], hist, motion=mot, change=chg)
        got = fray.temporal_accumulate(rgb, feat, I["view0"], hist, motion=mot, change=chg, weight=ones_d, units_in=units)
        assert len(got) == 4
        _same(mode + " hist_out", got[0], want[0])
        _same(mode + " signal", got[2], want[1])
        _same(mode + " variance", got[3], want[2])
        _same(mode + " units_out against N", got[1], _np(got[0])[..., 3])
        deep += int((_np(got[0])[..., 3] > 1).sum())
        # the first frame
        want = fray.temporal_accumulate(rgb, feat, motion=mot, change=chg)
        got = fray.temporal_accumulate(rgb, feat, motion=mot, change=chg, weight=ones_d)
        for k, (a, b) in enumerate(((got[0], want[0]), (got[2], want[1]), (got[3], want[2]), (got[1], _np(got[0])[..., 3]))):
            _same("%s first frame output %d" % (mode, k), a, b)
    assert deep > 0                                     # some pixel of every size fetched a history


# ---- 2. adversarial weights against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("W,H", cases.SIZES)
def test_weighted_matches_restatement(fray, abi, gpu, W, H, dev):
    I = _inputs(fray, abi, W, H, 5)
    rng = np.random.default_rng(17)
    for mh in (32, 4):
        values = np.array([math.nan, 0.0, -0.0, -3.0, 0.5, 1.0, 3.0, mh, 2 * mh, math.inf], F)
        w0, w1 = rng.choice(values, (H, W)), rng.choice(values, (H, W))
        prm = dict(max_history=mh)
        # frame 1: no history; frame 2 takes frame 1's outputs
        rgb0, feat0, w0_d = _to(dev, I["rgb0"], I["feat0"], w0)
        got0 = fray.temporal_accumulate(rgb0, feat0, weight=w0_d, **prm)
        ref0 = temporal_weighted_ref.accumulate(I["rgb0"], I["feat0"], w0, **prm)
        for name, a, b in zip(("hist_out", "units_out", "signal", "variance"), got0, ref0):
            _same("max_history %d frame 1 %s" % (mh, name), a, b)
        for mode in MODES:
            m = _mode(I, mode)
            rgb1, feat1, w1_d, mot, chg = _to(dev, I["rgb1"], I["feat1"], w1, m["motion"], m["change"])
            got = fray.temporal_accumulate(rgb1, feat1, I["view0"], got0[0], motion=mot, change=chg, weight=w1_d, units_in=got0[1], **prm)
            ref = temporal_weighted_ref.accumulate(I["rgb1"], I["feat1"], w1, motion=m["motion"], change=m["change"], prev_view=I["v0"],
                                                   hist_in=ref0[0], units_in=ref0[1], **prm)
            for name, a, b in zip(("hist_out", "units_out", "signal", "variance"), got, ref):
                _same("max_history %d %s frame 2 %s" % (mh, mode, name), a, b)
            u = _np(got[1])
            assert np.all(u <= mh) and np.all(u >= 1)


# ---- 3. the map against the restatement ------------------------------------------------------------------------------------------------------------
def _map_both(fray, dev, I, units, motion=None, change=None, **kw):
    """fray.history_map on frame 2 of the inputs (hist_in, units) against the restatement: all six results equal.  Returns the restatement's."""
    feat, hist, u, mot, chg = _to(dev, I["feat1"], I["hist"] if units is not None else None, units, motion, change)
    view = I["view0"] if units is not None else None
    add, weight, info = fray.history_map(feat, view, hist, u, motion=mot, change=chg, held=True, **kw)
    r_add, r_weight, r_held, r_info = history_map_ref.history_map(I["feat1"], I["v0"] if units is not None else None,
                                                                  I["hist"] if units is not None else None, units, motion=motion, change=change, **kw)
    _same("held", info["held"], r_held)
    _same("add", add, r_add)
    _same("weight", weight, r_weight)
    assert {k: info[k] for k in ("target_used", "samples", "boosted")} == r_info, (info, r_info)
    assert info["budget"] == kw.get("budget") and _np(add).dtype == np.int32
    return r_add, r_weight, r_held, r_info


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("W,H", cases.SIZES)
def test_history_map_matches_restatement(fray, abi, gpu, W, H, dev):
    I = _inputs(fray, abi, W, H, 7)
    n = W * H
    rng = np.random.default_rng(23)
    # first frame: nothing is held
    _, _, held, info = _map_both(fray, dev, I, None, base=2, target=6, max_units=4)
    assert not held.any() and info == dict(target_used=6, samples=2 * 4 * n, boosted=n)
    # every pixel in one bin (k = 0: half a unit where a history is fetched, nothing elsewhere): the contention case
    _, weight, held, info = _map_both(fray, dev, I, np.full((H, W), 0.5, F), base=3, target=8, max_units=8)
    assert held.max() < 1 and np.all(weight == 8) and info["boosted"] == n
    for mh, target, mu in ((32, 8, 8), (32, 32, 5), (1, 1, 3), (4096, 4096, 8), (4096, 600, 4096)):
        units = rng.uniform(0.0, 2.0 * mh, (H, W)).astype(F)
        bad = rng.uniform(size=(H, W))
        units[bad < 0.05] = math.nan
        units[(bad >= 0.05) & (bad < 0.1)] = -rng.uniform(0.0, 5.0)
        for mode in ("plain", "motion+change"):
            kw = dict(_mode(I, mode), base=2, target=target, max_units=mu, max_history=mh)
            _, _, held, free = _map_both(fray, dev, I, units, **kw)
            assert np.all(held >= 0)
            k = history_map_ref.whole_units(held, mh)
            S1, St = history_map_ref.total(k, 1, 2, mu), history_map_ref.total(k, target, 2, mu)
            assert free["target_used"] == target and free["samples"] == St and S1 == 2 * n
            # a budget that binds in the middle: from the restatement alone, before the library is asked
            middle = (S1 + St) // 2
            binds = St > middle
            _, _, _, info = _map_both(fray, dev, I, units, budget=middle, **kw)
            assert info["samples"] <= middle and (info["target_used"] < target) == binds
            if (W, H) == cases.SIZES[0] and mh > 1 and mode == "plain":
                assert binds and info["target_used"] < target           # the inputs were chosen so that it does
            # exactly one unit a pixel
            _, weight, _, info = _map_both(fray, dev, I, units, budget=S1, **kw)
            assert np.all(weight == 1) and info["samples"] == S1 and info["boosted"] == 0


# ---- 4. the map's held is the accumulation's fetch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", cases.SIZES)
def test_held_is_the_weighted_fetch(fray, abi, gpu, W, H):
    I = _inputs(fray, abi, W, H, 9)
    units = np.random.default_rng(31).uniform(0.0, 40.0, (H, W)).astype(F)
    ones = np.ones((H, W), F)
    fetched = 0
    for mode in ("plain", "motion"):
        m = _mode(I, mode)
        for mh in (32, 8):
            _, _, info = fray.history_map(I["feat1"], I["view0"], I["hist"], units, motion=m["motion"], base=1, held=True, max_history=mh)
            hist, u, _, _ = fray.temporal_accumulate(I["rgb1"], I["feat1"], I["view0"], I["hist"], motion=m["motion"], weight=ones, units_in=units,
                                                     max_history=mh)
            # where no history is fetched held is 0 and units_out is the weight, 1: the same expression covers both
            _same("%s max_history %d" % (mode, mh), u, np.fmin(info["held"] + F(1), F(mh)).astype(F))
            fetched += int((info["held"] > 0).sum())
    assert fetched > 0


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------------------------
def test_history_map_is_deterministic(fray, abi, gpu):
    import torch
    W, H = cases.SIZES[0]
    I = _inputs(fray, abi, W, H, 11)
    units = np.random.default_rng(37).uniform(0.0, 64.0, (H, W)).astype(F)
    feat, hist, u, mot, chg = _to(True, I["feat1"], I["hist"], units, I["motion"], I["change"])
    budget = 2 * W * H * 2
    kw = dict(motion=mot, change=chg, base=2, target=8, max_units=8, budget=budget, held=True)
    first = fray.history_map(feat, I["view0"], hist, u, **kw)
    want = history_map_ref.history_map(I["feat1"], I["v0"], I["hist"], units, motion=I["motion"], change=I["change"], base=2, target=8, max_units=8,
                                       budget=budget)[3]
    assert {k: first[2][k] for k in want} == want
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for stream in (None, side):
        again = fray.history_map(feat, I["view0"], hist, u, stream=stream, **kw)
        _same("add", again[0], first[0])
        _same("weight", again[1], first[1])
        _same("held", again[2]["held"], first[2]["held"])
        assert {k: v for k, v in again[2].items() if k != "held"} == {k: v for k, v in first[2].items() if k != "held"}
    torch.cuda.current_stream().wait_stream(side)
    assert first[2]["target_used"] < 8                  # the budget binds: the select kernel's search ran


# ---- 6-8. sequences ---------------------------------------------------------------------------------------------------------------------------------
W3, H3, SPP, SEED, FRAMES = 64, 48, 2, 21, 3
YAW = 6.0                                               # degrees a frame: a strip of new wall enters, most pixels keep their history


def _cams(abi, s, yaw_step=YAW):
    out = []
    for k in range(FRAMES):
        c = abi.Camera.from_buffer_copy(s.camera)
        c.yaw += yaw_step * k
        out.append(c)
    return out


def _open(fray):
    s = open_scene(fray, "cornell_box.fray", W3, H3, numPaths=SPP)
    s.beginRender()
    return s


def test_sequence_boost_of_one_unit_is_the_plain_sequence(fray, abi, gpu):
    s = _open(fray)
    cams = _cams(abi, s)
    plain = [(_np(o), _np(r), _np(i["history"])) for o, r, i in s.render_sequence(cams, seed=SEED, feature_samples=2)]
    for k, (out, raw, info) in enumerate(s.render_sequence(cams, seed=SEED, feature_samples=2, boost=dict(target=1, max_units=1))):
        assert out.is_cuda and raw.is_cuda and info["units"].is_cuda and info["counts"].is_cuda and info["weight"].is_cuda
        _same("frame %d out" % k, out, plain[k][0])
        _same("frame %d raw" % k, raw, plain[k][1])
        _same("frame %d history" % k, info["history"], plain[k][2])
        _same("frame %d units against N" % k, info["units"], plain[k][2][..., 3])
        assert info["boost"] == dict(target_used=1, samples=W3 * H3 * SPP, boosted=0, budget=None)
        assert bool((info["counts"] == SPP).all()) and bool((info["weight"] == 1).all())
    assert k == FRAMES - 1
    s.close()


def _check_counts(s, k, raw, info, n_max):
    """counts = spp * weight, and every pixel of raw is that pixel of the uniform frame at its count (at most n_max distinct counts)."""
    counts, weight = _np(info["counts"]), _np(info["weight"])
    assert counts.dtype == np.int32 and np.array_equal(counts, (SPP * weight).astype(np.int32))
    distinct = np.unique(counts)
    assert 1 <= len(distinct) <= n_max and distinct.min() >= SPP
    raw = _np(raw)
    for c in distinct:
        uniform, _ = s.render_samples(int(c), seed=SEED + k)         # the scene's camera is frame k's while the generator is suspended
        at = counts == c
        assert np.array_equal(raw[at].view(np.uint32), uniform[at].view(np.uint32)), (k, int(c))
    return counts


def test_sequence_boost_spends_samples_where_history_is_short(fray, abi, gpu):
    s = _open(fray)
    cams = _cams(abi, s)
    n = W3 * H3
    prev = None
    for k, (out, raw, info) in enumerate(s.render_sequence(cams, seed=SEED, feature_samples=2, boost=dict(target=4, max_units=4))):
        counts = _check_counts(s, k, raw, info, 4)
        b = info["boost"]
        assert b["samples"] == int(counts.sum()) and b["boosted"] == int((counts > SPP).sum()) and b["target_used"] == 4
        if k == 0:
            assert bool((counts == 4 * SPP).all())
        if k == 1:
            # both classes: pixels that found four units of history get one unit, pixels that entered the view get four
            assert 0 < b["boosted"] < n and (counts == SPP).any() and (counts == 4 * SPP).any()
        units, hist = _np(info["units"]), _np(info["history"])
        # N counts frames whatever the weight (a bilinear fetch leaves it a few roundings off the integer), the units hold at least this frame's
        assert np.all(units <= 32) and np.all(units >= _np(info["weight"])) and np.all(hist[..., 3] <= (k + 1) * (1 + 1e-6))
    assert k == FRAMES - 1
    # under a budget of two base frames: the budget holds, and the target is the restatement's from the frame's own held
    budget = n * SPP * 2
    prev = None
    lowered = 0
    for k, (out, raw, info) in enumerate(s.render_sequence(cams, seed=SEED, feature_samples=2, boost=dict(target=4, max_units=4, budget=budget))):
        counts = _check_counts(s, k, raw, info, 4)
        b = info["boost"]
        assert b["samples"] == int(counts.sum()) <= budget and b["budget"] == budget
        if prev is None:
            held = np.zeros((H3, W3), F)
        else:
            held = _np(fray.history_map(info["features_frame"], prev["view"], prev["history"], prev["units"], base=SPP, target=4, max_units=4,
                                        held=True, film_offset=info["film_offset"])[2]["held"])
        kk = history_map_ref.whole_units(held, 32)
        want = max(t for t in range(1, 5) if history_map_ref.total(kk, t, SPP, 4) <= budget)
        assert b["target_used"] == want, (k, b, want)
        lowered += int(want < 4)
        prev = info
    assert lowered > 0                                   # frame 0 holds nothing and would ask for four units everywhere: the budget binds there
    s.close()


def test_sequence_boost_under_a_moved_light(fray, abi, gpu):
    s = _open(fray)
    cam = abi.Camera.from_buffer_copy(s.camera)

    def edit(k, scene):
        if k == 1:
            scene_edits.apply(fray, scene, scene_edits.CASES["cornell-light"]["edit"])
            scene.update()
    dropped = 0
    # gain 8: one probe sample a pixel leaves most windows with a ratio below 1; the gain lifts a good share of them to exactly 1
    for k, (out, raw, info) in enumerate(s.render_sequence([cam] * FRAMES, seed=SEED, feature_samples=2, edit=edit, change_samples=1,
                                                           change=dict(gain=8.0), boost=dict(target=4, max_units=4))):
        counts = _check_counts(s, k, raw, info, 4)
        if k == 0:
            assert info["change"] is None
            continue
        chg = _np(info["change"])
        full = chg >= 1
        assert np.all(counts[full] == 4 * SPP)           # nothing held there: target - 0 units, capped at max_units
        assert np.all(_np(info["history"])[..., 3][full] == 1)
        if k == 1:
            dropped = int(full.sum())
        else:
            assert not chg.any()                         # the light moved once
    assert dropped > 0
    s.close()
