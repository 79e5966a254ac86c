"""Weighted accumulation and history maps (include/frayhip.h "weighted accumulation and history maps"), what can be checked without a GPU: the
five entries and frayhip_history_map_defaults are exported, declared and mirrored, struct frayhip_history_map's layout and defaults match,
every argument check answers FRAYHIP_E_ARG with the entry's name before the device is touched, the Python side and the CLI refuse what they
should, and the two numpy restatements (tests/temporal_weighted_ref.py, tests/history_map_ref.py) behave as the header says on synthetic inputs."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import change_ref
import history_map_cases as cases
import history_map_ref
import motion_ref
import temporal_ref
import temporal_weighted_ref
from conftest import ROOT
from test_abi import header_functions

ENTRIES = ["frayhip_temporal_accumulate_weighted", "frayhip_temporal_accumulate_weighted_device", "frayhip_history_map_defaults",
           "frayhip_history_map", "frayhip_history_map_device"]
F = np.float32


def test_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    assert callable(fray.history_map) and "history_map" in fray.__all__


def test_struct_and_defaults(fray, abi):
    M = abi.HistoryMap
    assert fray.lib.frayhip_sizeof(b"frayhip_history_map") == C.sizeof(M) == 48
    assert (M.base.offset, M.target.offset, M.max_units.offset, M.reserved.offset, M.budget.offset, M.samples.offset, M.boosted.offset,
            M.target_used.offset, M.pad.offset) == (0, 4, 8, 12, 16, 24, 32, 40, 44)
    assert "frayhip_history_map" not in abi.STRUCTS            # a struct tag without a typedef, as frayhip_denoise
    m = M(base=7, samples=5, boosted=6, target_used=3, reserved=9)
    assert fray.lib.frayhip_history_map_defaults(C.byref(m)) == abi.OK
    assert abi.NO_BUDGET == (1 << 64) - 1
    assert (m.base, m.target, m.max_units, m.reserved, m.budget) == (0, 8, 8, 0, abi.NO_BUDGET)
    assert (m.samples, m.boosted, m.target_used, m.pad) == (0, 0, 0, 0)
    assert fray.lib.frayhip_history_map_defaults(None) == abi.E_ARG
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning
    src = open(os.path.join(ROOT, "include", "frayhip.h")).read()
    assert "struct frayhip_history_map {" in src and "a maintainer's choice, not a measurement" in src


def _buffers(W, H):
    b = dict(rgb=np.zeros((H, W, 3), F), feat=np.zeros((H, W, 10), F), motion=np.zeros((H, W, 8), F), change=np.zeros((H, W), F),
             weight=np.ones((H, W), F), hin=np.zeros((H, W, 12), F), uin=np.zeros((H, W), F), hout=np.zeros((H, W, 12), F),
             uout=np.zeros((H, W), F), sig=np.zeros((H, W, 3), F), var=np.zeros((H, W), F), add=np.zeros((H, W), np.int32),
             wout=np.zeros((H, W), F), held=np.zeros((H, W), F))
    for k in ("motion", "hin", "hout"):
        assert b[k].ctypes.data % 16 == 0
    return b


def _params(L, abi, over):
    prm = abi.Temporal()
    L.frayhip_temporal_defaults(C.byref(prm))
    for k, val in over.items():
        setattr(prm, k, val)
    return prm


def _view(abi, W, H, vw):
    vv = cases.ctypes_view(abi, cases.view(W, H))
    for k, val in (vw or {}).items():
        if k == "pos0":
            vv.pos[0] = val
        else:
            setattr(vv, k, val)
    return vv


@pytest.mark.parametrize("dev", [False, True])
def test_weighted_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    B = _buffers(W, H)
    ptr = {k: v.ctypes.data for k, v in B.items()}
    who = "frayhip_temporal_accumulate_weighted_device" if dev else "frayhip_temporal_accumulate_weighted"

    def call(w=W, h=H, v="view", p="default", vw=None, prm=None, **over):
        a = dict(ptr, **over)
        pp = C.byref(_params(L, abi, prm or {})) if p == "default" else None
        vp = C.byref(_view(abi, W, H, vw)) if v == "view" else None
        args = (w, h, a["rgb"], a["feat"], a["motion"], a["change"], a["weight"], vp, a["hin"], a["uin"], pp, a["hout"], a["uout"], a["sig"], a["var"])
        if dev:
            return L.frayhip_temporal_accumulate_weighted_device(*args, None, None)
        return L.frayhip_temporal_accumulate_weighted(*args, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, rc
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    # the adaptive entry's list
    expect(call(w=0), "width and height")
    expect(call(h=-1), "width and height")
    expect(call(w=1 << 16, h=1 << 15), "2^30")
    expect(call(rgb=None), "null rgb")
    expect(call(feat=None), "null feat")
    expect(call(p=None), "null parameters")
    expect(call(hout=None), "null hist_out")
    expect(call(sig=None), "null signal")
    expect(call(var=None), "null variance")
    expect(call(v=None), "both")
    expect(call(hin=None), "both")
    expect(call(vw=dict(width=W + 1)), "size")
    expect(call(vw=dict(pos0=math.nan)), "non-finite")
    expect(call(vw=dict(tan_y=0.0)), "tan_x and tan_y")
    expect(call(prm=dict(demodulate=2)), "demodulate")
    for n in (0, 4097):
        expect(call(prm=dict(max_history=n)), "max_history")
        expect(call(prm=dict(variance_history=n)), "variance_history")
    for x in (-0.1, 1.5, math.nan):
        expect(call(prm=dict(alpha_min=x)), "alpha_min")
    expect(call(prm=dict(film_offset=math.inf)), "film_offset")
    expect(call(prm=dict(plane_tolerance=-1.0)), "plane_tolerance")
    expect(call(prm=dict(normal_min_dot=math.nan)), "normal_min_dot")
    expect(call(hout=ptr["hin"] + 48), "overlap")
    expect(call(sig=ptr["rgb"]), "overlap")
    expect(call(var=ptr["feat"] + 40), "overlap")
    expect(call(sig=ptr["motion"]), "overlap")
    expect(call(var=ptr["change"]), "overlap")
    expect(call(sig=ptr["hout"] + 16), "overlap")
    # the weight plane and the units planes
    expect(call(weight=None), "null weight")
    expect(call(uout=None), "null units_out")
    expect(call(uin=None), "units_in")
    expect(call(hin=None, v=None), "units_in")
    expect(call(hout=ptr["weight"]), "overlap")
    expect(call(var=ptr["weight"] + 4), "overlap")
    expect(call(sig=ptr["uin"]), "overlap")
    expect(call(uout=ptr["uin"]), "overlap")
    expect(call(uout=ptr["weight"] + 8), "overlap")
    expect(call(uout=ptr["feat"]), "overlap")
    expect(call(uout=ptr["hin"] + 96), "overlap")
    expect(call(uout=ptr["hout"] + 4), "overlap")
    expect(call(uout=ptr["sig"]), "overlap")
    expect(call(uout=ptr["var"]), "overlap")
    if dev:
        expect(call(rgb=ptr["rgb"] + 2), "aligned")
        expect(call(hin=ptr["hin"] + 4), "16-byte")
        expect(call(motion=ptr["motion"] + 8), "16-byte")
        expect(call(weight=ptr["weight"] + 2), "aligned")
        expect(call(uin=ptr["uin"] + 1), "aligned")
        expect(call(uout=ptr["uout"] + 2), "aligned")
        expect(call(change=ptr["change"] + 2), "aligned")


@pytest.mark.parametrize("dev", [False, True])
def test_history_map_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    B = _buffers(W, H)
    ptr = {k: v.ctypes.data for k, v in B.items()}
    who = "frayhip_history_map_device" if dev else "frayhip_history_map"

    def call(w=W, h=H, v="view", p="default", m="default", vw=None, prm=None, mp=None, **over):
        a = dict(ptr, **over)
        pp = C.byref(_params(L, abi, prm or {})) if p == "default" else None
        vp = C.byref(_view(abi, W, H, vw)) if v == "view" else None
        mm = abi.HistoryMap()
        L.frayhip_history_map_defaults(C.byref(mm))
        mm.base = 2
        for k, val in (mp or {}).items():
            setattr(mm, k, val)
        mq = C.byref(mm) if m == "default" else None
        args = (w, h, a["feat"], a["motion"], a["change"], vp, a["hin"], a["uin"], pp, mq, a["add"], a["wout"], a["held"])
        if dev:
            return L.frayhip_history_map_device(*args, None, None)
        return L.frayhip_history_map(*args, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, rc
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    expect(call(w=0), "width and height")
    expect(call(h=-3), "width and height")
    expect(call(w=1 << 16, h=1 << 15), "2^30")
    expect(call(feat=None), "null feat")
    expect(call(p=None), "null parameters")
    expect(call(m=None), "null map")
    expect(call(add=None), "null add")
    expect(call(wout=None), "null weight")
    expect(call(v=None), "all")
    expect(call(hin=None), "all")
    expect(call(uin=None), "all")
    expect(call(hin=None, uin=None), "all")
    expect(call(vw=dict(height=H + 1)), "size")
    expect(call(vw=dict(tan_x=math.inf)), "non-finite")
    expect(call(prm=dict(max_history=0)), "max_history")
    expect(call(prm=dict(film_offset=math.nan)), "film_offset")
    expect(call(prm=dict(normal_min_dot=2.0)), "normal_min_dot")
    expect(call(mp=dict(base=0)), "base")
    expect(call(mp=dict(target=0)), "target")
    expect(call(mp=dict(target=33)), "target")
    expect(call(mp=dict(target=5), prm=dict(max_history=4)), "target")
    expect(call(mp=dict(max_units=0)), "max_units")
    expect(call(mp=dict(base=1 << 21, max_units=9)), "2^24")
    expect(call(mp=dict(reserved=1)), "reserved")
    expect(call(mp=dict(budget=2 * W * H - 1)), "budget")
    expect(call(mp=dict(budget=0)), "budget")
    expect(call(add=ptr["feat"]), "overlap")
    expect(call(add=ptr["uin"]), "overlap")
    expect(call(wout=ptr["hin"] + 100), "overlap")
    expect(call(wout=ptr["motion"]), "overlap")
    expect(call(held=ptr["change"] + 4), "overlap")
    expect(call(wout=ptr["add"]), "overlap")
    expect(call(held=ptr["add"] + 8), "overlap")
    expect(call(held=ptr["wout"]), "overlap")
    if dev:
        expect(call(feat=ptr["feat"] + 2), "aligned")
        expect(call(hin=ptr["hin"] + 8), "16-byte")
        expect(call(motion=ptr["motion"] + 4), "16-byte")
        expect(call(uin=ptr["uin"] + 2), "aligned")
        expect(call(add=ptr["add"] + 1), "aligned")
        expect(call(wout=ptr["wout"] + 2), "aligned")
        expect(call(held=ptr["held"] + 3), "aligned")


def test_python_side_refuses_bad_inputs(fray, abi):
    rgb, feat = np.zeros((4, 5, 3), F), np.zeros((4, 5, 10), F)
    hist, plane = np.zeros((4, 5, 12), F), np.ones((4, 5), F)
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    view = fray.view_from_camera(s.camera, 5, 4)
    # a later frame (hist_in given) with weight but without its units plane, and the reverse
    with pytest.raises(ValueError, match="units_in"):
        fray.temporal_accumulate(rgb, feat, view, hist, weight=plane)
    with pytest.raises(ValueError, match="units_in"):
        fray.temporal_accumulate(rgb, feat, weight=plane, units_in=plane)
    with pytest.raises(ValueError, match="weight"):
        fray.temporal_accumulate(rgb, feat, view, hist, units_in=plane)
    with pytest.raises(ValueError):
        fray.temporal_accumulate(rgb, feat, weight=plane[:, :4])
    with pytest.raises(ValueError, match="base"):
        fray.history_map(feat)
    with pytest.raises(ValueError, match="all"):
        fray.history_map(feat, view, hist, base=2)
    with pytest.raises(ValueError, match="all"):
        fray.history_map(feat, None, hist, plane, base=2)
    with pytest.raises(TypeError):
        fray.history_map(feat, s.camera, hist, plane, base=2)
    with pytest.raises(TypeError):
        fray.history_map(feat, base=2, history=3)
    with pytest.raises(TypeError):
        fray.history_map(feat, base=2, budget=1.5)
    with pytest.raises(ValueError):
        fray.history_map(feat, view, hist, plane[:3], base=2)
    with pytest.raises(fray.FrayError, match="target"):
        fray.history_map(feat, base=2, target=33)
    with pytest.raises(fray.FrayError, match="budget"):
        fray.history_map(feat, base=2, budget=39)
    if "torch" in sys.modules:
        import torch
        with pytest.raises(TypeError, match="mix"):
            fray.history_map(torch.zeros(4, 5, 10), view, hist, plane, base=2)
        with pytest.raises(TypeError, match="mix"):
            fray.temporal_accumulate(rgb, feat, weight=torch.ones(4, 5))
        with pytest.raises(TypeError, match="CPU tensor"):
            fray.history_map(torch.zeros(4, 5, 10), base=2)
    # the sequence: refused from the arguments alone, before the device is asked for
    with pytest.raises(ValueError, match="split"):
        next(s.render_sequence([s.camera], split=True, boost=dict(target=4)))
    with pytest.raises(TypeError, match="units"):
        next(s.render_sequence([s.camera], boost=dict(target=4, units=2)))
    with pytest.raises(fray.FrayError, match="beginRender"):
        next(s.render_sequence([s.camera], boost=dict(target=4)))
    s.close()


def test_cli_lists_the_boost_flags():
    env = dict(os.environ, FRAYHIP_NO_TORCH="1")
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr
    for flag in ("--boost", "--boost-max", "--sample-budget"):
        assert flag in out.stdout, flag
    from fray_amd.__main__ import build_parser, check_args
    ap = build_parser()
    a = ap.parse_args(["scene.fray", "--denoise", "--frames", "8", "--boost", "6", "--boost-max", "4", "--sample-budget", "100000"])
    check_args(ap, a)
    assert (a.boost, a.boost_max, a.sample_budget) == (6, 4, 100000)
    for argv, words in ((["--boost", "4"], "--boost needs --denoise --frames"),
                        (["--denoise", "--frames", "3", "--boost", "4", "--split"], "--boost cannot be combined"),
                        (["--denoise", "--refine", "0.1", "--max-spp", "64", "--boost", "4"], "--boost cannot be combined"),
                        (["--denoise", "--frames", "3", "--boost", "0"], "--boost: T must be"),
                        (["--denoise", "--frames", "3", "--boost-max", "2"], "--boost-max needs --boost"),
                        (["--denoise", "--frames", "3", "--sample-budget", "5"], "--sample-budget needs --refine")):
        # refused before the scene is read: the scene file need not exist
        r = subprocess.run([sys.executable, "-m", "fray_amd", "missing.fray"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 2 and words in r.stderr, (argv, r.stderr)


# ---- the restatements on synthetic inputs --------------------------------------------------------------------------------------------------------

def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("W,H", cases.SIZES)
def test_weighted_restatement_with_ones_is_the_unweighted_one(W, H):
    (rgb0, feat0, v0), (rgb1, feat1, v1) = cases.pair(W, H, seed=3)
    ones = np.ones((H, W), F)
    mot = cases.motion_frame(feat1)
    rng = np.random.default_rng(5)
    chg = rng.choice(np.array([0.0, -0.0, 0.25, 0.7, 1.0, math.nan], F), (H, W))
    h0, u0, s0, q0 = temporal_weighted_ref.accumulate(rgb0, feat0, ones)
    r0 = temporal_ref.accumulate(rgb0, feat0)
    assert _same_bits(h0, r0[0]) and _same_bits(s0, r0[1]) and _same_bits(q0, r0[2]) and _same_bits(u0, h0[..., 3]) and np.all(u0 == 1)
    # a history some frames deep, so that N is not 1 everywhere: three more frames of the first view
    for k in range(3):
        h0 = temporal_ref.accumulate(cases.frame(W, H, 0.0, seed=10 + k)[0], feat0, v0, h0)[0]
    N0 = h0[..., 3].copy()
    found = 0
    for name, want, kw in (("plain", temporal_ref.accumulate(rgb1, feat1, v0, h0), {}),
                           ("motion", motion_ref.accumulate(rgb1, feat1, mot, v0, h0), dict(motion=mot)),
                           ("change", change_ref.accumulate(rgb1, feat1, chg, None, v0, h0), dict(change=chg)),
                           ("motion+change", change_ref.accumulate(rgb1, feat1, chg, mot, v0, h0), dict(motion=mot, change=chg))):
        h, u, s, q = temporal_weighted_ref.accumulate(rgb1, feat1, ones, prev_view=v0, hist_in=h0, units_in=N0, **kw)
        assert _same_bits(h, want[0]) and _same_bits(s, want[1]) and _same_bits(q, want[2]), name
        assert _same_bits(u, h[..., 3]), name
        found += int((h[..., 3] > 1).sum())
    assert found > 0 or W * H == 1


def test_weighted_restatement_units_bounds_and_running_weighted_mean():
    W, H = 37, 29
    (rgb0, feat0, v0), (rgb1, feat1, v1) = cases.pair(W, H, seed=7)
    rng = np.random.default_rng(9)
    for mh in (1, 4, 32):
        w0 = rng.choice(np.array([math.nan, 0.0, -0.0, -3.0, 0.5, 1.0, 3.0, mh, 2 * mh, math.inf], F), (H, W))
        w1 = rng.uniform(0.0, 2.0 * mh, (H, W)).astype(F)
        h0, u0, _, _ = temporal_weighted_ref.accumulate(rgb0, feat0, w0, max_history=mh)
        c0 = temporal_weighted_ref.clean_weight(w0, mh)
        assert _same_bits(u0, c0) and np.all(h0[..., 3] == 1)
        h1, u1, _, _ = temporal_weighted_ref.accumulate(rgb1, feat1, w1, prev_view=v0, hist_in=h0, units_in=u0, max_history=mh)
        c1 = temporal_weighted_ref.clean_weight(w1, mh)
        assert np.all(u1 <= mh) and np.all(u1 >= np.minimum(c1, F(mh))) and np.all(c1 >= 1) and np.all(c1 <= mh)
        assert np.all((h1[..., 3] >= 1) & (h1[..., 3] <= mh))
    # what the weight is for: 8 units of value a, then 1 unit of value b, is the weighted mean (8 a + b) / 9, not the frame mean (a + b) / 2
    feat, v = feat0, v0
    a, b = np.full((H, W, 3), 0.9, F), np.full((H, W, 3), 0.0, F)
    h, u, _, _ = temporal_weighted_ref.accumulate(a, feat, np.full((H, W), 8, F), demodulate=0, alpha_min=0.0)
    h, u, sig, _ = temporal_weighted_ref.accumulate(b, feat, np.ones((H, W), F), prev_view=v, hist_in=h, units_in=u, demodulate=0, alpha_min=0.0)
    hit = h[..., 3] > 1
    # N and U are fetched like the colour, sum(b x_q) / sum(b): a few FP32 roundings away from the integers
    assert hit.any() and np.abs(h[..., 3][hit] - 2).max() <= 1e-5 and np.abs(u[hit] - 9).max() <= 1e-5
    assert np.abs(sig[hit] - 0.8).max() <= 1e-5


@pytest.mark.parametrize("W,H", cases.SIZES)
def test_map_restatement_properties(W, H):
    (rgb0, feat0, v0), (rgb1, feat1, v1) = cases.pair(W, H, seed=1)
    h0 = temporal_ref.accumulate(rgb0, feat0)[0]
    n = W * H
    rng = np.random.default_rng(2)
    units = rng.uniform(0.0, 12.0, (H, W)).astype(F)
    base, target, mu = 3, 8, 5
    # first frame: nothing held, every pixel asks for min(target, max_units) units
    add, weight, held, info = history_map_ref.history_map(feat0, base=base, target=target, max_units=mu)
    assert np.all(held == 0) and np.all(add == base * mu) and np.all(weight == mu) and info == dict(target_used=target, samples=base * mu * n, boosted=n)
    hp = history_map_ref.held(feat1, v0, h0, units)
    k = history_map_ref.whole_units(hp, 32)
    assert np.all(hp >= 0) and np.all((k >= 0) & (k <= 32))
    S = [history_map_ref.total(k, t, base, mu) for t in range(1, 33)]
    assert all(a <= b for a, b in zip(S, S[1:])) and S[0] == base * n
    for budget in (None, S[target - 1], (S[0] + S[target - 1]) // 2, S[0]):
        add, weight, held, info = history_map_ref.history_map(feat1, v0, h0, units, base=base, target=target, max_units=mu, budget=budget)
        assert _same_bits(held, hp) and np.array_equal(add, (base * weight).astype(np.int32)) and info["samples"] == int(add.sum())
        assert np.all((weight >= 1) & (weight <= mu)) and info["boosted"] == int((weight > 1).sum())
        t = info["target_used"]
        if budget is None or S[target - 1] <= budget:
            assert t == target
        else:
            assert info["samples"] <= budget and t < target and S[t] > budget          # S[t] is S(t + 1)
        if budget == S[0]:
            assert np.all(weight == 1) and (t == 1 or S[t - 1] == S[0])
    # a change frame: 1 (and NaN) drops what is held, a part scales it, 0 leaves it
    for g, want in ((1.0, np.zeros_like(hp)), (math.nan, np.zeros_like(hp)), (0.0, hp), (-0.0, hp), (0.25, (hp * F(0.75)).astype(F))):
        got = history_map_ref.held(feat1, v0, h0, units, change=np.full((H, W), g, F))
        assert _same_bits(got, np.where(hp > 0, want, hp)), g
    # NaN and negative units are held as nothing
    bad = units.copy()
    bad[::2] = math.nan
    bad[1::2] = -4.0
    assert np.all(history_map_ref.held(feat1, v0, h0, bad) == 0)
