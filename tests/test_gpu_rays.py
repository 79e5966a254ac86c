"""Ray queries on the GPU (include/frayhip.h "ray queries"): rays and segments the caller chooses, against the reference's own probe records
(tests/golden/ref_*.npz, tests/golden/generated/*.npz: camera rays and incoherent secondary rays with oracle/_ref's closestHit record), the CPU
oracle, MODE_PRIMARY_ID frames, and the documented answers for degenerate input."""
import ctypes as C
import math
import os
import pathlib

import numpy as np
import pytest

from conftest import ROOT, open_scene
from test_fuzz_parity import random_scene
from test_oracle_vs_ref import FIXTURES, load_case
from test_oracle_vs_ref_fuzz import FAN_SEEDS, SEEDS, ref_fixture, scene_digest

pytestmark = pytest.mark.gpu

GENERATED = [("fz%d_%d" % (s, g), s, False) for s in SEEDS for g in (s % 2, 1 - s % 2)] + [("fans%d" % s, s, True) for s in FAN_SEEDS]
# The device's atan2 / asin are not glibc's bit for bit.  Their difference of an ulp or two reaches u = (atan2(..) / PI * 180 + 180) / 360 through a sum
# of magnitude up to 360, so it is bounded in ulps of the scale of u, v (1.0, 2^-52), not of u itself: near u = 0 that sum cancels, and one ulp of the
# angle is dozens of ulps of a small u.
SPHERE_UV_ULPS = 4


def _generated_case(fray, tmp_path, name, seed, fans):
    gi = 0 if fans else seed % 2
    scene = random_scene(np.random.default_rng(seed), pathlib.Path(tmp_path), gi, flavour=seed % 3, bump_on=("blob",), fans=fans)
    digest = scene_digest(tmp_path)
    s = fray.Scene.parseScene(scene)
    z = ref_fixture(scene, name, s.settings.frameWidth, s.settings.frameHeight, "gi=%d" % (int(name[-1]) if not fans else 0), tmp_path, digest)
    assert (s.settings.frameWidth, s.settings.frameHeight) == (int(z["W"]), int(z["H"]))
    return z, s


def _has_sphere(desc, g, depth=0):
    """Does geometry g (a leaf, or a CsgOp tree) contain a sphere?"""
    ref = desc.geoms[g]
    if ref.kind == 1:
        return True
    if ref.kind == 4 and depth < 16:
        c = desc.csgs[ref.index]
        return _has_sphere(desc, c.left, depth + 1) or _has_sphere(desc, c.right, depth + 1)
    return False


def _check_records(s, z, hid, rec, label):
    """hid / rec (the device's) against the fixture's reference records; returns the number of sphere u, v that differ."""
    want_id, want = z["hit_id"], z["hit_rec"]
    assert np.array_equal(hid, want_id), (label, np.argwhere(hid != want_id)[:5].ravel())
    miss, light, node = want_id == -1, want_id <= -2, want_id >= 0
    assert (rec[miss, 0] == 1e99).all() and (want[miss, 0] == 1e99).all() and (rec[miss, 1:] == 0).all(), label
    assert np.array_equal(rec[light, :7], want[light, :7]), label
    assert (rec[light, 7:] == 0).all(), label
    assert np.array_equal(rec[node, :7], want[node, :7]), (label, np.argwhere((rec[node, :7] != want[node, :7]).any(axis=1))[:5].ravel())
    uv_diff = (rec[:, 7:] != want[:, 7:]).any(axis=1) & node
    sphere = np.array([i >= 0 and _has_sphere(s.desc, s.desc.nodes[int(i)].geom) for i in want_id], bool)
    assert not (uv_diff & ~sphere).any(), (label, "u, v differ on a winner without a sphere", np.argwhere(uv_diff & ~sphere)[:5].ravel())
    if uv_diff.any():
        assert np.abs(rec[uv_diff, 7:] - want[uv_diff, 7:]).max() <= SPHERE_UV_ULPS * 2.0 ** -52, label
    return int(uv_diff.sum())


def _records_three_ways(torch, s, z):
    """hit records of the fixture's rays: host entry, device entry on a non-default stream, host entry with the counting kernels"""
    S, D = np.ascontiguousarray(z["ray_start"]), np.ascontiguousarray(z["ray_dir"])
    h = s.trace_rays(S, D, record=True)
    stream = torch.cuda.Stream()
    d = s.trace_rays(torch.from_numpy(S).cuda(), torch.from_numpy(D).cuda(), record=True, stream=stream)
    c = s.trace_rays(S, D, record=True, stats=True)
    for k in ("hit_id", "hit_dist", "hit_rec"):
        assert np.array_equal(h[k], d[k].cpu().numpy()), k                    # host and device entries: one code path
        assert np.array_equal(h[k], c[k]), k                                    # the counting variants: the same records
    assert np.array_equal(h["hit_dist"], h["hit_rec"][..., 0])
    assert c["stats"]["closest_rays"] == len(S) and h["stats"]["trace_launches"] == 1
    return h


@pytest.fixture(scope="module")
def torch_cuda(gpu):
    import torch
    assert torch.cuda.is_available()
    return torch


SPHERE_UV_TOTAL = {}


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[4:-4])
def test_trace_rays_equal_reference_records(fray, torch_cuda, path):
    z, s = load_case(fray, path)
    s.beginRender()
    h = _records_three_ways(torch_cuda, s, z)
    n = _check_records(s, z, h["hit_id"], h["hit_rec"], os.path.basename(path))
    SPHERE_UV_TOTAL[os.path.basename(path)] = n
    print("%s: %d rays, %d sphere u, v differ (<= %d x 2^-52)" % (os.path.basename(path), len(h["hit_id"]), n, SPHERE_UV_ULPS))
    s.close()


@pytest.mark.parametrize("name,seed,fans", GENERATED, ids=[g[0] for g in GENERATED])
def test_trace_rays_equal_reference_records_generated(fray, torch_cuda, tmp_path, name, seed, fans):
    z, s = _generated_case(fray, tmp_path, name, seed, fans)
    s.beginRender()
    h = _records_three_ways(torch_cuda, s, z)
    n = _check_records(s, z, h["hit_id"], h["hit_rec"], name)
    SPHERE_UV_TOTAL[name] = n
    print("%s: %d rays, %d sphere u, v differ (<= %d x 2^-52)" % (name, len(h["hit_id"]), n, SPHERE_UV_ULPS))
    s.close()


def test_sphere_uv_report():
    """(runs after the two above) the count the PR reports: sphere u, v that are not glibc's bits"""
    if SPHERE_UV_TOTAL:
        print("sphere u, v differing from the reference: %d over %d fixtures" % (sum(SPHERE_UV_TOTAL.values()), len(SPHERE_UV_TOTAL)))


# ---- camera rays -------------------------------------------------------------------------------------------------------------------------
def _stereo_scene(fray, name):
    return fray.Scene.parseScene(os.path.join(ROOT, "tests", "scenes", name, "scene.fray"))


@pytest.mark.parametrize("scene", ["cornell_box.fray", "boxed.fray", "fuzz3009"])
def test_camera_rays_equal_oracle(fray, oracle, gpu, scene):
    s = _stereo_scene(fray, scene) if scene.startswith("fuzz") else open_scene(fray, scene, 64, 48)
    s.beginRender()
    W, H = s.frame_size
    o, d = s.camera_rays()
    assert o.shape == (H, W, 3) and d.shape == (H, W, 3)
    so, sd = np.zeros(3), np.zeros(3)
    for y in range(H):
        for x in range(W):
            oracle.lib.fray_oracle_camera_ray(s.desc, float(x), float(y), so.ctypes.data, sd.ctypes.data)
            assert np.array_equal(o[y, x], so) and np.array_equal(d[y, x], sd), (x, y)
    # film positions given explicitly, integer and not, through both entries
    rng = np.random.default_rng(7)
    xy = np.concatenate([np.stack(np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)), -1).reshape(-1, 2),
                         rng.random((300, 2)) * [W, H]])
    o2, d2 = s.camera_rays(xy)
    assert np.array_equal(o2[:W * H], o.reshape(-1, 3)) and np.array_equal(d2[:W * H], d.reshape(-1, 3))
    for i in range(W * H, len(xy), 37):
        oracle.lib.fray_oracle_camera_ray(s.desc, xy[i, 0], xy[i, 1], so.ctypes.data, sd.ctypes.data)
        assert np.array_equal(o2[i], so) and np.array_equal(d2[i], sd), i
    import torch
    ot, dt = s.camera_rays(torch.from_numpy(xy).cuda())
    assert np.array_equal(ot.cpu().numpy(), o2) and np.array_equal(dt.cpu().numpy(), d2)
    s.close()


@pytest.mark.parametrize("name", ["fuzz3009", "fuzz3010"])
def test_camera_rays_stereo_eyes(fray, gpu, name):
    s = _stereo_scene(fray, name)
    sep = s.camera.stereoSeparation
    assert sep > 0
    s.beginRender()
    oc, dc = s.camera_rays()
    oL, dL = s.camera_rays(eye=1)
    oR, dR = s.camera_rays(eye=2)
    assert np.array_equal(dL, dc) and np.array_equal(dR, dc)
    vL, vR = (oc - oL).reshape(-1, 3), (oR - oc).reshape(-1, 3)
    assert np.allclose(vL, vR, rtol=0, atol=1e-12 * (1 + np.abs(oc).max()))
    assert np.allclose(np.linalg.norm(vL, axis=1), sep, rtol=1e-9) and np.allclose(np.linalg.norm(vR, axis=1), sep, rtol=1e-9)
    s.close()


FULL_SIZE = [("cornell_box.fray", 1920, 1080), ("hw9/dragon.fray", 1920, 1080), ("forest.fray", None, None), ("csg_nested", None, None)]


@pytest.mark.parametrize("scene,W,H", FULL_SIZE, ids=[f[0] for f in FULL_SIZE])
def test_trace_camera_rays_equal_primary_hits(fray, torch_cuda, scene, W, H):
    torch = torch_cuda
    if scene == "csg_nested":
        s = fray.Scene.parseScene(os.path.join(ROOT, "tests", "scenes", "csg_nested.fray"))
    else:
        s = open_scene(fray, scene, W, H)
    s.beginRender()
    ids, dist, pst = s.primary_hits(stats=True)
    o, d = s.camera_rays()
    r = s.trace_rays(o, d)
    assert np.array_equal(r["hit_id"], ids) and np.array_equal(r["hit_dist"], dist)
    rt = s.trace_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), stats=True)
    assert np.array_equal(rt["hit_id"].cpu().numpy(), ids) and np.array_equal(rt["hit_dist"].cpu().numpy(), dist)
    for k in ("closest_rays", "node_tests", "kd_inner_visits", "leaf_refs", "tri_tests", "prim_tests", "smooth_hits"):
        assert rt["stats"][k] == pst[k], (k, rt["stats"][k], pst[k])
    assert rt["stats"]["closest_rays"] == ids.size and rt["stats"]["alg_bytes_trace"] == 0
    s.close()


# ---- visibility --------------------------------------------------------------------------------------------------------------------------
def _oracle_visible(oracle, abi, desc, a, b):
    """visible(a, b) from the oracle's probe: the nodes only (n_lights = 0), d = (b - a) * (1.0 / len) in the reference's order"""
    dl = abi.SceneDesc.from_buffer_copy(desc)
    dl.n_lights = 0
    out = np.zeros(9)
    res = np.zeros(len(a), bool)
    for i in range(len(a)):
        e = b[i] - a[i]
        ln = math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
        if not (ln > 0 and math.isfinite(ln)):
            res[i] = True
            continue
        dd = np.ascontiguousarray(e * (1.0 / ln))
        st = np.ascontiguousarray(a[i])
        hid = oracle.lib.fray_oracle_probe(C.byref(dl), st.ctypes.data, dd.ctypes.data, out.ctypes.data)
        res[i] = not (hid >= 0 and out[0] < ln)
    return res


def _segments(desc, z, seed, per=120):
    hits = z["hit_rec"][z["hit_id"] >= 0, 1:4][:per]
    targets = []
    for i in range(desc.n_lights):
        L = desc.lights[i]
        targets.append(np.array(L.center[:] if L.kind == 1 else L.pos[:]))
    rng = np.random.default_rng(seed)
    a, b = [], []
    for p in hits:
        for t in targets:
            a.append(p); b.append(t)
        a.append(p); b.append(p + rng.normal(size=3) * 6)
    return np.array(a).reshape(-1, 3), np.array(b).reshape(-1, 3)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[4:-4])
def test_visible_equals_oracle(fray, abi, oracle, torch_cuda, path):
    z, s = load_case(fray, path)
    s.beginRender()
    a, b = _segments(s.desc, z, 11)
    assert len(a) > 0
    want = _oracle_visible(oracle, abi, s.desc, a, b)
    vis, st = s.visible(a, b, stats=True)
    assert vis.dtype == np.bool_ and np.array_equal(vis, want), np.argwhere(vis != want)[:5].ravel()
    assert st["shadow_rays"] == len(a) and st["shadow_launches"] == 1
    vt, _ = s.visible(torch_cuda.from_numpy(a).cuda(), torch_cuda.from_numpy(b).cuda(), stream=torch_cuda.cuda.Stream())
    assert vt.dtype == torch_cuda.bool and np.array_equal(vt.cpu().numpy(), want)
    s.close()


@pytest.mark.parametrize("name,seed,fans", GENERATED[::3], ids=[g[0] for g in GENERATED[::3]])
def test_visible_equals_oracle_generated(fray, abi, oracle, gpu, tmp_path, name, seed, fans):
    z, s = _generated_case(fray, tmp_path, name, seed, fans)
    s.beginRender()
    a, b = _segments(s.desc, z, seed)
    want = _oracle_visible(oracle, abi, s.desc, a, b)
    vis, _ = s.visible(a, b)
    assert np.array_equal(vis, want), np.argwhere(vis != want)[:5].ravel()
    s.close()


# ---- degenerate and edge input -----------------------------------------------------------------------------------------------------------
def test_degenerate_rays_and_segments(fray, abi, oracle, gpu):
    s = open_scene(fray, "hw9/dragon.fray", 64, 48)
    s.beginRender()
    nan, inf = float("nan"), float("inf")
    o = np.array([[nan, 0, 0], [0, inf, 0], [0, 0, 0], [0, 1, -20], [0, 1, -20], [0, 1, -20], [1e200, 0, 0]])
    d = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0], [nan, 0, 1], [0, -inf, 1], [1e300, 1e300, 0], [0, 0, 1]])
    r = s.trace_rays(o, d, record=True, stats=True)
    assert (r["hit_id"][:6] == -1).all() and (r["hit_dist"][:6] == 1e99).all()
    assert (r["hit_rec"][:6, 0] == 1e99).all() and (r["hit_rec"][:6, 1:] == 0).all()
    assert r["stats"]["closest_rays"] == 1                     # only the last ray is traced
    a = np.array([[1, 2, 3], [nan, 0, 0], [0, 0, 0], [-1e308, 0, 0]])
    b = np.array([[1, 2, 3], [0, 0, 0], [inf, 0, 0], [1e308, 0, 0]])
    vis, st = s.visible(a, b, stats=True)
    assert vis.all() and st["shadow_rays"] == 0
    # far-away origins and directions with tiny components: the oracle's probe
    rng = np.random.default_rng(5)
    O = np.concatenate([rng.normal(size=(40, 3)) * 1e6, rng.normal(size=(40, 3)) * 3 + [0, 1, -12]])
    target = rng.normal(size=(80, 3)) * 0.5 + [0, 1, 0]
    D = target - O
    D[np.arange(40, 80), rng.integers(0, 3, 40)] *= 1e-30
    D[60:70] = [[0, 0, 1]] * 10
    D[60:70, 0] = 1e-300
    r = s.trace_rays(O, D, record=True)
    out = np.zeros(9)
    nhit = 0
    for i in range(len(O)):
        oi, di = np.ascontiguousarray(O[i]), np.ascontiguousarray(D[i])
        hid = oracle.lib.fray_oracle_probe(s.desc, oi.ctypes.data, di.ctypes.data, out.ctypes.data)
        assert r["hit_id"][i] == hid and r["hit_dist"][i] == out[0], i
        nhit += hid >= 0
    assert nhit > 5
    # n = 0 and n = 1, both entries
    e = s.trace_rays(np.zeros((0, 3)), np.zeros((0, 3)), record=True)
    assert e["hit_id"].shape == (0,) and e["hit_rec"].shape == (0, 9)
    v0, _ = s.visible(np.zeros((0, 3)), np.zeros((0, 3)))
    assert v0.shape == (0,)
    one = s.trace_rays(O[70:71], D[70:71])
    assert one["hit_id"][0] == r["hit_id"][70]
    import torch
    t0 = s.trace_rays(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), torch.zeros((0, 3), dtype=torch.float64, device="cuda"))
    assert t0["hit_id"].shape == (0,)
    t1 = s.trace_rays(torch.from_numpy(O[70:71]).cuda(), torch.from_numpy(D[70:71]).cuda())
    assert int(t1["hit_id"][0]) == r["hit_id"][70]
    with pytest.raises(TypeError):
        s.trace_rays(O.astype(np.float32), D)
    with pytest.raises(ValueError):
        s.trace_rays(O[:, :2], D[:, :2])
    s.close()


# ---- scale -------------------------------------------------------------------------------------------------------------------------------
def test_many_rays_in_one_call(fray, torch_cuda):
    torch = torch_cuda
    s = open_scene(fray, "hw9/dragon.fray", 320, 240)
    s.beginRender()
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    n = 1 << 24
    O = torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=g) * 4 + torch.tensor([0.0, 1.0, -6.0], dtype=torch.float64, device="cuda")
    D = torch.randn((n, 3), dtype=torch.float64, device="cuda", generator=g)
    whole = s.trace_rays(O, D)
    parts = [s.trace_rays(O[k:k + n // 64], D[k:k + n // 64]) for k in range(0, n, n // 64)]
    assert torch.equal(whole["hit_id"], torch.cat([p["hit_id"] for p in parts]))
    assert torch.equal(whole["hit_dist"], torch.cat([p["hit_dist"] for p in parts]))
    assert int((whole["hit_id"] >= 0).sum()) > 1000
    s.close()


# ---- scene state -------------------------------------------------------------------------------------------------------------------------
FIGURES = ("whitted_path", "contracted_launches", "fans_filed", "fan_children", "fan_children_looked_up", "fans_given_up", "pt_budget_effective_mib",
           "pt_lanes", "speculate_fans", "fp_contract", "fused_whitted_max")


@pytest.mark.parametrize("scene,gi", [("boxed.fray", 0), ("cornell_box.fray", 1)])
def test_query_leaves_the_scene_as_it_was(fray, gpu, scene, gi):
    s = open_scene(fray, scene, 96, 64, gi=gi, numPaths=8)
    s.beginRender()
    img1, _ = s.render(seed=3)
    before = {k: s.get_option(k) for k in FIGURES}
    o, d = s.camera_rays()
    s.trace_rays(o, d, record=True, stats=True)
    s.visible(o.reshape(-1, 3), (o + d * 3).reshape(-1, 3), stats=True)
    assert {k: s.get_option(k) for k in FIGURES} == before
    img2, _ = s.render(seed=3)
    assert np.array_equal(img1, img2)
    s.close()


def test_query_from_inside_a_progress_callback(fray, abi, gpu):
    a = open_scene(fray, "cornell_box.fray", 48, 48, numPaths=8)
    b = open_scene(fray, "boxed.fray", 32, 32)
    a.beginRender()
    b.beginRender()
    O, D = np.array([[0.0, 50, -100]]), np.array([[0.0, 0, 1]])
    seen = []

    def progress(info):
        for sc in (a, b):
            try:
                sc.trace_rays(O, D)
                seen.append("ok")
            except fray.FrayError as e:
                seen.append(e.code)
        try:
            a.visible(O, O + D)
            seen.append("ok")
        except fray.FrayError as e:
            seen.append(e.code)
        return False

    _, st = a.render(seed=1, spp_chunk=2, progress=progress)
    assert not st["cancelled"] and len(seen) >= 3
    assert seen[0::3] == [abi.E_ARG] * (len(seen) // 3) and seen[1::3] == ["ok"] * (len(seen) // 3) and seen[2::3] == [abi.E_ARG] * (len(seen) // 3)
    a.trace_rays(O, D)                                      # the frame is over: the scene answers again
    a.close()
    b.close()
