"""Radiance queries on the GPU (include/frayhip.h "radiance queries"): trace(ray, rnd) for rays the caller chooses, checked bit for bit against the
library's own frames -- Whitted samples from camera rays with rng_skip 0, path-traced samples from the jittered camera rays with rng_skip 2 -- and
against the documented answers for batching, degenerate input, keys, streams and scene state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, open_scene
from test_gpu_parity import _csg_chain
from test_gpu_rays import GENERATED, _generated_case
from test_oracle_vs_ref import FIXTURES, load_case

pytestmark = pytest.mark.gpu

AA_OFFSETS = [(0, 0), (0.6, 0), (0.3, 0.3), (0, 0.6), (0.6, 0.6)]      # main.cpp:55-61


@pytest.fixture(scope="module")
def torch_cuda(gpu):
    import torch
    assert torch.cuda.is_available()
    return torch


def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def sample_seed(seed, pixel, sample):
    """The RNG contract's per-(pixel, sample) seed (dev_rng.hpp sample_seed), vectorised over uint32 pixels."""
    with np.errstate(over="ignore"):
        p = np.asarray(pixel, np.uint32)
        h = _fmix32(np.uint32(seed) ^ (p * np.uint32(0x9E3779B1)))
        return _fmix32(h ^ (np.uint32(sample) * np.uint32(0x85EBCA77)) ^ np.uint32(0x27D4EB2F))


def jitter(fray, seeds):
    """The first two randfloat()s of a generator seeded with each seed: a path-traced frame's pixel jitter (main.cpp:351-353)."""
    out = np.empty((len(seeds), 2), np.float32)
    f = np.empty(2, np.float32)
    for i, s in enumerate(seeds):
        assert fray.lib.frayhip_debug_rng(int(s), 2, f.ctypes.data, None, None, 0) == 0
        out[i] = f
    return out


def whitted_single_sample(s):
    """the scene's camera rays through every integer pixel, shaded once with seed 42 and key = pixel index"""
    o, d = s.camera_rays()
    return s.shade_rays(o, d, seed=42)


def pixel_grid(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return x.astype(np.float32), y.astype(np.float32)


def pt_by_samples(fray, s, spp, stats=False):
    """A path-traced frame's picture rebuilt from radiance queries: per sample k, the camera rays through the jittered film positions of
    sample_seed(42, p, k), shaded with rng_skip 2 and sample_first k; the float32 sequential mean over k.  Also the summed counters."""
    W, H = s.frame_size
    xs, ys = pixel_grid(W, H)
    p = np.arange(W * H, dtype=np.uint32)
    acc = np.zeros((H, W, 3), np.float32)
    tot = {}
    for k in range(spp):
        j = jitter(fray, sample_seed(42, p, k)).reshape(H, W, 2)
        xy = np.stack([(xs + j[..., 0]).astype(np.float64), (ys + j[..., 1]).astype(np.float64)], axis=-1)      # int + float, main.cpp:359
        o, d = s.camera_rays(xy)
        r = s.shade_rays(o, d, seed=42, sample_first=k, rng_skip=2, stats=stats)
        if stats:
            r, st = r
            for key, v in st.items():
                tot[key] = tot.get(key, 0) + v
        acc = acc + r
    return acc / np.float32(spp), tot


COUNTERS = ("samples", "closest_rays", "shadow_rays", "node_tests", "kd_inner_visits", "leaf_refs", "tri_tests", "prim_tests")


# ---- 1 and 4: Whitted, one sample, against MODE_RENDER ---------------------------------------------------------------------------------------
def _check_whitted(s, z=None):
    """Some fuzz scenes carry a thin lens or a stereo rig: the query stands for neither, so the frame is rendered without them (and then
    compared with the fixture's picture only where it still equals it)."""
    assert not s.settings.gi
    s.settings.wantAA = 0
    s.camera.dof = 0
    s.camera.stereoSeparation = 0
    s.beginRender()
    frame, _ = s.render(seed=42)
    q = whitted_single_sample(s)
    assert q.dtype == np.float32 and q.shape == frame.shape
    bad = np.argwhere((q != frame).any(axis=2))
    assert len(bad) == 0, ("pixels differ from the frame", len(bad), bad[:5].tolist())
    if z is not None and np.array_equal(frame, z["image"]):
        assert np.array_equal(q, z["image"])                  # the reference's own picture, where the frame is it
    # the counting variants: the same colours, and the frame's work counters
    fs, fst = s.render(seed=42, stats=True)
    o, d = s.camera_rays()
    qs, qst = s.shade_rays(o, d, seed=42, stats=True)
    assert np.array_equal(qs, q)
    for k in COUNTERS:
        assert qst[k] == fst[k], (k, qst[k], fst[k])
    return s


# the stored fixtures whose scenes are Whitted (the _aa ones are rendered here with wantAA off; the _dof ones are left to the DOF-free
# fixtures of the same scenes), and the generated scenes of even seeds and of the glossy-fan seeds (random_scene: gi = seed % 2, fans without gi)
WHITTED_FIXTURES = [p for p in FIXTURES if not p.endswith(("_pt.npz", "_dof.npz"))]
WHITTED_GENERATED = [g for g in GENERATED if g[2] or g[1] % 2 == 0]


@pytest.mark.parametrize("path", WHITTED_FIXTURES, ids=lambda p: os.path.basename(p)[4:-4])
def test_whitted_one_sample_equals_frame(fray, gpu, path):
    z, s = load_case(fray, path)
    _check_whitted(s, z).close()


@pytest.mark.parametrize("name,seed,fans", WHITTED_GENERATED, ids=[g[0] for g in WHITTED_GENERATED])
def test_whitted_one_sample_equals_frame_generated(fray, gpu, tmp_path, name, seed, fans):
    z, s = _generated_case(fray, tmp_path, name, seed, fans)
    _check_whitted(s, z).close()


# ---- 2: Whitted with AA ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ref_boxed_aa.npz", "ref_nonconvex_aa.npz"])
def test_whitted_aa_is_mean_of_offset_samples(fray, gpu, name):
    z, s = load_case(fray, os.path.join(ROOT, "tests", "golden", name))
    assert s.settings.wantAA and not s.settings.gi and not s.camera.dof and not s.camera.stereoSeparation > 0
    s.beginRender()
    frame, _ = s.render(seed=42)
    W, H = s.frame_size
    xs, ys = pixel_grid(W, H)
    acc = np.zeros((H, W, 3), np.float32)
    for i, (ox, oy) in enumerate(AA_OFFSETS):
        xy = np.stack([(xs + np.float32(ox)).astype(np.float64), (ys + np.float32(oy)).astype(np.float64)], axis=-1)
        o, d = s.camera_rays(xy)
        acc = acc + s.shade_rays(o, d, seed=42, sample_first=i, keys=np.arange(W * H, dtype=np.uint32).reshape(H, W))
    assert np.array_equal(acc / np.float32(5), frame)
    s.close()


# ---- 3 and 4: path tracing ---------------------------------------------------------------------------------------------------------------------
PT_CASES = ["ref_cornell_pt.npz", "ref_smallpt_pt.npz", "ref_sphtri_pt.npz", "ref_fuzz3001_pt.npz"]


@pytest.mark.parametrize("name", PT_CASES)
def test_path_traced_frame_from_samples(fray, gpu, name):
    z, s = load_case(fray, os.path.join(ROOT, "tests", "golden", name))
    assert s.settings.gi and not s.camera.dof
    s.settings.numPaths, s.settings.wantAA = 3, 0          # (with wantAA on a frame takes max(5, numPaths) samples)
    s.beginRender()
    frame, _ = s.render(seed=42)
    img, _ = pt_by_samples(fray, s, 3)
    bad = np.argwhere((img != frame).any(axis=2))
    assert len(bad) == 0, ("pixels differ from the frame", len(bad), bad[:5].tolist())
    _, fst = s.render(seed=42, stats=True)
    imgs, qst = pt_by_samples(fray, s, 3, stats=True)
    assert np.array_equal(imgs, frame)
    for k in COUNTERS:
        assert qst[k] == fst[k], (k, qst[k], fst[k])
    assert qst["trace_launches"] == 3 * (s.settings.maxTraceDepth + 2)
    s.close()


def test_path_traced_generated_fixture(fray, gpu, tmp_path):
    name, seed, fans = next(g for g in GENERATED if not g[2] and g[1] % 2 == 1)          # odd seeds make path-traced scenes
    z, s = _generated_case(fray, tmp_path, name, seed, fans)
    assert s.settings.gi
    s.camera.dof = 0
    s.settings.numPaths, s.settings.wantAA = 2, 0
    s.beginRender()
    frame, _ = s.render(seed=42)
    img, _ = pt_by_samples(fray, s, 2)
    assert np.array_equal(img, frame)
    s.close()


# ---- 5: batching is invisible --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,gi", [("cornell_box.fray", 1), ("boxed.fray", 0)])
def test_batching_is_invisible(fray, gpu, scene, gi):
    s = open_scene(fray, scene, 640, 480, gi=gi, wantAA=0)
    s.beginRender()
    o, d = s.camera_rays()
    one = s.shade_rays(o, d, spp=8, rng_skip=2)
    acc = np.zeros_like(one)
    for k in range(8):
        acc = acc + s.shade_rays(o, d, spp=1, sample_first=k, rng_skip=2)
    assert np.array_equal(acc / np.float32(8), one)
    counted, st = s.shade_rays(o, d, spp=8, rng_skip=2, stats=True)
    assert np.array_equal(counted, one) and st["samples"] == 8 * 640 * 480
    if gi:
        # 64 MiB at 338 bytes per path (maxTraceDepth 6): 198 546 paths per batch, so 307 200 rays x 8 samples run as two ranges of rays times
        # eight batches of one sample
        s.set_option("pt_budget_mib", 64)
        small, st2 = s.shade_rays(o, d, spp=8, rng_skip=2, stats=True)
        assert st2["trace_launches"] == 16 * (s.settings.maxTraceDepth + 2), st2["trace_launches"]
        assert np.array_equal(small, one)
    s.close()


# ---- 6: long streams -----------------------------------------------------------------------------------------------------------------------
def test_whitted_long_generator_streams(fray, gpu):
    """sphtri's three RectLights of 225 samples each draw far more than 227 words per sample"""
    s = open_scene(fray, "hw12/sphtri.fray", 48, 36, gi=0, wantAA=0)
    _check_whitted(s).close()


def test_path_tracing_long_generators_unsupported(fray, gpu):
    s = open_scene(fray, "cornell_box.fray", 32, 24, wantAA=0, maxTraceDepth=20, numPaths=2)
    s.beginRender()
    o, d = s.camera_rays()
    with pytest.raises(fray.FrayError) as e:
        s.shade_rays(o, d, rng_skip=2)
    assert e.value.code == fray.abi.E_UNSUPPORTED and "maxTraceDepth" in str(e.value)
    s.settings.maxTraceDepth = 19                    # the last depth with register generators: answered
    s.beginRender()
    frame, _ = s.render(seed=42)
    img, _ = pt_by_samples(fray, s, 2)
    assert np.array_equal(img, frame)
    s.close()


@pytest.mark.parametrize("gi", [0, 1])
def test_csg_sixteen_levels(fray, gpu, tmp_path, gi):
    s = fray.Scene.parseScene(_csg_chain(tmp_path, 16))
    s.settings.frameWidth, s.settings.frameHeight, s.settings.wantAA, s.settings.gi, s.settings.numPaths = 40, 30, 0, gi, 2
    if not gi:
        _check_whitted(s).close()
        return
    s.beginRender()
    frame, _ = s.render(seed=42)
    img, _ = pt_by_samples(fray, s, 2)
    assert np.array_equal(img, frame)
    s.close()


# ---- 7: edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gi", [0, 1])
def test_degenerate_rays_black_and_uncounted(fray, gpu, gi):
    s = open_scene(fray, "cornell_box.fray", 16, 16, gi=gi, wantAA=0)
    s.beginRender()
    o, d = s.camera_rays()
    o, d = o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()
    good, _ = s.shade_rays(o, d, spp=2, stats=True)
    d[3] = 0
    d[5, 1] = np.nan
    o[7, 2] = np.inf
    d[9] = [1e200, 0, 0]
    r, st = s.shade_rays(o, d, spp=2, stats=True)
    dead = [3, 5, 7, 9]
    assert (r[dead] == 0).all()
    keep = np.setdiff1d(np.arange(len(o)), dead)
    assert np.array_equal(r[keep], good[keep])
    assert st["samples"] == 2 * (len(o) - len(dead))
    s.close()


def test_negative_depth_is_black_and_empty_is_ok(fray, gpu):
    s = open_scene(fray, "boxed.fray", 16, 12, wantAA=0, maxTraceDepth=-1)
    s.beginRender()
    o, d = s.camera_rays()
    r = s.shade_rays(o, d, spp=3)
    assert r.shape == (12, 16, 3) and (r == 0).all()
    e = s.shade_rays(np.empty((0, 3)), np.empty((0, 3)))
    assert e.shape == (0, 3)
    s.close()


def test_2_24_rays_in_one_call(fray, torch_cuda, gpu):
    torch = torch_cuda
    s = open_scene(fray, "smallpt.fray", 64, 64, gi=0, wantAA=0)
    s.beginRender()
    o, d = s.camera_rays()
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    rep = (1 << 24) // len(o)
    do = torch.from_numpy(o).cuda().repeat(rep, 1)
    dd = torch.from_numpy(d).cuda().repeat(rep, 1)
    big = s.shade_rays(do, dd)
    assert big.shape == (1 << 24, 3)
    pick = np.random.default_rng(7).choice(1 << 24, 2000, replace=False)
    small = s.shade_rays(o[pick % len(o)], d[pick % len(o)], keys=pick.astype(np.uint32))
    assert np.array_equal(big[torch.from_numpy(pick).cuda()].cpu().numpy(), small)
    s.close()


def test_explicit_keys_on_shuffled_pixels(fray, gpu):
    s = open_scene(fray, "boxed.fray", 64, 48, wantAA=0)
    s.beginRender()
    full = whitted_single_sample(s).reshape(-1, 3)
    o, d = s.camera_rays()
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    pick = np.random.default_rng(3).permutation(len(o))[:700]
    r = s.shade_rays(o[pick], d[pick], keys=pick.astype(np.uint32))
    assert np.array_equal(r, full[pick])
    s.close()


# ---- 8: device entry and scene state -----------------------------------------------------------------------------------------------------------
OPTIONS = ("whitted_path", "contracted_launches", "fans_filed", "fan_children", "fan_children_looked_up", "fans_given_up", "pt_budget_mib", "fp_contract")


@pytest.mark.parametrize("scene,gi", [("cornell_box.fray", 1), ("boxed.fray", 0)])
def test_device_entry_and_scene_state(fray, torch_cuda, gpu, scene, gi):
    torch = torch_cuda
    s = open_scene(fray, scene, 48, 36, gi=gi, wantAA=0, numPaths=4)
    s.beginRender()
    before, _ = s.render(seed=42)
    opts = {k: s.get_option(k) for k in OPTIONS}
    o, d = s.camera_rays()
    keys = np.arange(48 * 36, dtype=np.int32).reshape(36, 48)[::-1].copy()
    host = s.shade_rays(o, d, spp=2, rng_skip=2, keys=keys.astype(np.uint32))
    stream = torch.cuda.Stream()
    dev = s.shade_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), spp=2, rng_skip=2, keys=torch.from_numpy(keys).cuda(), stream=stream)
    assert dev.dtype == torch.float32 and dev.is_cuda
    assert np.array_equal(dev.cpu().numpy(), host)
    assert {k: s.get_option(k) for k in OPTIONS} == opts
    after, _ = s.render(seed=42)
    assert np.array_equal(before, after)
    # option fp_contract: the query's arithmetic stays exact, and the last frame's contracted launches stay what they were
    s.set_option("fp_contract", 1)
    contracted = s.get_option("contracted_launches")
    assert np.array_equal(s.shade_rays(o, d, spp=2, rng_skip=2, keys=keys.astype(np.uint32)), host)
    assert s.get_option("contracted_launches") == contracted
    s.close()


def test_query_from_progress_callback_is_refused(fray, gpu):
    s = open_scene(fray, "cornell_box.fray", 32, 24, wantAA=0, numPaths=8)
    s.beginRender()
    o, d = s.camera_rays()
    seen = []

    def progress(info):
        with pytest.raises(fray.FrayError) as e:
            s.shade_rays(o, d)
        seen.append((e.value.code, str(e.value)))

    s.render(seed=42, spp_chunk=2, progress=progress)
    assert seen and all(c == fray.abi.E_ARG and "rendering" in m for c, m in seen)
    assert s.shade_rays(o, d).shape == (24, 32, 3)             # and answered once the frame is done
    s.close()


# ---- 9: the CLI ----------------------------------------------------------------------------------------------------------------------------------
def test_cli_probe_shade_is_the_frame_pixel(fray, gpu):
    scene = os.path.join(ROOT, "scenes", "boxed.fray")          # Whitted, wantAA false
    W, H, X, Y = 64, 48, 21, 30
    s = fray.Scene.parseScene(scene)
    s.settings.frameWidth, s.settings.frameHeight = W, H
    assert not s.settings.gi and not s.settings.wantAA and not s.camera.dof
    s.beginRender()
    frame, _ = s.render(seed=42)
    s.close()
    r = subprocess.run([sys.executable, "-m", "fray_amd", scene, "--probe", str(X), str(Y), "--shade", "--width", str(W), "--height", str(H)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert np.array_equal(np.array(line["rgb"], np.float32), frame[Y, X])
    r = subprocess.run([sys.executable, "-m", "fray_amd", scene, "--probe", str(X), str(Y), "--width", str(W), "--height", str(H)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rgb" not in json.loads(r.stdout.strip().splitlines()[-1])
