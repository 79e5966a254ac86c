"""Adaptive frames on a real MI355X (include/frayhip.h "adaptive frames").  Every pixel of an adaptive frame must equal, bit for bit, that pixel of
the ordinary frame rendered at the pixel's final sample count; so every check here is built from fixed-spp frames F_r of the ladder's rungs and the
numpy restatement of the stop rule (tests/adaptive_ladder.py): the expected image, sample-count map and error map, compared exactly."""
import ctypes as C
import math
import os
import shutil

import numpy as np
import pytest

from adaptive_ladder import expected, ladder, rung_error
from conftest import ROOT, bucket_xy, open_scene
from test_gpu_parity import TEXTURED_PLAIN_SCENE

pytestmark = pytest.mark.gpu
CSG = os.path.join(ROOT, "tests", "scenes", "csg_nested.fray")
FLOOR = 0.01


def scene(fray, name, W, H, **over):
    s = open_scene(fray, name, W, H, **over)
    s.beginRender()
    return s


def textured_scene(fray, tmp_path, W, H, spp):
    shutil.copy(os.path.join(ROOT, "tests", "scenes", "plates.obj"), tmp_path / "plates.obj")
    f = tmp_path / "textured_plain.fray"
    f.write_text(TEXTURED_PLAIN_SCENE % ("gi on\n\tpathsPerPixel %d" % spp, "plates.obj"))
    s = fray.Scene.parseScene(str(f))
    s.settings.frameWidth, s.settings.frameHeight, s.settings.wantAA = W, H, 0
    s.beginRender()
    d = s.desc
    assert d.n_textures == 2 and not any(d.meshes[i].has_kd for i in range(d.n_meshes))     # the <8> / <9> variants
    return s


def rung_frames(s, rs, stats=False):
    """F_r for every rung r: the scene's ordinary frame with numPaths = r (wantAA off, numDOFSamples <= r), then the scene's spp restored."""
    n0 = s.settings.numPaths
    out = {}
    for r in rs:
        s.settings.numPaths = r
        s.beginFrame()
        assert s.samples_per_pixel() == r
        out[r] = s.render(seed=42, stats=stats)[0]
    s.settings.numPaths = n0
    s.beginFrame()
    return out


def pick_threshold(frames, mn, spp):
    """A quantile of the rung-1 error under which at least three distinct rungs occur in the expected frame."""
    rs = ladder(mn, spp)
    e = rung_error(frames[rs[1]], frames[rs[0]], FLOOR)
    e = e[np.isfinite(e)]
    for q in (0.5, 0.35, 0.65, 0.2, 0.8, 0.1, 0.9):
        thr = float(np.quantile(e, q))
        if len(np.unique(expected(frames, mn, spp, thr, FLOOR)[1])) >= 3:
            return thr
    pytest.fail("no rung-1 quantile gives three distinct rungs")


def check_against_rungs(s, mn, stats=False, frames=None):
    spp = s.samples_per_pixel()
    rs = ladder(mn, spp)
    frames = frames or rung_frames(s, rs)
    thr = pick_threshold(frames, mn, spp)
    want_rgb, want_spp, want_err = expected(frames, mn, spp, thr, FLOOR)
    rgb, sm, em, info = s.render_adaptive(thr, min_spp=mn, err_floor=FLOOR, stats=stats)
    assert np.array_equal(sm, want_spp), (np.unique(sm, return_counts=True), np.unique(want_spp, return_counts=True))
    assert np.array_equal(rgb, want_rgb)
    assert np.array_equal(em, want_err)
    assert len(np.unique(sm)) >= 3
    assert info["samples"] == int(sm.sum()) == info["stats"]["samples"]
    assert info["rungs"] == len(rs) or (sm < spp).all()
    assert rgb.mean() > 0.0
    if stats:
        assert info["stats"]["closest_rays"] > 0 and info["stats"]["shadow_rays"] > 0
    return info


# (id, scene, W, H, overrides, min_spp, stats)
CASES = [
    ("cornell", "cornell_box.fray", 96, 72, dict(wantAA=0, numPaths=64), 4, False),
    ("smallpt", "smallpt.fray", 64, 48, dict(wantAA=0, numPaths=32), 4, False),
    ("boxed-kd", "boxed.fray", 64, 48, dict(wantAA=0, gi=1, numPaths=16), 2, False),
    ("csg", CSG, 64, 48, dict(wantAA=0, gi=1, numPaths=16), 4, False),
    ("cornell-dof", "cornell_box.fray", 64, 48, dict(wantAA=0, numPaths=32, dof=1, numDOFSamples=2, fNumber=2.0, focalPlaneDist=800.0), 4, False),
    ("cornell-stats", "cornell_box.fray", 64, 48, dict(wantAA=0, numPaths=32), 4, True),
    ("csg-stats", CSG, 64, 48, dict(wantAA=0, gi=1, numPaths=8), 2, True),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_adaptive_equals_its_rung_frames(fray, gpu, case):
    _, name, W, H, over, mn, stats = case
    s = scene(fray, name, W, H, **over)
    check_against_rungs(s, mn, stats)
    s.close()


def test_adaptive_textured_equals_its_rung_frames(fray, gpu, tmp_path):
    s = textured_scene(fray, tmp_path, 64, 48, 16)
    check_against_rungs(s, 2)
    check_against_rungs(s, 2, stats=True)
    s.close()


def test_min_spp_equal_spp_and_infinite_threshold(fray, gpu):
    s = scene(fray, "cornell_box.fray", 64, 48, wantAA=0, numPaths=16)
    full, _ = s.render(seed=42)
    rgb, sm, em, info = s.render_adaptive(0.0, min_spp=16)
    assert np.array_equal(rgb, full) and (sm == 16).all() and info["rungs"] == 2
    rgb, sm, em, info = s.render_adaptive(0.0, min_spp=1000)           # clamped to the frame's spp
    assert np.array_equal(rgb, full) and (sm == 16).all()
    f4 = rung_frames(s, [4])[4]
    rgb, sm, em, info = s.render_adaptive(math.inf, min_spp=4)
    assert np.array_equal(rgb, f4) and (sm == 4).all() and info["rungs"] == 2 and info["samples"] == 4 * 64 * 48
    assert np.isfinite(em).all()
    s.close()


def test_batching_does_not_change_results(fray, gpu):
    s = scene(fray, "cornell_box.fray", 256, 192, wantAA=0, numPaths=64)
    base = s.render_adaptive(0.05, min_spp=4)
    one = s.render_adaptive(0.05, min_spp=4, spp_chunk=1)
    three = s.render_adaptive(0.05, min_spp=4, spp_chunk=3)
    s.set_option("pt_budget_mib", 1)                 # the 64 MiB floor: 49 152 pixels x 32 samples of a rung take several batches
    s.set_option("pt_lanes", 1)
    small = s.render_adaptive(0.05, min_spp=4)
    for other in (one, three, small):
        for a, b in zip(base[:3], other[:3]):
            assert np.array_equal(a, b)
        assert other[3]["samples"] == base[3]["samples"] and other[3]["rungs"] == base[3]["rungs"]
    assert len(np.unique(base[1])) >= 3
    s.close()


def test_buckets_union_and_untouched_pixels(fray, gpu):
    W, H = 150, 100
    s = scene(fray, "cornell_box.fray", W, H, wantAA=0, numPaths=16)
    whole = s.render_adaptive(0.05, min_spp=2)
    BW, BH = (W - 1) // 48 + 1, (H - 1) // 48 + 1
    union = [np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.int32), np.zeros((H, W), np.float32)]
    total = 0
    for first in (0, 1):
        out = (np.full((H, W, 3), -7.0, np.float32), np.full((H, W), -3, np.int32), np.full((H, W), -5.0, np.float32))
        rgb, sm, em, info = s.render_adaptive(0.05, min_spp=2, bucket_first=first, bucket_stride=2, out=out)
        assert rgb is out[0]
        mask = np.zeros((H, W), bool)
        for b in range(first, BW * BH, 2):
            bx, by = bucket_xy(W, b)
            mask[by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48] = True
        assert (rgb[~mask] == -7.0).all() and (sm[~mask] == -3).all() and (em[~mask] == -5.0).all()
        assert (sm[mask] >= 2).all()
        assert info["samples"] == int(sm[mask].sum())
        total += info["samples"]
        union[0][mask], union[1][mask], union[2][mask] = rgb[mask], sm[mask], em[mask]
    for a, b in zip(whole[:3], union):
        assert np.array_equal(a, b)
    assert total == whole[3]["samples"]
    s.close()


def test_fp_contract_does_not_apply(fray, gpu):
    s = scene(fray, "cornell_box.fray", 64, 48, wantAA=0, numPaths=16)
    exact = s.render_adaptive(0.05, min_spp=2)
    s.set_option("fp_contract", 1)
    s.render(seed=42)
    assert s.get_option("contracted_launches") > 0
    relaxed = s.render_adaptive(0.05, min_spp=2)
    assert s.get_option("contracted_launches") == 0
    for a, b in zip(exact[:3], relaxed[:3]):
        assert np.array_equal(a, b)
    s.close()


def test_black_frame(fray, gpu):
    s = scene(fray, "cornell_box.fray", 61, 47, wantAA=0, numPaths=16, maxTraceDepth=-1)
    rgb, sm, em, info = s.render_adaptive(0.0, min_spp=4, stats=True)
    assert (rgb == 0).all() and (sm == 4).all() and (em == 0).all()
    assert info["samples"] == 4 * 61 * 47 == info["stats"]["samples"] and info["rungs"] == 2
    s.close()


def _raw(fray, abi, s, a, fr=None):
    W, H = s.frame_size
    rgb = np.zeros((H, W, 3), np.float32)
    fr = fr or abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=0, bucket_stride=1)
    return fray.lib.frayhip_render_adaptive(s._dev, C.byref(fr), C.byref(a), rgb.ctypes.data, None, None, None)


@pytest.mark.parametrize("what", ["whitted", "stereo", "long-generators"])
def test_unsupported_frames(fray, abi, gpu, what):
    over = {"whitted": dict(gi=0, wantAA=1), "stereo": dict(wantAA=0, numPaths=8, stereoSeparation=12.0),
            "long-generators": dict(wantAA=0, numPaths=8, maxTraceDepth=25)}[what]
    s = scene(fray, "cornell_box.fray", 32, 24, **over)
    before, _ = s.render(seed=42)
    with pytest.raises(fray.FrayError) as e:
        s.render_adaptive(0.05, min_spp=2)
    assert e.value.code == abi.E_UNSUPPORTED
    after, _ = s.render(seed=42)
    assert np.array_equal(before, after) and np.isfinite(after).all()
    s.close()


def test_argument_checks_with_a_scene(fray, abi, gpu):
    s = scene(fray, "cornell_box.fray", 100, 60, wantAA=0, numPaths=8)
    assert _raw(fray, abi, s, abi.Adaptive(min_spp=9, threshold=0.1, err_floor=0.01)) == abi.E_ARG
    assert b"min_spp must be <=" in fray.lib.frayhip_last_error()
    for first, stride in ((2, 2), (-1, 1), (5, 3)):
        fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=first, bucket_stride=stride)
        assert _raw(fray, abi, s, abi.Adaptive(min_spp=2, threshold=0.1, err_floor=0.01), fr) == abi.E_ARG
        assert b"bucket" in fray.lib.frayhip_last_error()
    # a call from inside a progress callback: the scene is rendering
    codes = []

    def progress(info):
        try:
            s.render_adaptive(0.1, min_spp=2)
        except fray.FrayError as e:
            codes.append(e.code)
    s.render(seed=42, spp_chunk=4, progress=progress)
    assert codes and set(codes) == {abi.E_ARG}
    assert _raw(fray, abi, s, abi.Adaptive(min_spp=8, threshold=0.1, err_floor=0.01)) == abi.OK
    s.close()


def test_device_entry_on_a_stream(fray, gpu):
    import torch
    s = scene(fray, "cornell_box.fray", 80, 60, wantAA=0, numPaths=32)
    host = s.render_adaptive(0.05, min_spp=4)
    dev = torch.device("cuda", 0)
    rgb = torch.full((60, 80, 3), -1.0, dtype=torch.float32, device=dev)
    spp = torch.full((60, 80), -1, dtype=torch.int32, device=dev)
    err = torch.full((60, 80), -1.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        info = s.render_adaptive_device(rgb.data_ptr(), spp.data_ptr(), err.data_ptr(), threshold=0.05, min_spp=4, stream=stream)
    torch.cuda.current_stream(dev).wait_stream(stream)
    assert np.array_equal(rgb.cpu().numpy(), host[0]) and np.array_equal(spp.cpu().numpy(), host[1]) and np.array_equal(err.cpu().numpy(), host[2])
    assert info["samples"] == host[3]["samples"] and info["rungs"] == host[3]["rungs"]
    rgb2 = torch.zeros_like(rgb)
    s.render_adaptive_device(rgb2.data_ptr(), threshold=0.05, min_spp=4, stream=stream.cuda_stream)      # spp / err not asked for
    assert torch.equal(rgb, rgb2)
    s.close()


def test_larger_frame_equals_its_rung_frames(fray, gpu):
    s = scene(fray, "cornell_box.fray", 640, 480, wantAA=0, numPaths=64)
    check_against_rungs(s, 4)
    s.close()
