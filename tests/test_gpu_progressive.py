"""Progressive frames on a real MI355X (include/frayhip.h): progress callbacks, running-mean previews and cancel at the batch seam.

The per-pixel FP32 sum runs in sample order from batch to batch and a sample's seed does not depend on the frame's spp, so after s
samples the running mean IS the frame of s samples per pixel: every comparison here is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, bucket_xy, open_scene

pytestmark = pytest.mark.gpu
COUNTERS = ["closest_rays", "shadow_rays", "node_tests", "kd_inner_visits", "leaf_refs", "tri_tests", "prim_tests",
            "smooth_hits", "samples", "texture_fetches"]
CSG = os.path.join(ROOT, "tests", "scenes", "csg_nested.fray")

# (id, scene, W, H, overrides, spp_chunk, the setting that holds spp -- None where no frame of fewer samples exists)
CASES = [
    ("pt-mono-4lanes", "cornell_box.fray", 640, 480, dict(numPaths=80, wantAA=0), 8, "numPaths"),    # 25.8 M samples: four lanes
    ("pt-stereo", "cornell_box.fray", 96, 64, dict(numPaths=12, wantAA=0, stereoSeparation=12.0), 2, "numPaths"),
    ("pt-long-generators", "cornell_box.fray", 64, 48, dict(numPaths=12, wantAA=0, maxTraceDepth=25), 2, "numPaths"),
    ("pt-csg", CSG, 96, 72, dict(gi=1, numPaths=12, wantAA=0), 2, "numPaths"),
    ("whitted-fans", "hw9/dragon.fray", 96, 64, dict(wantAA=1), 1, None),                    # five AA samples, speculative glossy fans
    ("wavefront-dof-kd", "forest.fray", 96, 72, dict(wantAA=0, dof=1, numDOFSamples=12, interactive=0), 2, "numDOFSamples"),
    ("fused-dof", "zaphod.fray", 96, 64, dict(wantAA=0, dof=1, numDOFSamples=12), 2, "numDOFSamples"),
    ("black", "cornell_box.fray", 61, 47, dict(numPaths=6, wantAA=0, maxTraceDepth=-1), 2, None),
]


def scene_for(fray, name, W, H, over):
    s = open_scene(fray, name, W, H, **over)
    s.beginRender()
    return s


def with_spp(fray, case, spp):
    """A fresh scene of the case, rendering `spp` samples per pixel."""
    _, name, W, H, over, _, field = case
    return scene_for(fray, name, W, H, dict(over, **{field: spp}))


class Recorder:
    """A progress callback that keeps every call (previews copied) and cancels at the `cancel_at`-th call."""

    def __init__(self, cancel_at=None, inside=None):
        self.calls, self.cancel_at, self.inside = [], cancel_at, inside

    def __call__(self, info):
        rec = dict(info)
        if "image" in info:
            rec["image"] = info["image"].copy()
        self.calls.append(rec)
        if self.inside:
            self.inside(info)
        return self.cancel_at is not None and len(self.calls) == self.cancel_at

    def check_sequence(self, batches_total=None):
        done = [c["samples_done"] for c in self.calls]
        assert all(a < b for a, b in zip(done, done[1:])), done
        assert [c["final"] for c in self.calls] == [0] * (len(self.calls) - 1) + [1]
        assert all(c["samples_total"] == self.calls[0]["samples_total"] and c["batches_total"] == self.calls[0]["batches_total"] for c in self.calls)
        assert [c["batches_done"] for c in self.calls[:-1]] == list(range(1, len(self.calls)))
        if batches_total is not None:
            assert self.calls[-1]["batches_total"] == batches_total
        return self.calls[-1]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_progressive_frame_equals_the_blocking_frame(fray, abi, gpu, case):
    _, name, W, H, over, chunk, _ = case
    s = scene_for(fray, name, W, H, over)
    spp = s.samples_per_pixel()
    ref, _ = s.render(spp_chunk=chunk)
    rec = Recorder()
    img, st = s.render(spp_chunk=chunk, progress=rec, preview_ms=0)
    assert not st["cancelled"] and st["samples_done"] == spp
    assert np.array_equal(img, ref)
    nb = 1 if over.get("maxTraceDepth", 0) < 0 else -(-spp // chunk)
    last = rec.check_sequence(batches_total=nb)
    assert last["samples_done"] == spp == last["samples_total"] and last["batches_done"] == nb
    assert last["preview"] == 1 and np.array_equal(last["image"], ref)
    assert all(c["preview"] == 1 for c in rec.calls)                           # preview_ms = 0: after every batch
    # every work counter of the instrumented variants
    _, ref_st = s.render(spp_chunk=chunk, stats=True)
    img2, st2 = s.render(spp_chunk=chunk, stats=True, progress=Recorder(), preview_ms=0)
    assert np.array_equal(img2, ref)
    for k in COUNTERS:
        assert st2[k] == ref_st[k], k
    s.close()


def test_progressive_primary_ids_make_one_final_call(fray, abi, gpu):
    s = scene_for(fray, "boxed.fray", 100, 75, dict(wantAA=0))
    ids, dist, ref_st = s.primary_hits(stats=True)
    calls = []

    def cb(_user, p):
        calls.append(p.contents.as_dict())
        return 1                                         # the final call's return value is ignored
    req = abi.Progressive(fn=abi.PROGRESS_FN(cb), user=None, preview_ms=0.0)
    fr = abi.Frame(mode=abi.MODE_PRIMARY_ID, seed=0, bucket_first=0, bucket_stride=1, spp_chunk=0, flags=abi.FRAME_STATS)
    ids2 = np.full_like(ids, -9)
    dist2 = np.zeros_like(dist)
    st = abi.Stats()
    assert fray.lib.frayhip_render_progressive(s._dev, C.byref(fr), C.byref(req), None, ids2.ctypes.data, dist2.ctypes.data, C.byref(st)) == 0
    assert np.array_equal(ids, ids2) and np.array_equal(dist, dist2)
    assert len(calls) == 1 and calls[0]["final"] == 1 and calls[0]["preview"] == 0
    assert calls[0]["samples_done"] == calls[0]["samples_total"] == 1
    for k in COUNTERS:
        assert getattr(st, k) == ref_st[k], k
    s.close()


PREVIEW_CASES = [c for c in CASES if c[0] in ("pt-mono-4lanes", "pt-stereo", "wavefront-dof-kd")] + [
    ("whitted-recursive-dof", "hw9/dragon.fray", 64, 48, dict(wantAA=0, dof=1, numDOFSamples=6), 2, "numDOFSamples"),
]


@pytest.mark.parametrize("case", PREVIEW_CASES, ids=lambda c: c[0])
def test_previews_are_exact_lower_spp_frames(fray, abi, gpu, case):
    _, name, W, H, over, chunk, field = case
    s = scene_for(fray, name, W, H, over)
    if case[0] == "whitted-recursive-dof":
        s.render(spp_chunk=chunk)
        assert s.get_option("whitted_path") == 0
    rec = Recorder()
    s.render(spp_chunk=chunk, progress=rec, preview_ms=0)
    rec.check_sequence()
    previews = [c for c in rec.calls if c["preview"] and not c["final"]]
    assert len(previews) >= 2
    for c in previews[:3] + previews[-1:]:
        t = with_spp(fray, case, c["samples_done"])
        low, _ = t.render(spp_chunk=chunk)
        assert np.array_equal(c["image"], low), c["samples_done"]
        t.close()
    s.close()


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "black"], ids=lambda c: c[0])
def test_cancel_gives_the_exact_frame_of_the_samples_resolved(fray, abi, gpu, case):
    _, name, W, H, over, chunk, field = case
    # a fresh scene's frame, then cancel at the first callback of a frame with more batches than lanes
    fresh = scene_for(fray, name, W, H, over)
    ref, _ = fresh.render(spp_chunk=chunk)
    fresh.close()
    s = scene_for(fray, name, W, H, over)
    spp = s.samples_per_pixel()
    assert -(-spp // chunk) >= 5
    rec = Recorder(cancel_at=1)
    img, st = s.render(spp_chunk=chunk, progress=rec, preview_ms=-1)
    last = rec.check_sequence()
    assert st["cancelled"] and last["final"] == 1 and last["samples_done"] == st["samples_done"] < spp
    assert st["samples_done"] % chunk == 0 and st["samples_done"] > rec.calls[0]["samples_done"]
    assert rec.calls[0]["preview"] == 0 and last["preview"] == 1 and np.array_equal(last["image"], img)
    if field is not None:
        t = with_spp(fray, case, st["samples_done"])
        low, _ = t.render(spp_chunk=chunk)
        assert np.array_equal(img, low)
        t.close()
        # the work counters of the cancelled frame are those of the frame of its samples
        _, cst = s.render(spp_chunk=chunk, stats=True, progress=Recorder(cancel_at=1))
        assert cst["cancelled"]
        t = with_spp(fray, case, cst["samples_done"])
        _, low_st = t.render(spp_chunk=chunk, stats=True)
        for k in COUNTERS:
            assert cst[k] == low_st[k], k
        t.close()
    # the scene is as reusable after a cancel as after a finished frame
    again, _ = s.render(spp_chunk=chunk)
    assert np.array_equal(again, ref)
    s.close()


def test_cancel_with_the_c_abi_returns_e_cancelled(fray, abi, gpu):
    s = scene_for(fray, "cornell_box.fray", 96, 64, dict(numPaths=24, wantAA=0))
    calls = []

    def cb(_user, p):
        calls.append(p.contents.as_dict())
        return 1
    req = abi.Progressive(fn=abi.PROGRESS_FN(cb), user=None, preview_ms=-1.0)
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=2, flags=0)
    rgb = np.zeros((64, 96, 3), np.float32)
    st = abi.Stats()
    assert fray.lib.frayhip_render_progressive(s._dev, C.byref(fr), C.byref(req), rgb.ctypes.data, None, None, C.byref(st)) == abi.E_CANCELLED
    assert calls[-1]["final"] == 1 and calls[-1]["samples_done"] < 24
    s.close()


def test_device_entry_on_a_torch_stream(fray, abi, gpu):
    import torch
    case = CASES[1]
    _, name, W, H, over, chunk, _ = case
    s = scene_for(fray, name, W, H, over)
    ref, _ = s.render(spp_chunk=chunk)
    host = Recorder()
    s.render(spp_chunk=chunk, progress=host, preview_ms=0)
    d = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    seen = []

    def cb(info):
        if info["preview"]:
            assert info["d_rgb"] == d.data_ptr()
            seen.append((info["samples_done"], d.cpu().numpy().copy()))
    st = s.render_device(d.data_ptr(), spp_chunk=chunk, stream=stream.cuda_stream, progress=cb, preview_ms=0)
    stream.synchronize()
    assert not st["cancelled"]
    assert np.array_equal(d.cpu().numpy(), ref)
    hp = {c["samples_done"]: c["image"] for c in host.calls if c["preview"]}
    assert [k for k, _ in seen] == sorted(hp)
    for k, img in seen:
        assert np.array_equal(img, hp[k]), k
    # cancelled on the device entry: the frame of the samples resolved
    st = s.render_device(d.data_ptr(), spp_chunk=chunk, stream=stream.cuda_stream, progress=lambda i: True)
    stream.synchronize()
    assert st["cancelled"]
    low, _ = with_spp(fray, case, st["samples_done"]).render(spp_chunk=chunk)
    assert np.array_equal(d.cpu().numpy(), low)
    s.close()


def test_bucket_subset_leaves_other_pixels_untouched(fray, abi, gpu):
    W, H = 150, 100
    s = scene_for(fray, "cornell_box.fray", W, H, dict(numPaths=12, wantAA=0))
    full, _ = s.render(spp_chunk=2)
    mine = np.zeros((H, W), bool)
    for b in range(1, ((W + 47) // 48) * ((H + 47) // 48), 3):
        bx, by = bucket_xy(W, b)
        mine[by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48] = True
    out = np.full((H, W, 3), -7.0, np.float32)
    rec = Recorder()
    img, _ = s.render(spp_chunk=2, bucket_first=1, bucket_stride=3, out=out, progress=rec, preview_ms=0)
    rec.check_sequence()
    assert len(rec.calls) > 2
    for c in rec.calls:
        assert np.all(c["image"][~mine] == -7.0)
    assert np.all(img[~mine] == -7.0) and np.array_equal(img[mine], full[mine])
    s.close()


def test_render_from_inside_the_callback_is_refused(fray, abi, gpu):
    s = scene_for(fray, "cornell_box.fray", 96, 64, dict(numPaths=8, wantAA=0))
    ref, _ = s.render(spp_chunk=2)
    codes = []

    def inside(info):
        if info["final"]:
            return
        try:
            s.render(spp_chunk=2)
            codes.append(0)
        except fray.FrayError as e:
            codes.append(e.code)
        try:
            s.set_option("pt_lanes", 1)
            codes.append(0)
        except fray.FrayError as e:
            codes.append(e.code)
    rec = Recorder(inside=inside)
    img, st = s.render(spp_chunk=2, progress=rec)
    assert codes and all(c == abi.E_ARG for c in codes)
    assert not st["cancelled"] and np.array_equal(img, ref)
    s.close()


def test_exception_in_the_callback_cancels_and_is_raised(fray, abi, gpu):
    s = scene_for(fray, "cornell_box.fray", 96, 64, dict(numPaths=24, wantAA=0))
    ref, _ = s.render(spp_chunk=2)
    calls = []

    def boom(info):
        calls.append(info)
        if not info["final"]:
            raise ValueError("stop here")
    with pytest.raises(ValueError, match="stop here"):
        s.render(spp_chunk=2, progress=boom)
    assert calls[-1]["final"] == 1 and calls[-1]["samples_done"] < 24 and len(calls) == 2
    again, _ = s.render(spp_chunk=2)
    assert np.array_equal(again, ref)
    s.close()
