"""Temporal accumulation on the GPU (include/frayhip.h "temporal accumulation"):
1. the library against the numpy restatement (tests/temporal_ref.py) on rendered inputs, bit for bit, host and device entries;
2. the reprojection rule: a repeated view finds every pixel's history, a view turned by two degrees at least nine in ten;
3. frayhip_denoise_signal against frayhip_denoise;
4. Scene.render_sequence is the functional calls chained by hand, and leaves the scene as it found it;
5. quality of the last of eight 4-spp frames against a 1024-spp frame."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import temporal_ref
from conftest import open_scene

pytestmark = pytest.mark.gpu
F = np.float32


def _camera(abi, s, yaw=0.0, move=(0.0, 0.0, 0.0)):
    c = abi.Camera.from_buffer_copy(s.camera)
    c.yaw += yaw
    for k in range(3):
        c.pos[k] += move[k]
    return c


def _set_camera(s, cam):
    C.memmove(C.byref(s.desc.camera), C.byref(cam), C.sizeof(cam))
    s.beginFrame()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _report(what, got, ref):
    """array_equal, with the worst pixel in the message when it fails."""
    if np.array_equal(got, ref):
        return
    bad = np.argwhere(got != ref)
    i = tuple(bad[0])
    raise AssertionError("%s: %d of %d values differ, first at %s: library %r, restatement %r" % (what, len(bad), got.size, i, got[i], ref[i]))


# ---- 1. the library against the restatement ----------------------------------------------------------------------------------------------------
def _chain(fray, abi, name, W, H, cams, seed, over, params):
    """Frames and features along `cams`, then the accumulation chain through the host entry, the device entry and the restatement."""
    import torch
    s = open_scene(fray, name, W, H, **over)
    s.beginRender()
    base = abi.Camera.from_buffer_copy(s.camera)
    frames = []
    for k, (yaw, move) in enumerate(cams):
        cam = abi.Camera.from_buffer_copy(base)
        cam.yaw += yaw
        for i in range(3):
            cam.pos[i] += move[i]
        _set_camera(s, cam)
        rgb, _ = s.render(seed=seed + k)
        feat = s.render_features(min(4, s.samples_per_pixel()), seed=seed + k)
        frames.append((rgb, feat, fray.view_from_camera(cam, W, H)))
    s.close()
    hist = hist_t = hist_r = view = None
    for k, (rgb, feat, v) in enumerate(frames):
        hist, sig, var, st = fray.temporal_accumulate(rgb, feat, view, hist, stats=True, **params)
        assert st["ms_kernels"] > 0 and np.isfinite(hist).all() and np.isfinite(var).all()
        hist_r, sig_r, var_r = temporal_ref.accumulate(rgb, feat, view, hist_r, **params)
        _report("%s frame %d hist_out" % (name, k), hist, hist_r)
        _report("%s frame %d signal" % (name, k), sig, sig_r)
        _report("%s frame %d variance" % (name, k), var, var_r)
        t = fray.temporal_accumulate(torch.from_numpy(rgb).cuda(), torch.from_numpy(feat).cuda(), view, hist_t, **params)
        hist_t = t[0]
        assert _same_bits(t[0].cpu().numpy(), hist) and _same_bits(t[1].cpu().numpy(), sig) and _same_bits(t[2].cpu().numpy(), var), k
        view = v
        N = hist[..., 3]
        hit = np.any(hist[..., 8:11] != 0, axis=2)
        print("%s frame %d: %.1f %% of the pixels with a normal found history, N max %.3f, %d pixels on the spatial variance"
              % (name, k, 100.0 * (N[hit] > 1).mean(), N.max(), int((N < params.get("variance_history", 4)).sum())))
    return hist


@pytest.mark.parametrize("demodulate", [1, 0])
def test_accumulate_matches_restatement_cornell(fray, abi, gpu, demodulate):
    cams = [(0.0, (0, 0, 0)), (2.0, (0, 0, 0)), (2.0, (5.0, 0.0, 0.0))]
    hist = _chain(fray, abi, "cornell_box.fray", 131, 77, cams, 5, dict(numPaths=4), dict(demodulate=demodulate))
    N = hist[..., 3]
    assert N.max() > 2.5 and (N == 1).any()            # a three-frame chain: history two frames deep, and pixels without any


def test_accumulate_matches_restatement_forest(fray, abi, gpu):
    # KD meshes, bump-mapped normals, environment misses; a DOF frame's jittered samples
    hist = _chain(fray, abi, "forest.fray", 131, 77, [(0.0, (0, 0, 0)), (1.5, (0, 0, 0))], 9, dict(gi=0, dof=1, numDOFSamples=4), {})
    miss = ~np.any(hist[..., 8:11] != 0, axis=2)
    assert miss.any() and np.all(hist[miss][:, 3] == 1) and (hist[..., 3] > 1).any()


def test_short_variance_history_skips_the_window(fray, abi, gpu):
    s = open_scene(fray, "cornell_box.fray", 64, 48, numPaths=2)
    s.beginRender()
    rgb, _ = s.render(seed=3)
    feat = s.render_features(2, seed=3)
    s.close()
    for vh in (1, 2, 9):
        got = fray.temporal_accumulate(rgb, feat, variance_history=vh)
        ref = temporal_ref.accumulate(rgb, feat, variance_history=vh)
        for a, b in zip(got, ref):
            _report("variance_history %d" % vh, a, b)
        assert (got[2].any()) == (vh > 1)               # one frame: m2 - m1^2 is zero, only the window sees a spread


# ---- 2. the rule finds history where it should ---------------------------------------------------------------------------------------------------
def _whitted_features(fray, abi, name, W, H, yaws):
    s = open_scene(fray, name, W, H, gi=0, wantAA=0, dof=0)
    s.beginRender()
    base = abi.Camera.from_buffer_copy(s.camera)
    out = []
    for yaw in yaws:
        cam = abi.Camera.from_buffer_copy(base)
        cam.yaw += yaw
        _set_camera(s, cam)
        rgb, _ = s.render(seed=42)
        out.append((rgb, s.render_features(1), fray.view_from_camera(cam, W, H)))
    s.close()
    return out


@pytest.mark.parametrize("name", ["cornell_box.fray", "forest.fray"])
def test_same_view_twice_finds_every_pixel(fray, abi, gpu, name):
    (rgb, feat, view), = _whitted_features(fray, abi, name, 160, 120, [0.0])
    h0, _, _ = fray.temporal_accumulate(rgb, feat, film_offset=0.0)
    h1, _, _ = fray.temporal_accumulate(rgb, feat, view, h0, film_offset=0.0)
    hit = np.any(h1[..., 8:11] != 0, axis=2)
    assert hit.any() and np.all(h0[..., 3] == 1)
    N = h1[..., 3]
    assert np.all(N[hit] == 2), (int((N[hit] != 2).sum()), np.argwhere(hit & (N != 2))[:5])
    assert np.all(N[~hit] == 1)


def test_turned_view_finds_most_pixels(fray, abi, gpu):
    shares = {}
    for name in ("cornell_box.fray", "smallpt.fray"):
        for yaw in (1.0, 2.0, 5.0):
            (rgb0, feat0, view0), (rgb1, feat1, _) = _whitted_features(fray, abi, name, 96, 72, [0.0, yaw])
            h0, _, _ = fray.temporal_accumulate(rgb0, feat0, film_offset=0.0)
            h1, _, _ = fray.temporal_accumulate(rgb1, feat1, view0, h0, film_offset=0.0)
            hit = np.any(h1[..., 8:11] != 0, axis=2)
            shares[name, yaw] = float((h1[..., 3][hit] == 2).mean())
            print("%s yaw +%g: %.1f %% of the pixels with a normal have N = 2" % (name, yaw, 100 * shares[name, yaw]))
    # The floor only catches a projection that rejects wholesale: the strip that enters the frame and the silhouettes have no history.
    assert shares["cornell_box.fray", 2.0] >= 0.90, shares


# ---- 3. the levels on a given signal ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [0, 1])
def test_denoise_signal_matches_denoise(fray, gpu, demodulate):
    import torch
    s = open_scene(fray, "cornell_box.fray", 131, 77, numPaths=8)
    s.beginRender()
    rgb, _ = s.render(seed=5)
    feat = s.render_features(4, seed=5)
    s.settings.numPaths = 4
    s.beginFrame()
    half, _ = s.render(seed=5)
    s.close()
    g = denoise_ref.prepare(rgb, feat, half, demodulate)
    for levels in (1, 5):
        want = fray.denoise(rgb, feat, half, levels=levels, demodulate=demodulate)
        got, st = fray.denoise_signal(g["c"], g["var"], feat, stats=True, levels=levels, demodulate=demodulate)
        err = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-3)
        print("demodulate %d levels %d: worst relative difference %.3g" % (demodulate, levels, err.max()))
        assert st["ms_kernels"] > 0 and err.max() <= 1e-5, (err.max(), np.unravel_index(err.argmax(), err.shape))
        td = fray.denoise_signal(torch.from_numpy(g["c"]).cuda(), torch.from_numpy(g["var"]).cuda(), torch.from_numpy(feat).cuda(),
                                 levels=levels, demodulate=demodulate)
        assert _same_bits(td.cpu().numpy(), got)


# ---- 4. composition -------------------------------------------------------------------------------------------------------------------------------
def test_render_sequence_composition(fray, abi, gpu):
    W, H = 100, 70
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4)
    s.beginRender()
    before, _ = s.render(seed=7)
    start = abi.Camera.from_buffer_copy(s.camera)
    cams = [_camera(abi, s, yaw=1.5 * k) for k in range(3)]
    tparams = dict(max_history=16, plane_tolerance=0.03)
    frames = []
    for out, raw, info in s.render_sequence(cams, seed=7, feature_samples=2, temporal=tparams, levels=3):
        assert out.is_cuda and raw.is_cuda and info["history"].is_cuda and info["film_offset"] == 0.5
        frames.append((out.cpu().numpy(), raw.cpu().numpy(), info["features_frame"].cpu().numpy(), info["history"].cpu().numpy()))
    assert len(frames) == 3
    assert bytes(s.camera) == bytes(start)
    after, _ = s.render(seed=7)
    assert np.array_equal(before, after)
    # by hand, through the host entries
    hist = view = None
    for k, cam in enumerate(cams):
        _set_camera(s, cam)
        raw, _ = s.render(seed=7 + k)
        feat = s.render_features(2, seed=7 + k)
        hist, sig, var = fray.temporal_accumulate(raw, feat, view, hist, film_offset=0.5, **tparams)
        out = fray.denoise_signal(sig, var, feat, levels=3)
        view = fray.view_from_camera(cam, W, H)
        assert _same_bits(frames[k][1], raw), k
        assert _same_bits(frames[k][2], feat) and _same_bits(frames[k][3], hist), k
        assert _same_bits(frames[k][0], out), k
    _set_camera(s, start)
    # a generator closed early restores the camera too
    gen = s.render_sequence(cams[1:], seed=7)
    next(gen)
    assert bytes(s.camera) != bytes(start)
    gen.close()
    assert bytes(s.camera) == bytes(start) and np.array_equal(s.render(seed=7)[0], before)
    # Whitted frames: the film offset follows the sampling
    s.settings.gi = 0
    for aa, off in ((0, 0.0), (1, 0.3)):
        s.settings.wantAA = aa
        s.beginFrame()
        _, _, info = next(s.render_sequence([start]))
        assert info["film_offset"] == off
    with pytest.raises(ValueError, match="demodulate"):
        next(s.render_sequence([start], temporal=dict(demodulate=0)))
    with pytest.raises(TypeError):
        next(s.render_sequence([start], temporal=dict(alpha=1)))
    s.close()


def test_render_sequence_refusals(fray, abi, gpu):
    s = open_scene(fray, "boxed.fray", 64, 48, stereoSeparation=1.0)
    s.beginRender()
    start = abi.Camera.from_buffer_copy(s.camera)
    with pytest.raises(fray.FrayError, match="stereo") as e:
        next(s.render_sequence([start]))
    assert e.value.code == abi.E_UNSUPPORTED
    s.close()
    s = open_scene(fray, "cornell_box.fray", 64, 48, numPaths=4, maxTraceDepth=20)
    s.beginRender()
    with pytest.raises(fray.FrayError, match="maxTraceDepth") as e:
        next(s.render_sequence([abi.Camera.from_buffer_copy(s.camera)]))
    assert e.value.code == abi.E_UNSUPPORTED
    s.close()


# ---- 5. quality ---------------------------------------------------------------------------------------------------------------------------------------
FRAMES = 8


def _quality(fray, abi, name, yaw_step):
    """RMS against the 1024-spp frame of the last view: (raw 4-spp frame, render_denoised on it, the sequence's last frame, share of pixels
    with history per frame)."""
    W, H = 320, 240
    s = open_scene(fray, name, W, H, numPaths=1024)
    s.beginRender()
    start = abi.Camera.from_buffer_copy(s.camera)
    cams = [_camera(abi, s, yaw=yaw_step * k) for k in range(FRAMES)]
    _set_camera(s, cams[-1])
    ref, _ = s.render(seed=42)
    ref = ref.astype(np.float64)
    _set_camera(s, start)
    s.settings.numPaths = 4
    s.beginFrame()
    shares = []
    for out, raw, info in s.render_sequence(cams, seed=42, feature_samples=4):
        h = info["history"]
        hit = (h[..., 8:11] != 0).any(dim=2)
        shares.append(float((h[..., 3][hit] > 1).float().mean()))
    seq, raw_last = out.cpu().numpy(), raw.cpu().numpy()
    # the accumulated signal before the filter, albedo multiplied back: what the history alone gives
    acc = (info["signal"] * info["features_frame"][..., 6:9].clamp(min=1e-3)).cpu().numpy()
    # the spatial filter alone on the very same 4-spp frame
    _set_camera(s, cams[-1])
    den, raw, _ = s.render_denoised(seed=42 + FRAMES - 1, feature_samples=4)
    s.close()
    assert np.array_equal(raw, raw_last)
    rms = lambda a: float(np.sqrt(((a.astype(np.float64) - ref) ** 2).mean()))
    r_raw, r_den, r_seq = rms(raw), rms(den), rms(seq)
    print("%s, yaw step %g: RMS raw %.4f, render_denoised %.4f, temporal %.4f (accumulated, unfiltered %.4f); temporal / render_denoised %.3f, "
          "temporal / raw %.3f; history found per frame %s"
          % (name, yaw_step, r_raw, r_den, r_seq, rms(acc), r_seq / r_den, r_seq / r_raw, " ".join("%.3f" % x for x in shares)))
    return r_raw, r_den, r_seq, shares


@pytest.mark.parametrize("name,yaw_step", [("cornell_box.fray", 0.0), ("smallpt.fray", 0.0), ("cornell_box.fray", 1.0)],
                         ids=["cornell_static", "smallpt_static", "cornell_moving"])
def test_temporal_quality(fray, abi, gpu, name, yaw_step):
    r_raw, r_den, r_seq, shares = _quality(fray, abi, name, yaw_step)
    # Only the direction is asserted, as test_denoised_quality does: eight frames of history beat the spatial filter on the same last frame.
    # The estimate was a ratio near 0.5.  Measured on one MI355X ("Temporal accumulation"): temporal / render_denoised 0.81
    # (cornell_box, static), 0.83 (smallpt, static), 0.86 (cornell_box, moving), 0.94 (smallpt, moving: not asserted).
    # Away from the light (97-99 % of the pixels) the ratios are 0.60, 0.39, 0.65 and 0.41: the rest of the squared error is the light's
    # silhouette, which the levels smear with or without history.
    assert r_seq < r_den, (r_raw, r_den, r_seq)
    assert shares[0] == 0


def test_temporal_quality_smallpt_moving_is_recorded(fray, abi, gpu):
    # smallpt has a mirror and a glass sphere: what they show moves with the camera while their first hit does not, so their history is stale
    # by construction.  Printed and recorded ("Temporal accumulation"), not asserted.
    r_raw, r_den, r_seq, shares = _quality(fray, abi, "smallpt.fray", 1.0)
    assert np.isfinite([r_raw, r_den, r_seq]).all() and shares[0] == 0
