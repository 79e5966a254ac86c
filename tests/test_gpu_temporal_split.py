"""Split temporal accumulation on the GPU (include/frayhip.h "split temporal accumulation").  Every comparison is bit for bit:
1. a synthetic five-frame chain: the fused host entry against the restatement (tests/temporal_split_ref.py), the device entry against the host
   entry, and the fused outputs taken apart against two calls of the existing entry;
2. the same chain through a motion frame, against the existing _motion entry, and a motion frame that moves nothing against motion=None;
3. rendered components of cornell_box along three cameras;
4. Scene.render_sequence(split=True) is the public pieces chained by hand, with and without edit=, and its defaults;
5. what it refuses."""
import ctypes as C

import numpy as np
import pytest

import motion_ref
import temporal_ref
import temporal_split_ref as split_ref
from conftest import open_scene

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ("hist_out", "signal_direct", "signal_indirect", "variance_direct", "variance_indirect")


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a).view(np.uint32)


def _same(what, got, want):
    """Equal bit patterns, with the first differing value in the message."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    i = tuple(bad[0])
    raise AssertionError("%s: %d of %d values differ, first at %s: %r against %r" % (what, len(bad), g.size, i, g.view(F)[i], w.view(F)[i]))


def _view(abi, v):
    """An abi.View of the restatement's view dict."""
    out = abi.View()
    for k in ("pos", "right", "up", "front"):
        for i in range(3):
            getattr(out, k)[i] = v[k][i]
    out.tan_x, out.tan_y, out.width, out.height = v["tan_x"], v["tan_y"], v["width"], v["height"]
    return out


def _set_camera(s, cam):
    C.memmove(C.byref(s.desc.camera), C.byref(cam), C.sizeof(cam))
    s.beginFrame()


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(a).cuda()


def _fused_three_ways(fray, k, what, rgb_d, rgb_i, feat, view, hist, hist_t, motion, direct, indirect, shared):
    """One frame of a chain: the fused host entry, the fused device entry against it, and the two existing calls against its parts.  Returns the
    host entry's outputs and the device entry's history."""
    got = fray.temporal_accumulate_split(rgb_d, rgb_i, feat, view, hist, motion=motion, direct=direct, indirect=indirect, **shared)
    t = fray.temporal_accumulate_split(_cuda(rgb_d), _cuda(rgb_i), _cuda(feat), view, hist_t, motion=_cuda(motion), direct=direct,
                                       indirect=indirect, **shared)
    for name, a, b in zip(NAMES, t, got):
        _same("%s frame %d %s, device entry against host entry" % (what, k, name), a, b)
    hd, hi = fray.split_history_parts(got[0])
    hin_d, hin_i = fray.split_history_parts(hist) if hist is not None else (None, None)
    for comp, rgb, hin, want_h, sig, var, prm in (("direct", rgb_d, hin_d, hd, got[1], got[3], direct),
                                                 ("indirect", rgb_i, hin_i, hi, got[2], got[4], indirect)):
        two = fray.temporal_accumulate(rgb, feat, view, hin, motion=motion, **dict(shared, **prm))
        for name, a, b in zip(("history", "signal", "variance"), (want_h, sig, var), two):
            _same("%s frame %d %s %s, fused against the existing entry" % (what, k, comp, name), a, b)
    return got, t[0]


# ---- 1. the synthetic chain ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [0, 1])
def test_synthetic_chain(fray, abi, gpu, demodulate):
    D, I = split_ref.CHAIN_DIRECT, split_ref.CHAIN_INDIRECT
    hist = hist_t = hist_r = view = view_r = None
    differ, young, old, lost = [], [], [], []
    for k, (rgb_d, rgb_i, feat, v, _) in enumerate(split_ref.chain_frames()):
        ref = split_ref.accumulate_split(rgb_d, rgb_i, feat, view_r, hist_r, direct=D, indirect=I, demodulate=demodulate)
        hist_r, view_r = ref[0], v
        ND, NI = hist_r[..., 3], hist_r[..., 15]
        hit = np.any(feat[..., 3:6] != 0, axis=2)
        differ.append(int((ND != NI).sum()))
        young.append(int((NI < I["variance_history"]).sum()))
        old.append(int((NI >= I["variance_history"]).sum()))
        lost.append(int((hit & (NI == 1)).sum()))
        assert not (ND < D["variance_history"]).any()                  # no pixel is ever young for the direct component
        got, hist_t = _fused_three_ways(fray, k, "chain", rgb_d, rgb_i, feat, view, hist, hist_t, None, D, I, dict(demodulate=demodulate))
        for name, a, b in zip(NAMES, got, ref):
            _same("chain frame %d %s, host entry against the restatement" % (k, name), a, b)
        hist, view = got[0], _view(abi, v)
    # what the restatement says these inputs exercise: components whose counts differ, pixels on the window beside pixels off it for the
    # indirect component while the direct one never takes it, and history lost (frame 1 repeats frame 0's view and loses none)
    assert differ[2:] == [648, 360, 378], differ
    assert (young[3], old[3]) == (491, 360) and (young[4], old[4]) == (473, 378), (young, old)
    assert all(n > 0 for n in lost[2:]), lost


# ---- 2. through a motion frame -------------------------------------------------------------------------------------------------------------------
def test_synthetic_chain_with_motion(fray, abi, gpu):
    D, I = split_ref.CHAIN_DIRECT, split_ref.CHAIN_INDIRECT
    hist = hist_t = hist_r = hist_n = view = view_r = None
    hd_r = hi_r = None
    fetched_elsewhere = False
    for k, (rgb_d, rgb_i, feat, v, motion) in enumerate(split_ref.chain_frames(with_motion=True)):
        assert (motion[..., 3] == 1).sum() == 18 * 8 and not motion[:, 30:32, 4:7].any()
        ref = split_ref.accumulate_split(rgb_d, rgb_i, feat, view_r, hist_r, motion=motion, direct=D, indirect=I, demodulate=0)
        hd_r, sd_r, vd_r = motion_ref.accumulate(rgb_d, feat, motion, view_r, hd_r, demodulate=0, **D)
        hi_r, si_r, vi_r = motion_ref.accumulate(rgb_i, feat, motion, view_r, hi_r, demodulate=0, **I)
        hist_r, view_r = ref[0], v
        got, hist_t = _fused_three_ways(fray, k, "motion chain", rgb_d, rgb_i, feat, view, hist, hist_t, motion, D, I, dict(demodulate=0))
        for name, a, b in zip(NAMES, got, ref):
            _same("motion chain frame %d %s, host entry against the restatement" % (k, name), a, b)
        parts = fray.split_history_parts(got[0])
        for name, a, b in zip(("direct history", "indirect history", "signal_direct", "signal_indirect", "variance_direct", "variance_indirect"),
                              parts + got[1:], (hd_r, hi_r, sd_r, si_r, vd_r, vi_r)):
            _same("motion chain frame %d %s against motion_ref.accumulate" % (k, name), a, b)
        # a motion frame that moves nothing: every bit of the motion=None call
        still = np.zeros_like(motion)
        still[..., 0:3], still[..., 4:7] = feat[..., 0:3], feat[..., 3:6]
        a = fray.temporal_accumulate_split(rgb_d, rgb_i, feat, view, hist_n, motion=still, direct=D, indirect=I, demodulate=0)
        b = fray.temporal_accumulate_split(rgb_d, rgb_i, feat, view, hist_n, direct=D, indirect=I, demodulate=0)
        for name, x, y in zip(NAMES, a, b):
            _same("frame %d %s, a still motion frame against none" % (k, name), x, y)
        hist_n = b[0]
        hist, view = got[0], _view(abi, v)
        fetched_elsewhere = fetched_elsewhere or bool((hist[..., 15] != hist_n[..., 15]).any())
    assert fetched_elsewhere                        # and the moved columns did fetch another history in some frame


# ---- 3. rendered ------------------------------------------------------------------------------------------------------------------------------------
def test_rendered_cornell(fray, abi, gpu):
    W, H, seed = 131, 77, 5
    cams = [(0.0, (0, 0, 0)), (2.0, (0, 0, 0)), (2.0, (5.0, 0.0, 0.0))]          # test_accumulate_matches_restatement_cornell's
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4)
    s.beginRender()
    base = abi.Camera.from_buffer_copy(s.camera)
    frames = []
    for k, (yaw, move) in enumerate(cams):
        cam = abi.Camera.from_buffer_copy(base)
        cam.yaw += yaw
        for i in range(3):
            cam.pos[i] += move[i]
        _set_camera(s, cam)
        rgb_d, rgb_i, _state = s.render_components(4, seed=seed + k, noise=False)
        frames.append((rgb_d, rgb_i, s.render_features(4, seed=seed + k), fray.view_from_camera(cam, W, H)))
    s.close()
    D, I = dict(max_history=3), {}
    hist = hist_t = hist_r = view = None
    for k, (rgb_d, rgb_i, feat, v) in enumerate(frames):
        ref = split_ref.accumulate_split(rgb_d, rgb_i, feat, view, hist_r, direct=D, indirect=I)
        hist_r = ref[0]
        got, hist_t = _fused_three_ways(fray, k, "cornell", rgb_d, rgb_i, feat, view, hist, hist_t, None, D, I, {})
        for name, a, b in zip(NAMES, got, ref):
            _same("cornell frame %d %s, host entry against the restatement" % (k, name), a, b)
        hist, view = got[0], v
    ND, NI = hist[..., 3], hist[..., 15]
    print("cornell: N_D max %.3f, N_I max %.3f, %d pixels with N = 1, %d with N_D != N_I" % (ND.max(), NI.max(), int((NI == 1).sum()), int((ND != NI).sum())))
    assert NI.max() > 2.5 and (NI == 1).any() and (ND == 1).any() and ND.max() <= 3


# ---- 4. composition ---------------------------------------------------------------------------------------------------------------------------------
KEYS = ("features_frame", "history", "direct", "indirect", "direct_rgb", "indirect_rgb", "signal_direct", "signal_indirect", "variance_direct",
        "variance_indirect")


def _move(fray, s, node, d):
    T = fray.Transform(s.nodes[node])
    T.translate(*d)
    T.store(s.nodes[node])
    s.update()


@pytest.mark.parametrize("edited", [False, True])
def test_render_sequence_split_composition(fray, abi, gpu, edited):
    W, H, seed = 100, 70, 7
    d = (-36.0, -24.0, -24.0)
    tparams = dict(plane_tolerance=0.03)
    tdirect, tindirect = dict(max_history=4, alpha_min=0.2), dict(variance_history=3)
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4)
    s.beginRender()
    start = abi.Camera.from_buffer_copy(s.camera)
    cams = []
    for k in range(3):
        c = abi.Camera.from_buffer_copy(start)
        c.yaw += 1.5 * k
        cams.append(c)
    edit = (lambda _k, scene: _move(fray, scene, 5, d)) if edited else None
    frames = []
    for out, raw, info in s.render_sequence(cams, seed=seed, feature_samples=2, temporal=tparams, edit=edit, split=True, temporal_direct=tdirect,
                                            temporal_indirect=tindirect, levels=3):
        assert out.is_cuda and raw.is_cuda and info["film_offset"] == 0.5 and tuple(info["history"].shape) == (H, W, 20)
        assert ("motion" in info) == edited and "denoise" not in info
        assert info["params_direct"]["max_history"] == 4 and info["params_indirect"]["max_history"] == 32
        assert info["params_direct"]["variance_history"] == 4 and info["params_indirect"]["variance_history"] == 3
        for key in ("render", "features", "temporal", "denoise_direct", "denoise_indirect"):
            assert info[key]["ms_kernels"] > 0, key
        frames.append((out.cpu().numpy(), raw.cpu().numpy(), {key: info[key].cpu().numpy() for key in KEYS + (("motion",) if edited else ())}))
    assert len(frames) == 3 and bytes(s.camera) == bytes(start)
    s.close()
    # by hand, from the public pieces, on the same states of the scene
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4)
    s.beginRender()
    hd = hi = view = None
    for k, cam in enumerate(cams):
        _set_camera(s, cam)
        motion = None
        if edited:
            prev = s.node_transforms()
            if k:
                _move(fray, s, 5, d)
            feat, motion = s.render_features_motion(prev, 2, seed=seed + k)
        else:
            feat = s.render_features(2, seed=seed + k)
        state = tuple(fray.Accumulation.empty((W, H), seed + k, device="cuda") for _ in range(2))
        rgb_d, rgb_i, _state = s.render_components(4, state, seed=seed + k)
        rgb_d, rgb_i = rgb_d.cpu().numpy(), rgb_i.cpu().numpy()
        hd, sig_d, var_d = fray.temporal_accumulate(rgb_d, feat, view, hd, motion=motion, film_offset=0.5, **dict(tparams, **tdirect))
        hi, sig_i, var_i = fray.temporal_accumulate(rgb_i, feat, view, hi, motion=motion, film_offset=0.5, **dict(tparams, **tindirect))
        out_d = fray.denoise_signal(sig_d, var_d, feat, levels=3)
        out_i = fray.denoise_signal(sig_i, var_i, feat, levels=3)
        view = fray.view_from_camera(cam, W, H)
        want = dict(features_frame=feat, history=fray.join_history_parts(hd, hi), direct=out_d, indirect=out_i, direct_rgb=rgb_d, indirect_rgb=rgb_i,
                    signal_direct=sig_d, signal_indirect=sig_i, variance_direct=var_d, variance_indirect=var_i)
        if edited:
            want["motion"] = motion
        for key, w in want.items():
            _same("frame %d info[%r]" % (k, key), frames[k][2][key], w)
        _same("frame %d picture" % k, frames[k][0], out_d + out_i)
        _same("frame %d raw" % k, frames[k][1], rgb_d + rgb_i)
    if edited:
        assert (frames[2][2]["motion"][..., 3] == 1).any()
    s.close()


def test_render_sequence_split_defaults(fray, abi, gpu):
    s = open_scene(fray, "cornell_box.fray", 64, 48, numPaths=2)
    s.beginRender()
    cam = abi.Camera.from_buffer_copy(s.camera)
    want = {k: getattr(fray.temporal_params(), k) for k, _ in abi.Temporal._fields_}
    _, _, info = next(s.render_sequence([cam], split=True))
    assert info["params_indirect"] == want and want["max_history"] == 32
    assert info["params_direct"] == dict(want, max_history=8)          # the maintainer's choice for direct light ("split sequences")
    _, _, info = next(s.render_sequence([cam], split=True, temporal=dict(max_history=5)))          # temporal= still sets both
    assert info["params_direct"]["max_history"] == info["params_indirect"]["max_history"] == 5
    _, _, info = next(s.render_sequence([cam], split=True, temporal=dict(max_history=5), temporal_direct=dict(max_history=2)))
    assert (info["params_direct"]["max_history"], info["params_indirect"]["max_history"]) == (2, 5)
    s.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_render_sequence_split_refusals(fray, abi, gpu):
    for over, words in ((dict(gi=0, wantAA=0), "path-traced"), (dict(numPaths=4, stereoSeparation=12.0), "stereo")):
        s = open_scene(fray, "cornell_box.fray", 64, 48, **over)
        s.beginRender()
        start = abi.Camera.from_buffer_copy(s.camera)
        turned = abi.Camera.from_buffer_copy(start)
        turned.yaw += 3.0
        rendered = []
        with pytest.raises(fray.FrayError, match=words) as e:
            next(s.render_sequence([turned], split=True, edit=lambda k, scene: rendered.append(k)))
        assert e.value.code == abi.E_UNSUPPORTED and not rendered
        assert bytes(s.camera) == bytes(start)
        s.close()
    s = open_scene(fray, "cornell_box.fray", 64, 48, numPaths=2)
    s.beginRender()
    start = abi.Camera.from_buffer_copy(s.camera)
    with pytest.raises(ValueError, match="demodulate"):
        next(s.render_sequence([start], split=True, temporal=dict(demodulate=0)))
    with pytest.raises(ValueError, match="demodulate"):
        next(s.render_sequence([start], split=True, temporal_indirect=dict(demodulate=0), demodulate=1))
    with pytest.raises(ValueError, match="plane_tolerance"):
        next(s.render_sequence([start], split=True, temporal_direct=dict(plane_tolerance=0.5)))
    with pytest.raises(TypeError):
        next(s.render_sequence([start], split=True, temporal_direct=dict(alpha=1)))
    with pytest.raises(ValueError, match="split=True"):
        next(s.render_sequence([start], temporal_direct=dict(max_history=2)))
    assert bytes(s.camera) == bytes(start)
    s.close()
