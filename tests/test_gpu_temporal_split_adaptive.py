"""Adaptive split accumulation on the GPU (include/frayhip.h "change frames", frayhip_temporal_accumulate_split_adaptive).  Every comparison is
of bit patterns:
1. the synthetic chain of tests/temporal_split_adaptive_ref.py, with and without the motion frame, demodulate 0 and 1: the host entry against
   the restatement, the device entry against the host entry, the fused outputs taken apart against two calls of the adaptive entry, change
   frames of +0 against the split entry and change frames of 1 against the first-frame call;
2. a change frame of +0 for one component and the mixed one for the other, both ways round: the untouched component is the split entry's;
3. the smallest shapes, 1 x 1 and 5 x 3, with change frames that hold every kind of value in turn;
4. Scene.render_sequence(split=True, change_samples=2) is the public pieces chained by hand with the unfused pair, and makes no
   split_history_parts, join_history_parts or temporal_accumulate call."""
import sys

import numpy as np
import pytest

import scene_edits
import temporal_split_adaptive_ref as ref
import temporal_split_ref as split_ref
from conftest import open_scene

pytestmark = pytest.mark.gpu
F = np.float32
NAMES = ref.NAMES
D, I = ref.CHAIN_DIRECT, ref.CHAIN_INDIRECT


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _bits(a):
    return np.ascontiguousarray(_np(a)).view(np.uint32)


def _same(what, got, want):
    """Equal bit patterns, with the first differing value in the message."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    i = tuple(bad[0])
    raise AssertionError("%s: %d of %d values differ, first at %s: %r against %r" % (what, len(bad), g.size, i, g.view(F)[i], w.view(F)[i]))


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=F, order="C")).cuda()          # a copy: the shared chain is read-only


def _view(abi, v):
    """An abi.View of the restatement's view dict (None stays None)."""
    if v is None:
        return None
    out = abi.View()
    for k in ("pos", "right", "up", "front"):
        for i in range(3):
            getattr(out, k)[i] = v[k][i]
    out.tan_x, out.tan_y, out.width, out.height = v["tan_x"], v["tan_y"], v["width"], v["height"]
    return out


# ---- 1. the synthetic chain ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_motion", [False, True])
@pytest.mark.parametrize("demodulate", [0, 1])
def test_chain(fray, abi, gpu, with_motion, demodulate):
    frames = ref.chain(with_motion, demodulate)
    pairs, count = ref.chain_coverage(frames)                              # what the restatement says these inputs exercise
    assert all(len(p) == 9 for p in pairs[1:]) and all(y > 0 and o > 0 for y, o in count.values()), (pairs, count)
    split = fray.temporal_accumulate_split
    hist = hist_t = None
    for k, fr in enumerate(frames):
        rgb_d, rgb_i, feat, motion, chg_d, chg_i = (fr[key] for key in ("rgb_d", "rgb_i", "feat", "motion", "chg_d", "chg_i"))
        view = _view(abi, fr["prev_view"])
        shape = rgb_d.shape[:2]
        kw = dict(motion=motion, direct=D, indirect=I, demodulate=demodulate)
        got = split(rgb_d, rgb_i, feat, view, hist, change_direct=chg_d, change_indirect=chg_i, **kw)
        for name, a, b in zip(NAMES, got, fr["ref"]):
            _same("chain frame %d %s, host entry against the restatement" % (k, name), a, b)
        dev = split(_cuda(rgb_d), _cuda(rgb_i), _cuda(feat), view, hist_t, change_direct=_cuda(chg_d), change_indirect=_cuda(chg_i),
                    **dict(kw, motion=_cuda(motion)))
        assert all(a.is_cuda for a in dev)
        for name, a, b in zip(NAMES, dev, got):
            _same("chain frame %d %s, device entry against host entry" % (k, name), a, b)
        # the fused outputs taken apart against two calls of the adaptive entry on the history's parts
        parts = fray.split_history_parts(got[0])
        hin = fray.split_history_parts(hist) if hist is not None else (None, None)
        for comp, rgb, chg, h_in, h_out, sig, var, prm in (("direct", rgb_d, chg_d, hin[0], parts[0], got[1], got[3], D),
                                                          ("indirect", rgb_i, chg_i, hin[1], parts[1], got[2], got[4], I)):
            two = fray.temporal_accumulate(rgb, feat, view, h_in, motion=motion, change=chg, demodulate=demodulate, **prm)
            for name, a, b in zip(("history", "signal", "variance"), (h_out, sig, var), two):
                _same("chain frame %d %s %s, fused against the adaptive entry" % (k, comp, name), a, b)
        # two change frames of +0 are the split entry, in every output bit; two of 1 are the first-frame call
        zero = split(rgb_d, rgb_i, feat, view, hist, change_direct=np.zeros(shape, F), change_indirect=np.zeros(shape, F), **kw)
        plain = split(rgb_d, rgb_i, feat, view, hist, **kw)
        one = split(rgb_d, rgb_i, feat, view, hist, change_direct=np.ones(shape, F), change_indirect=np.ones(shape, F), **kw)
        first = split(rgb_d, rgb_i, feat, None, None, **kw)
        for name, a, b, c, d in zip(NAMES, zero, plain, one, first):
            _same("chain frame %d %s, change frames of +0 against the split entry" % (k, name), a, b)
            _same("chain frame %d %s, change frames of 1 against hist_in = NULL" % (k, name), c, d)
        hist, hist_t = got[0], dev[0]


# ---- 2. one component untouched ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_motion", [False, True])
def test_one_component_untouched(fray, abi, gpu, with_motion):
    """A swapped index between the components' change frames, parameters or rows shows here: the component whose change frame is +0 keeps the
    split entry's bits while the other one moves."""
    split = fray.temporal_accumulate_split
    moved = {"direct": 0, "indirect": 0}
    for k, fr in enumerate(ref.chain(with_motion, 0)):
        view = _view(abi, fr["prev_view"])
        shape = fr["rgb_d"].shape[:2]
        ins = (fr["rgb_d"], fr["rgb_i"], fr["feat"], view, fr["hist_in"])
        kw = dict(motion=fr["motion"], direct=D, indirect=I, demodulate=0)
        plain = split(*ins, **kw)
        pd, pi = fray.split_history_parts(plain[0])
        zero = np.zeros(shape, F)
        for touched, cd, ci in (("direct", fr["chg_d"], zero), ("indirect", zero, fr["chg_i"])):
            got = split(*ins, change_direct=cd, change_indirect=ci, **kw)
            want = ref.accumulate_split_adaptive(fr["rgb_d"], fr["rgb_i"], fr["feat"], cd, ci, fr["prev_view"], fr["hist_in"], **kw)
            for name, a, b in zip(NAMES, got, want):
                _same("frame %d, only %s changed, %s against the restatement" % (k, touched, name), a, b)
            gd, gi = fray.split_history_parts(got[0])
            if touched == "direct":
                same = ((gi, pi), (got[2], plain[2]), (got[4], plain[4]))
                other = got[1], plain[1]
            else:
                same = ((gd, pd), (got[1], plain[1]), (got[3], plain[3]))
                other = got[2], plain[2]
            for name, (a, b) in zip(("history", "signal", "variance"), same):
                _same("frame %d, only %s changed: the other component's %s against the split entry" % (k, touched, name), a, b)
            moved[touched] += int((_bits(other[0]) != _bits(other[1])).sum())
    assert moved["direct"] > 0 and moved["indirect"] > 0, moved


# ---- 3. the smallest shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (5, 3)])
def test_smallest_shapes(fray, abi, gpu, W, H):
    rng = np.random.default_rng(10 * W + H)
    feat, v = split_ref.plane_frame(W, H)
    view = _view(abi, v)
    split = fray.temporal_accumulate_split
    frames = [(rng.uniform(0.0, 1.0, (H, W, 3)).astype(F), rng.uniform(0.0, 2.0, (H, W, 3)).astype(F)) for _ in range(2)]
    for demodulate in (0, 1):
        kw = dict(direct=D, indirect=I, demodulate=demodulate)
        zero = np.zeros((H, W), F)
        h0 = split(frames[0][0], frames[0][1], feat, None, None, change_direct=zero, change_indirect=zero, **kw)
        want = ref.accumulate_split_adaptive(frames[0][0], frames[0][1], feat, zero, zero, **kw)
        for name, a, b in zip(NAMES, h0, want):
            _same("%dx%d frame 0 %s, host entry against the restatement" % (W, H, name), a, b)
        plain = split_ref.accumulate_split(frames[1][0], frames[1][1], feat, v, want[0], **kw)
        assert (plain[0][..., 3] > 1).all()                                # under the still camera every pixel fetches its history
        seen = set()
        for shift in range(len(ref.CHANGE_VALUES) if W * H < len(ref.CHANGE_VALUES) else 1):
            cd, ci = ref.cyclic_change_maps((H, W), shift)
            seen |= set(cd.view(np.uint32).ravel().tolist())
            got = split(frames[1][0], frames[1][1], feat, view, h0[0], change_direct=cd, change_indirect=ci, **kw)
            want1 = ref.accumulate_split_adaptive(frames[1][0], frames[1][1], feat, cd, ci, v, want[0], **kw)
            dev = split(_cuda(frames[1][0]), _cuda(frames[1][1]), _cuda(feat), view, _cuda(h0[0]), change_direct=_cuda(cd), change_indirect=_cuda(ci), **kw)
            for name, a, b, c in zip(NAMES, got, want1, dev):
                _same("%dx%d frame 1 shift %d %s, host entry against the restatement" % (W, H, shift, name), a, b)
                _same("%dx%d frame 1 shift %d %s, device entry against host entry" % (W, H, shift, name), c, a)
        assert seen == set(ref.CHANGE_VALUES.view(np.uint32).tolist())     # all eleven values


# ---- 4. render_sequence --------------------------------------------------------------------------------------------------------------------------
W4, H4, SEED, NPROBE, SPP, FRAMES, MOVE_AT = 64, 48, 42, 2, 8, 4, 2       # tests/test_gpu_change.py's sequence
INFO_KEYS = ("features_frame", "motion", "history", "direct", "indirect", "direct_rgb", "indirect_rgb", "signal_direct", "signal_indirect",
             "variance_direct", "variance_indirect", "change_direct", "change_indirect")


def _block_edit(fray, calls):
    def edit(k, scene):
        calls.append(k)
        if k == MOVE_AT:
            scene_edits.apply(fray, scene, scene_edits.CASES["cornell-block"]["edit"])
            scene.update()
    return edit


def _sequence(fray, abi):
    """The static-camera cornell sequence whose tall block moves before frame 2, split, with change_samples: [(out, raw, info as numpy)]."""
    s = open_scene(fray, "cornell_box.fray", W4, H4, numPaths=SPP)
    s.beginRender()
    start = abi.Camera.from_buffer_copy(s.camera)
    calls, frames = [], []
    for out, raw, info in s.render_sequence([start] * FRAMES, seed=SEED, edit=_block_edit(fray, calls), split=True, change_samples=NPROBE):
        assert info["temporal"]["ms_kernels"] > 0
        frames.append((_np(out), _np(raw), {k: (_np(info[k]) if info[k] is not None else None) for k in INFO_KEYS}))
    assert calls == [1, 2, 3] and len(frames) == FRAMES
    s.close()
    return frames


@pytest.fixture(scope="module")
def sequence(fray, abi, gpu):
    return _sequence(fray, abi)


def test_render_sequence_is_the_unfused_pieces(fray, abi, gpu, sequence):
    """Every array of the sequence against the public pieces chained by hand, frames k >= 1 with the UNFUSED pair on split_history_parts: what
    the sequence ran before it took the fused entry."""
    s = open_scene(fray, "cornell_box.fray", W4, H4, numPaths=SPP)
    s.beginRender()
    calls = []
    edit = _block_edit(fray, calls)
    tdirect, tindirect = dict(film_offset=0.5, max_history=8), dict(film_offset=0.5)         # render_sequence's defaults for a path-traced frame
    hist = view = None
    for k in range(FRAMES):
        seed = SEED + k
        s.beginFrame()                                                      # the camera stays; the sequence begins every frame so
        prev = s.node_transforms()
        probe = None
        if k:
            _, _, probe = s.render_components(NPROBE, seed=seed)
            edit(k, s)
        feat, motion = s.render_features_motion(prev, 4, seed=seed)
        chg_d = chg_i = None
        if k:
            _, _, state = s.render_components(NPROBE, seed=seed)
            first = [a.state.copy() for a in state]
            rgb_d, rgb_i, _ = s.render_components(SPP - NPROBE, state, seed=seed)
            chg_d = fray.change_frame(probe[0], first[0], motion)
            chg_i = fray.change_frame(probe[1], first[1], motion)
            hd, hi = fray.split_history_parts(hist)
            hd, sig_d, var_d = fray.temporal_accumulate(rgb_d, feat, view, hd, motion=motion, change=chg_d, **tdirect)
            hi, sig_i, var_i = fray.temporal_accumulate(rgb_i, feat, view, hi, motion=motion, change=chg_i, **tindirect)
            hist = fray.join_history_parts(hd, hi)
        else:
            rgb_d, rgb_i, _ = s.render_components(SPP, seed=seed)
            hist, sig_d, sig_i, var_d, var_i = fray.temporal_accumulate_split(rgb_d, rgb_i, feat, None, None, motion=motion, direct=tdirect,
                                                                              indirect=tindirect)
        out_d = fray.denoise_signal(sig_d, var_d, feat)
        out_i = fray.denoise_signal(sig_i, var_i, feat)
        view = fray.view_from_camera(s.camera, W4, H4)
        want = dict(features_frame=feat, motion=motion, history=hist, direct=out_d, indirect=out_i, direct_rgb=rgb_d, indirect_rgb=rgb_i,
                    signal_direct=sig_d, signal_indirect=sig_i, variance_direct=var_d, variance_indirect=var_i, change_direct=chg_d,
                    change_indirect=chg_i)
        got = sequence[k]
        for key in INFO_KEYS:
            if want[key] is None:
                assert got[2][key] is None, (k, key)
            else:
                _same("frame %d info[%r]" % (k, key), got[2][key], want[key])
        _same("frame %d picture" % k, got[0], out_d + out_i)
        _same("frame %d raw" % k, got[1], rgb_d + rgb_i)
    s.close()
    assert calls == [1, 2, 3]
    c2d, c2i = sequence[MOVE_AT][2]["change_direct"], sequence[MOVE_AT][2]["change_indirect"]
    assert c2d.any() and (c2d == 0).any() and c2i.any()                     # the edit did shorten histories, and not everywhere


def test_render_sequence_makes_no_unfused_call(fray, abi, gpu, sequence, monkeypatch):
    scene = sys.modules[fray.Scene.__module__]

    def refuse(name):
        def f(*a, **kw):
            raise AssertionError("render_sequence(split=True, change_samples=n) called %s" % name)
        return f
    for name in ("split_history_parts", "join_history_parts", "temporal_accumulate"):
        assert callable(getattr(scene, name))
        monkeypatch.setattr(scene, name, refuse(name))
    again = _sequence(fray, abi)
    for k in range(FRAMES):
        _same("frame %d picture" % k, again[k][0], sequence[k][0])
        _same("frame %d raw" % k, again[k][1], sequence[k][1])
        for key in INFO_KEYS:
            if sequence[k][2][key] is None:
                assert again[k][2][key] is None, (k, key)
            else:
                _same("frame %d info[%r]" % (k, key), again[k][2][key], sequence[k][2][key])
