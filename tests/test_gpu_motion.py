"""Motion frames on the GPU (include/frayhip.h "motion frames"):
1. the motion frame of a moved node against the numpy restatement on the query entry's hit records (tests/motion_ref.py), bit for bit, with the
   feature frame unchanged; the counting variant and the device entry;
2. nothing moved: the motion frame repeats the feature frame, and accumulating through it is accumulating without it, bit for bit;
3. several samples: the share of moved samples, P' against P - d within the FP32 budget, bucket subsets;
4. the accumulation through a motion frame against the restatement, bit for bit, with a moving node and a turning camera;
5. the point of it: a moved node's pixels keep their history through Scene.render_sequence(edit=...), and lose it in today's sequence;
6. refusals, and 7. a motion call leaves the scene as it found it."""
import ctypes as C
import os

import numpy as np
import pytest

import motion_ref
from conftest import ROOT, open_scene
from test_gpu_denoise import FIGURES

pytestmark = pytest.mark.gpu
F = np.float32
PLAIN = dict(gi=0, wantAA=0, dof=0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _report(what, got, ref):
    """Equal in every bit, with the first differing value in the message when not."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == F, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.argwhere(_bits(got) != _bits(ref))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d values differ, first at %s: library %r, expected %r" % (what, len(bad), got.size, i, got[i], ref[i]))


def _set_camera(s, cam):
    C.memmove(C.byref(s.desc.camera), C.byref(cam), C.sizeof(cam))
    s.beginFrame()


def _turned(abi, base, yaw):
    c = abi.Camera.from_buffer_copy(base)
    c.yaw += yaw
    return c


def _move(fray, s, node, steps):
    """Applies Transform steps [(name, args)] on top of the node's transform and pushes the edit."""
    T = fray.Transform(s.nodes[node])
    for name, args in steps:
        getattr(T, name)(*args)
    T.store(s.nodes[node])
    s.update()


# ---- 1. pinned, bit for bit ------------------------------------------------------------------------------------------------------------------------
ROT_TRANS = [("rotate", (7.0, -3.0, 2.0)), ("translate", (0.1, -1.0 / 3.0, 0.7))]          # 0.1, 1/3 and 0.7 have no FP64 representation
PINNED = {
    "cornell": ("cornell_box.fray", 67, 45, 5, [("rotate", (5.0, 0.0, 0.0)), ("translate", (8.1, 1.0 / 3.0, -4.7))]),
    "boxed": ("boxed.fray", 160, 120, None, None),
    "forest": ("forest.fray", 96, 64, 1, [("scale", (1.1, 0.9, 1.05))] + ROT_TRANS),        # node 1: a KD mesh (5332 triangles)
    "csg_nested": (os.path.join(ROOT, "tests", "scenes", "csg_nested.fray"), 96, 64, 1, ROT_TRANS),      # node 1: `a`
}


def _pinned_scene(fray, key):
    name, W, H, node, steps = PINNED[key]
    s = open_scene(fray, name, W, H, **PLAIN)
    s.beginRender()
    prev = s.node_transforms()
    if node is not None:
        _move(fray, s, node, steps)
    return s, prev, node


def _expected_motion(s, prev):
    """(motion float32 [H, W, 8] from the query entry's hit records, the mask of pixels whose normal the record holds as the feature pass does)."""
    o, d = s.camera_rays()
    r = s.trace_rays(o, d, record=True)
    ref = motion_ref.motion_from_hits(r["hit_id"], r["hit_rec"], s.node_transforms(), prev).astype(F)
    bump = np.array([n.bump_tex for n in s.nodes] + [-1], np.int32)
    ids = r["hit_id"]
    no_bump = bump[np.where(ids >= 0, ids, len(bump) - 1)] < 0
    return ref, no_bump, ids


@pytest.mark.parametrize("key", sorted(PINNED))
def test_motion_frame_matches_restatement(fray, abi, gpu, key):
    s, prev, node = _pinned_scene(fray, key)
    H, W = s.frame_size[1], s.frame_size[0]
    ref, no_bump, ids = _expected_motion(s, prev)
    feat, motion = s.render_features_motion(prev, 1)
    plain = s.render_features(1)
    s.close()
    assert motion.shape == (H, W, abi.MOTION_CHANNELS) and np.isfinite(motion).all()
    n_moved = int((ids == node).sum()) if node is not None else 0
    print("%s: %d pixels hit the moved node, %d a bump-mapped one, %d missed" % (key, n_moved, int((~no_bump).sum()), int((ids == -1).sum())))
    if node is not None:
        assert n_moved > 50 and (ids[ids >= 0] != node).any()
        # the moved node's P' differs from its P: the test sees the transform
        assert np.any(motion[ids == node][:, 0:3] != feat[ids == node][:, 0:3])
    else:
        assert (~no_bump).any() and not motion[..., 3].any()
    _report(key + " feat", feat, plain)
    _report(key + " P'", motion[..., 0:3], ref[..., 0:3])
    _report(key + " moved", motion[..., 3], ref[..., 3])
    _report(key + " channel 7", motion[..., 7], ref[..., 7])
    _report(key + " n'", motion[..., 4:7][no_bump], ref[..., 4:7][no_bump])
    assert np.array_equal(motion[..., 3] == 1, ids == node if node is not None else np.zeros((H, W), bool))
    # an unmoved pixel's rows repeat the feature frame's position and normal, bump-mapped or not
    still = motion[..., 3] == 0
    _report(key + " unmoved P'", motion[still][:, 0:3], feat[still][:, 0:3])
    _report(key + " unmoved n'", motion[still][:, 4:7], feat[still][:, 3:6])


def test_counting_variant(fray, abi, gpu):
    s, prev, node = _pinned_scene(fray, "forest")
    feat, motion = s.render_features_motion(prev, 1)
    feat_c, motion_c, st = s.render_features_motion(prev, 1, stats=True)
    _, st_plain = s.render_features(1, stats=True)
    s.close()
    _report("counting variant feat", feat_c, feat)
    _report("counting variant motion", motion_c, motion)
    counters = [k for k, v in st_plain.items() if isinstance(v, int) and not k.startswith("ms_")]
    assert any(st_plain[k] > 0 for k in counters) and st["samples"] == st_plain["samples"] == 96 * 64
    assert {k: st[k] for k in counters} == {k: st_plain[k] for k in counters}


def test_device_entry(fray, abi, gpu):
    import torch
    s, prev, node = _pinned_scene(fray, "csg_nested")
    W, H = s.frame_size
    feat, motion = s.render_features_motion(prev, 1)
    # sentinels: every pixel of a full call is written
    d_feat = torch.full((H, W, abi.FEAT_CHANNELS), 7.0, dtype=torch.float32, device="cuda")
    d_motion = torch.full((H, W, abi.MOTION_CHANNELS), 7.0, dtype=torch.float32, device="cuda")
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=0, bucket_stride=1)
    st = abi.Stats()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rc = fray.lib.frayhip_render_features_motion_device(s._dev, C.byref(fr), 1, prev, len(prev), d_feat.data_ptr(), d_motion.data_ptr(),
                                                            C.c_void_p(stream.cuda_stream), C.byref(st))
    assert rc == abi.OK, fray.lib.frayhip_last_error()
    s.close()
    assert st.ms_kernels > 0 and st.samples == W * H
    _report("device entry feat", d_feat.cpu().numpy(), feat)
    _report("device entry motion", d_motion.cpu().numpy(), motion)


# ---- 2. nothing moved --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box.fray", "smallpt.fray"])
def test_nothing_moved(fray, abi, gpu, name):
    W, H = 150, 100
    s = open_scene(fray, name, W, H, gi=1, numPaths=8)
    s.beginRender()
    base = abi.Camera.from_buffer_copy(s.camera)
    hist = hist_m = view = None
    for k, yaw in enumerate((0.0, 1.5, 3.0)):
        cam = _turned(abi, base, yaw)
        _set_camera(s, cam)
        rgb, _ = s.render(seed=11 + k)
        feat, motion = s.render_features_motion(s.node_transforms(), 4, seed=11 + k)
        _report("feat", feat, s.render_features(4, seed=11 + k))
        _report("P' == P", motion[..., 0:3], feat[..., 0:3])
        _report("n' == n", motion[..., 4:7], feat[..., 3:6])
        assert not motion[..., 3].any() and not motion[..., 7].any()
        a = fray.temporal_accumulate(rgb, feat, view, hist)
        b = fray.temporal_accumulate(rgb, feat, view, hist_m, motion=motion)
        for what, x, y in zip(("hist_out", "signal", "variance"), a, b):
            _report("%s frame %d %s" % (name, k, what), y, x)
        hist, hist_m = a[0], b[0]
        view = fray.view_from_camera(cam, W, H)
    s.close()
    assert hist[..., 3].max() > 2.5 and (hist[..., 3] == 1).any()


# ---- 3. several samples ------------------------------------------------------------------------------------------------------------------------------
def test_several_samples_and_buckets(fray, abi, gpu):
    W, H, n = 150, 100, 4
    d = np.array([8.0, 0.0, -4.0])
    s = open_scene(fray, "cornell_box.fray", W, H, gi=1, numPaths=8)
    s.beginRender()
    prev = s.node_transforms()
    _move(fray, s, 5, [("translate", tuple(d))])
    assert list(s.nodes[5].T.m) == list(s.nodes[5].T.invM) == [1, 0, 0, 0, 1, 0, 0, 0, 1]      # each sample's P' is ip - d, one FP64 rounding
    feat, motion = s.render_features_motion(prev, n, seed=3)
    _report("feat", feat, s.render_features(n, seed=3))
    moved = motion[..., 3]
    k = moved * F(n)
    assert np.array_equal(k, np.round(k)) and np.array_equal(moved, (k / F(n)).astype(F)) and k.min() == 0 and k.max() == n
    assert set(np.unique(k)) > {0.0, float(n)}, "no pixel with some samples on the block and some off it"
    full = moved == 1
    M = float(np.abs(feat[..., 0:3]).max() + np.abs(d).max())
    err = np.abs(motion[..., 0:3].astype(np.float64) - (feat[..., 0:3].astype(np.float64) - d))[full]
    print("several samples: %d pixels wholly on the moved node, |P' - (P - d)| max %.3g, bound %.3g (M = %.1f)" % (int(full.sum()), err.max(), 2.0 ** -20 * M, M))
    assert full.sum() > 200 and err.max() <= 2.0 ** -20 * M
    _report("unmoved P'", motion[k == 0][:, 0:3], feat[k == 0][:, 0:3])
    # n' = (norm * I) * I: the values of norm (a -0 component comes back as +0: (-0 * 1 + y * 0) + z * 0)
    assert np.array_equal(motion[..., 4:7][full], feat[..., 3:6][full])
    # bucket subsets: the others' pixels keep their sentinels, and the three together are the full call
    nb = fray.lib.frayhip_bucket_count(W, H, 0, 1)
    assert nb == 12
    f1, m1 = np.full((H, W, 10), -5.0, F), np.full((H, W, 8), -6.0, F)
    s.render_features_motion(prev, n, seed=3, bucket_first=1, bucket_stride=3, out=(f1, m1))
    own = np.zeros((H, W), bool)
    for b in range(1, nb, 3):
        bx, by = C.c_int(), C.c_int()
        fray.lib.frayhip_bucket_xy(W, H, b, C.byref(bx), C.byref(by))
        own[by.value * 48:(by.value + 1) * 48, bx.value * 48:(bx.value + 1) * 48] = True
    assert own.any() and not own.all()
    assert np.all(f1[~own] == -5.0) and np.all(m1[~own] == -6.0)
    _report("subset feat", f1[own], feat[own])
    _report("subset motion", m1[own], motion[own])
    for first in (0, 2):
        s.render_features_motion(prev, n, seed=3, bucket_first=first, bucket_stride=3, out=(f1, m1))
    s.close()
    _report("three subsets feat", f1, feat)
    _report("three subsets motion", m1, motion)


# ---- 4. accumulation, pinned ---------------------------------------------------------------------------------------------------------------------------
def _motion_chain(fray, abi, name, W, H, over, node, step, yaws, seed, params):
    """A chain with a moving node AND a turning camera: library (host entry) against the restatement; returns the frames."""
    s = open_scene(fray, name, W, H, **over)
    s.beginRender()
    base = abi.Camera.from_buffer_copy(s.camera)
    n = min(4, s.samples_per_pixel())
    frames = []
    for k, yaw in enumerate(yaws):
        cam = _turned(abi, base, yaw)
        _set_camera(s, cam)
        prev = s.node_transforms()
        if k:
            _move(fray, s, node, step)
        rgb, _ = s.render(seed=seed + k)
        feat, motion = s.render_features_motion(prev, n, seed=seed + k)
        frames.append((rgb, feat, motion, fray.view_from_camera(cam, W, H)))
    s.close()
    hist = hist_r = view = None
    for k, (rgb, feat, motion, v) in enumerate(frames):
        hist, sig, var = fray.temporal_accumulate(rgb, feat, view, hist, motion=motion, **params)
        hist_r, sig_r, var_r = motion_ref.accumulate(rgb, feat, motion, view, hist_r, **params)
        _report("%s frame %d hist_out" % (name, k), hist, hist_r)
        _report("%s frame %d signal" % (name, k), sig, sig_r)
        _report("%s frame %d variance" % (name, k), var, var_r)
        if k:
            # device-only cross-check: the motion kernel on (feat, motion) is the plain kernel on a feature frame that holds P' and n'
            feat2 = feat.copy()
            feat2[..., 0:3], feat2[..., 3:6] = motion[..., 0:3], motion[..., 4:7]
            h2, s2, _ = fray.temporal_accumulate(rgb, feat2, view, hist_in, **params)
            _report("cross-check acc, N", hist[..., 0:4], h2[..., 0:4])
            _report("cross-check m1", hist[..., 7], h2[..., 7])
            _report("cross-check m2", hist[..., 11], h2[..., 11])
            _report("cross-check signal", sig, s2)
            mv = motion[..., 3] == 1
            print("%s frame %d: %d moved pixels, %.1f %% of them found history (N > 1), %.1f %% of all pixels with a normal"
                  % (name, k, int(mv.sum()), 100.0 * (hist[..., 3][mv] > 1).mean(), 100.0 * (hist[..., 3][np.any(hist[..., 8:11] != 0, axis=2)] > 1).mean()))
            assert mv.sum() > 30 and (hist[..., 3][mv] > 1).mean() > 0.5
        hist_in = hist
        view = v
    return hist


@pytest.mark.parametrize("demodulate", [1, 0])
def test_accumulate_motion_matches_restatement_cornell(fray, abi, gpu, demodulate):
    hist = _motion_chain(fray, abi, "cornell_box.fray", 131, 77, dict(numPaths=4), 5, [("rotate", (4.0, 0.0, 0.0)), ("translate", (-30.1, 20.3, -25.7))],
                         (0.0, 1.5, 3.0), 5, dict(demodulate=demodulate))
    assert hist[..., 3].max() > 2.5 and (hist[..., 3] == 1).any()


def test_accumulate_motion_matches_restatement_forest(fray, abi, gpu):
    hist = _motion_chain(fray, abi, "forest.fray", 131, 77, PLAIN, 1, ROT_TRANS, (0.0, 1.0, 2.0), 9, dict(film_offset=0.0))
    assert hist[..., 3].max() > 2.5


# ---- 5. the point of it ----------------------------------------------------------------------------------------------------------------------------------
def test_moved_node_keeps_its_history(fray, abi, gpu):
    """Six frames of cornell_box, the short block (a mirror) translated by d each frame, the camera still.  d's component along each of the three
    visible faces' normals exceeds plane_tolerance * |P - pos|, so today's sequence REJECTS the faces' history (it does not smear it) and the
    moved pixels restart every frame; through the motion frame they keep counting.  The figures it prints belong in
    profiles/motion/README.md."""
    import torch
    W, H, K = 160, 120, 6
    d = (-36.0, -24.0, -24.0)           # down, so that the top face stays below the camera's eye level and in view
    tol = fray.temporal_params().plane_tolerance

    def step(scene):
        _move(fray, scene, 5, [("translate", d)])

    # through render_sequence(edit=...)
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4)
    s.beginRender()
    cam = abi.Camera.from_buffer_copy(s.camera)
    moved_any = np.zeros((H, W), bool)
    for k, (out, raw, info) in enumerate(s.render_sequence([cam] * K, seed=21, edit=lambda _k, scene: step(scene))):
        assert "motion" in info
        moved_any |= info["motion"][..., 3].cpu().numpy() > 0
    N_motion = info["history"][..., 3].cpu().numpy()
    motion = info["motion"].cpu().numpy()
    feat = info["features_frame"].cpu().numpy()
    out_motion = out.cpu().numpy()
    # today's calls on the same states of the scene
    s.close()
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4)
    s.beginRender()
    hist = view = None
    for k in range(K):
        if k:
            step(s)
        rgb, _ = s.render(seed=21 + k)
        f = s.render_features(4, seed=21 + k)
        hist, sig, var = fray.temporal_accumulate(rgb, f, view, hist)
        view = fray.view_from_camera(s.camera, W, H)
    out_static = fray.denoise_signal(sig, var, f)
    _report("the same last feature frame", feat, f)
    N_static = hist[..., 3]
    # the 1024-spp frame of the last state
    s.settings.numPaths = 1024
    s.beginFrame()
    truth, _ = s.render(seed=99)
    s.close()

    mv = motion[..., 3] == 1
    # both sides of the condition, per moved pixel whose samples all lie on one face (a unit mean normal)
    nrm = feat[..., 3:6].astype(np.float64)
    one_face = mv & (np.abs(np.linalg.norm(nrm, axis=2) - 1) < 1e-6)
    pos = np.array(list(cam.pos))
    along = np.abs(nrm[one_face] @ np.array(d))
    reach = tol * np.linalg.norm(feat[..., 0:3][one_face].astype(np.float64) - pos, axis=1)
    faces = np.unique(np.round(nrm[one_face], 3), axis=0)
    print("moved pixels %d (on one face %d, %d faces); |d . n| min %.2f against plane_tolerance * |P - pos| max %.2f"
          % (int(mv.sum()), int(one_face.sum()), len(faces), along.min(), reach.max()))
    assert len(faces) == 3 and along.min() > reach.max()
    share_motion = float((N_motion[mv] >= 3).mean())
    share_static = float((N_static[mv] >= 3).mean())
    rms = lambda img: float(np.sqrt(((img[mv].astype(np.float64) - truth[mv]) ** 2).mean()))
    print("share of moved pixels with N >= 3: %.3f with the motion frame, %.3f without; RMS of the denoised frame against 1024 spp over them: %.4f with, "
          "%.4f without" % (share_motion, share_static, rms(out_motion), rms(out_static)))
    assert mv.sum() > 300 and share_motion > share_static
    # static pixels far from the node: never moved, and eight pixels clear of every footprint -- the same count either way
    t = torch.from_numpy(moved_any[None, None].astype(np.float32))
    near = torch.nn.functional.max_pool2d(t, 17, 1, 8)[0, 0].numpy() > 0
    far = ~near
    assert far.sum() > W * H // 4
    assert np.array_equal(N_motion[far], N_static[far])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_alone(fray, abi, gpu):
    import torch
    L = fray.lib
    W, H = 64, 48
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4)
    s.beginRender()
    before, _ = s.render(seed=4)
    prev = s.node_transforms()
    n = len(prev)
    buf = np.zeros(H * W * 18 + 64, F)
    feat, motion = buf[:H * W * 10], buf[H * W * 10:H * W * 18]
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=4, bucket_first=0, bucket_stride=1)

    def call(T=prev, count=n, f=feat.ctypes.data, m=motion.ctypes.data, samples=2):
        return L.frayhip_render_features_motion(s._dev, C.byref(fr), samples, T, count, f, m, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, (rc, L.frayhip_last_error())
        msg = L.frayhip_last_error().decode()
        assert words in msg and "frayhip_render_features_motion:" in msg, msg

    assert call() == abi.OK
    expect(call(count=n - 1), "n_prev")
    expect(call(count=n + 1), "n_prev")
    expect(call(T=None), "null prev_T")
    expect(call(m=None), "null motion")
    expect(call(samples=5), "n_samples")
    for field, i in (("offset", 1), ("m", 4), ("invM", 8)):
        for v in (np.nan, np.inf):
            bad = s.node_transforms()
            getattr(bad[3], field)[i] = v
            expect(call(T=bad), "non-finite")
    expect(call(m=feat.ctypes.data), "overlap")
    expect(call(m=feat.ctypes.data + 4 * (H * W * 10 - 1)), "overlap")
    expect(call(f=motion.ctypes.data + 4 * (H * W * 8 - 1)), "overlap")
    # the device entries: misaligned pointers
    d_feat = torch.zeros(H * W * 10 + 4, dtype=torch.float32, device="cuda")
    d_motion = torch.zeros(H * W * 8 + 4, dtype=torch.float32, device="cuda")
    rc = L.frayhip_render_features_motion_device(s._dev, C.byref(fr), 2, prev, n, d_feat.data_ptr(), d_motion.data_ptr() + 2, None, None)
    assert rc == abi.E_ARG and "aligned" in L.frayhip_last_error().decode()
    rgb_t, hist_t = torch.zeros(H, W, 3, device="cuda"), torch.zeros(H, W, 12, device="cuda")
    sig_t, var_t = torch.zeros(H, W, 3, device="cuda"), torch.zeros(H, W, device="cuda")
    prm = fray.temporal_params()
    assert d_motion.data_ptr() % 16 == 0
    for off in (4, 8):
        rc = L.frayhip_temporal_accumulate_motion_device(W, H, rgb_t.data_ptr(), d_feat.data_ptr(), d_motion.data_ptr() + off, None, None, C.byref(prm),
                                                         hist_t.data_ptr(), sig_t.data_ptr(), var_t.data_ptr(), None, None)
        assert rc == abi.E_ARG and "16-byte" in L.frayhip_last_error().decode()
    after, _ = s.render(seed=4)
    assert np.array_equal(before, after)
    s.close()
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4, maxTraceDepth=20)
    s.beginRender()
    assert L.frayhip_render_features_motion(s._dev, C.byref(fr), 1, prev, n, feat.ctypes.data, motion.ctypes.data, None) == abi.E_UNSUPPORTED
    assert "maxTraceDepth" in L.frayhip_last_error().decode()
    s.close()
    s = open_scene(fray, "boxed.fray", W, H, stereoSeparation=1.0)
    s.beginRender()
    T = s.node_transforms()
    assert L.frayhip_render_features_motion(s._dev, C.byref(fr), 1, T, len(T), feat.ctypes.data, motion.ctypes.data, None) == abi.E_UNSUPPORTED
    assert "stereo" in L.frayhip_last_error().decode()
    s.close()
    # maxTraceDepth < 0: all zeros, in both frames
    s = open_scene(fray, "cornell_box.fray", W, H, numPaths=4, maxTraceDepth=-1)
    s.beginRender()
    f, m = s.render_features_motion(s.node_transforms(), 2, out=(np.full((H, W, 10), 3.0, F), np.full((H, W, 8), 3.0, F)))
    assert not f.any() and not m.any()
    s.close()


# ---- 7. the scene is not changed -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,over", [("cornell_box.fray", dict(numPaths=4)), ("boxed.fray", {})])
def test_motion_call_changes_nothing_of_the_scene(fray, abi, gpu, name, over):
    W, H = 150, 100
    s = open_scene(fray, name, W, H, **over)
    s.beginRender()
    prev = s.node_transforms()
    _move(fray, s, 6, [("translate", (0.5, 0.25, -0.5))])
    img_before, _ = s.render(seed=9)
    before = {k: s.get_option(k) for k in FIGURES}
    n = min(4, s.samples_per_pixel())
    a = s.render_features_motion(prev, n, seed=9)
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and (a[1][..., 3] > 0).any()
    assert {k: s.get_option(k) for k in FIGURES} == before
    b = s.render_features_motion(prev, n, seed=9)
    _report("repeatable feat", b[0], a[0])
    _report("repeatable motion", b[1], a[1])
    img_after, _ = s.render(seed=9)
    assert np.array_equal(img_before, img_after)
    assert {k: s.get_option(k) for k in FIGURES} == before
    s.close()
