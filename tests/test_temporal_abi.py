"""Temporal accumulation (include/frayhip.h "temporal accumulation"), what can be checked without a GPU: the six entries are exported and
mirrored, frayhip_view's and struct frayhip_temporal's layouts and the defaults match, every argument check answers FRAYHIP_E_ARG with the
entry's name before the device is touched, the Python side refuses mixed or mis-shaped inputs, the CLI lists its flags, the view that
frayhip_view_from_camera makes projects the oracle's camera rays back onto their film positions, and the numpy restatement
(tests/temporal_ref.py) behaves as the header says on synthetic inputs."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_ref
from conftest import ROOT, open_scene
from test_abi import header_functions

ENTRIES = ["frayhip_view_from_camera", "frayhip_temporal_defaults", "frayhip_temporal_accumulate", "frayhip_temporal_accumulate_device",
           "frayhip_denoise_signal", "frayhip_denoise_signal_device"]
F = np.float32


def test_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    for n in ("view_from_camera", "temporal_params", "temporal_accumulate", "denoise_signal"):
        assert callable(getattr(fray, n)), n
    assert callable(fray.Scene.render_sequence)


def test_structs_and_defaults(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_view") == C.sizeof(abi.View) == 64
    assert abi.STRUCTS["frayhip_view"] is abi.View
    assert (abi.View.right.offset, abi.View.front.offset, abi.View.tan_x.offset, abi.View.height.offset) == (12, 36, 48, 60)
    assert fray.lib.frayhip_sizeof(b"frayhip_temporal") == C.sizeof(abi.Temporal) == 28
    assert abi.Temporal.alpha_min.offset == 12 and abi.Temporal.normal_min_dot.offset == 24
    assert abi.HISTORY_CHANNELS == temporal_ref.HISTORY_CHANNELS == 12
    src = open(os.path.join(ROOT, "include", "frayhip.h")).read()
    assert "#define FRAYHIP_HISTORY_CHANNELS 12" in src
    p = abi.Temporal()
    assert fray.lib.frayhip_temporal_defaults(C.byref(p)) == abi.OK
    got = {k: getattr(p, k) for k, _ in abi.Temporal._fields_}
    assert got == {k: (F(v) if isinstance(v, float) else v) for k, v in temporal_ref.DEFAULTS.items()}
    assert (p.demodulate, p.max_history, p.variance_history) == (1, 32, 4)
    assert fray.lib.frayhip_temporal_defaults(None) == abi.E_ARG
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning
    q = fray.temporal_params(max_history=8, film_offset=0.0)
    assert (q.max_history, q.film_offset, q.variance_history) == (8, 0.0, 4)
    with pytest.raises(TypeError):
        fray.temporal_params(history=3)


def test_view_from_camera_argument_checks(fray, abi):
    L = fray.lib
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    v = abi.View()

    def call(cam="scene", w=64, h=48, out="view", **over):
        c = abi.Camera.from_buffer_copy(s.camera)
        for k, val in over.items():
            if k == "pos0":
                c.pos[0] = val
            else:
                setattr(c, k, val)
        return L.frayhip_view_from_camera(C.byref(c) if cam == "scene" else None, w, h, C.byref(v) if out == "view" else None)

    def expect(rc, words):
        assert rc == abi.E_ARG, rc
        msg = L.frayhip_last_error().decode()
        assert words in msg and "frayhip_view_from_camera:" in msg, msg

    assert call() == abi.OK and (v.width, v.height) == (64, 48)
    expect(call(cam=None), "null camera")
    expect(call(out=None), "null view")
    expect(call(w=0), "width and height")
    expect(call(h=-2), "width and height")
    for name in ("yaw", "pitch", "roll", "fov", "aspectRatio", "pos0"):
        expect(call(**{name: math.nan}), "finite")
        expect(call(**{name: math.inf}), "finite")
    for fov in (0.0, -10.0, 180.0, 200.0):
        expect(call(fov=fov), "fov")
    expect(call(aspectRatio=0.0), "aspectRatio")
    with pytest.raises(TypeError):
        fray.view_from_camera(s.settings, 64, 48)
    # stereo and DOF play no part
    a = fray.view_from_camera(s.camera, 64, 48)
    s.camera.stereoSeparation, s.camera.dof = 2.0, 1
    b = fray.view_from_camera(s.camera, 64, 48)
    assert bytes(a) == bytes(b)
    s.close()


@pytest.mark.parametrize("dev", [False, True])
def test_accumulate_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    rgb = np.zeros((H, W, 3), F)
    feat = np.zeros((H, W, 10), F)
    hin = np.zeros((H, W, 12), F)
    hout = np.zeros((H, W, 12), F)
    sig = np.zeros((H, W, 3), F)
    var = np.zeros((H, W), F)
    assert hin.ctypes.data % 16 == 0 and hout.ctypes.data % 16 == 0
    who = "frayhip_temporal_accumulate_device" if dev else "frayhip_temporal_accumulate"
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    view = fray.view_from_camera(s.camera, W, H)
    s.close()

    def call(w=W, h=H, r=rgb.ctypes.data, f=feat.ctypes.data, v="view", hi=hin.ctypes.data, p="default", ho=hout.ctypes.data, sg=sig.ctypes.data,
             va=var.ctypes.data, vw=None, **over):
        prm = abi.Temporal()
        L.frayhip_temporal_defaults(C.byref(prm))
        for k, val in over.items():
            setattr(prm, k, val)
        vv = abi.View.from_buffer_copy(view)
        for k, val in (vw or {}).items():
            if k == "pos0":
                vv.pos[0] = val
            else:
                setattr(vv, k, val)
        vp = C.byref(vv) if v == "view" else None
        pp = C.byref(prm) if p == "default" else None
        if dev:
            return L.frayhip_temporal_accumulate_device(w, h, r, f, vp, hi, pp, ho, sg, va, None, None)
        return L.frayhip_temporal_accumulate(w, h, r, f, vp, hi, pp, ho, sg, va, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, rc
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    expect(call(w=0), "width and height")
    expect(call(h=-1), "width and height")
    expect(call(w=1 << 16, h=1 << 15), "2^30")
    expect(call(r=None), "null rgb")
    expect(call(f=None), "null feat")
    expect(call(p=None), "null parameters")
    expect(call(ho=None), "null hist_out")
    expect(call(sg=None), "null signal")
    expect(call(va=None), "null variance")
    expect(call(v=None), "both")
    expect(call(hi=None), "both")
    expect(call(vw=dict(width=W + 1)), "size")
    expect(call(vw=dict(height=H - 1)), "size")
    expect(call(vw=dict(pos0=math.nan)), "non-finite")
    expect(call(vw=dict(tan_x=math.inf)), "non-finite")
    expect(call(vw=dict(tan_y=0.0)), "tan_x and tan_y")
    expect(call(demodulate=2), "demodulate")
    for n in (0, 4097):
        expect(call(max_history=n), "max_history")
        expect(call(variance_history=n), "variance_history")
    for x in (-0.1, 1.5, math.nan):
        expect(call(alpha_min=x), "alpha_min")
    for x in (math.nan, math.inf):
        expect(call(film_offset=x), "film_offset")
    for x in (-1.0, math.nan, math.inf):
        expect(call(plane_tolerance=x), "plane_tolerance")
    for x in (-1.5, 1.5, math.nan):
        expect(call(normal_min_dot=x), "normal_min_dot")
    # an output aliasing an input or another output, wholly or in part
    expect(call(ho=hin.ctypes.data), "overlap")
    expect(call(ho=hin.ctypes.data + 48), "overlap")
    expect(call(sg=rgb.ctypes.data), "overlap")
    expect(call(va=feat.ctypes.data + 40), "overlap")
    expect(call(sg=hout.ctypes.data + 16), "overlap")
    expect(call(va=sig.ctypes.data + 8), "overlap")
    if dev:
        expect(call(r=rgb.ctypes.data + 2), "aligned")
        expect(call(hi=hin.ctypes.data + 4), "16-byte")
        expect(call(ho=hout.ctypes.data + 8), "16-byte")


@pytest.mark.parametrize("dev", [False, True])
def test_denoise_signal_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    sig = np.zeros((H, W, 3), F)
    var = np.zeros((H, W), F)
    feat = np.zeros((H, W, 10), F)
    out = np.zeros((H, W, 3), F)
    who = "frayhip_denoise_signal_device" if dev else "frayhip_denoise_signal"

    def call(w=W, h=H, s=sig.ctypes.data, v=var.ctypes.data, f=feat.ctypes.data, p="default", o=out.ctypes.data, **over):
        prm = abi.Denoise()
        L.frayhip_denoise_defaults(C.byref(prm))
        for k, val in over.items():
            setattr(prm, k, val)
        pp = C.byref(prm) if p == "default" else None
        if dev:
            return L.frayhip_denoise_signal_device(w, h, s, v, f, pp, o, None, None)
        return L.frayhip_denoise_signal(w, h, s, v, f, pp, o, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, rc
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    expect(call(w=0), "width and height")
    expect(call(w=1 << 16, h=1 << 15), "2^30")
    expect(call(s=None), "null signal")
    expect(call(v=None), "null variance")
    expect(call(f=None), "null feat")
    expect(call(p=None), "null parameters")
    expect(call(o=None), "null out")
    expect(call(levels=0), "levels")
    expect(call(demodulate=-1), "demodulate")
    expect(call(sigma_depth=0.0), "sigma_depth")
    expect(call(sigma_normal=math.nan), "sigma_normal")
    expect(call(o=sig.ctypes.data), "overlap")
    expect(call(o=var.ctypes.data - 8), "overlap")
    expect(call(o=feat.ctypes.data + 40), "overlap")
    if dev:
        expect(call(v=var.ctypes.data + 2), "aligned")


def test_python_side_refuses_bad_inputs(fray, abi):
    rgb = np.zeros((4, 5, 3), F)
    feat = np.zeros((4, 5, 10), F)
    hist = np.zeros((4, 5, 12), F)
    var = np.zeros((4, 5), F)
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    view = fray.view_from_camera(s.camera, 5, 4)
    with pytest.raises(TypeError):
        fray.temporal_accumulate(rgb.astype(np.float64), feat)
    with pytest.raises(ValueError):
        fray.temporal_accumulate(rgb, feat[:, :4])
    with pytest.raises(ValueError):
        fray.temporal_accumulate(rgb, feat, view, hist[..., :11])
    with pytest.raises(ValueError, match="both"):
        fray.temporal_accumulate(rgb, feat, view, None)
    with pytest.raises(ValueError, match="both"):
        fray.temporal_accumulate(rgb, feat, None, hist)
    with pytest.raises(TypeError):
        fray.temporal_accumulate(rgb, feat, s.camera, hist)
    with pytest.raises(TypeError):
        fray.temporal_accumulate(rgb, feat, alpha=0.5)
    with pytest.raises(fray.FrayError, match="max_history"):
        fray.temporal_accumulate(rgb, feat, max_history=0)
    with pytest.raises(fray.FrayError, match="size"):
        fray.temporal_accumulate(rgb, feat, fray.view_from_camera(s.camera, 6, 4), hist)
    with pytest.raises(ValueError):
        fray.denoise_signal(rgb, var[:, :4], feat)
    with pytest.raises(ValueError):
        fray.denoise_signal(rgb, var[..., None], feat)
    with pytest.raises(TypeError):
        fray.denoise_signal(rgb, var.astype(np.float64), feat)
    with pytest.raises(fray.FrayError, match="levels"):
        fray.denoise_signal(rgb, var, feat, levels=11)
    if "torch" in sys.modules:
        import torch
        with pytest.raises(TypeError, match="mix"):
            fray.temporal_accumulate(torch.zeros(4, 5, 3), feat)
        with pytest.raises(TypeError, match="CPU tensor"):
            fray.denoise_signal(torch.zeros(4, 5, 3), torch.zeros(4, 5), torch.zeros(4, 5, 10))
    with pytest.raises(fray.FrayError, match="beginRender"):
        next(s.render_sequence([s.camera]))
    s.close()


def test_cli_lists_the_sequence_flags():
    env = dict(os.environ, FRAYHIP_NO_TORCH="1")
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr
    for flag in ("--frames", "--yaw-step"):
        assert flag in out.stdout, flag
    from fray_amd.__main__ import build_parser, sequence_path
    a = build_parser().parse_args(["scene.fray", "--denoise", "--frames", "8", "--yaw-step", "0.5"])
    assert a.denoise and a.frames == 8 and a.yaw_step == 0.5
    assert sequence_path("out.bmp", 0) == "out_0000.bmp" and sequence_path("d/x.y.bmp", 12) == "d/x.y_0012.bmp"
    # refused before the scene is read: the scene file need not exist
    r = subprocess.run([sys.executable, "-m", "fray_amd", "missing.fray", "--frames", "3"], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "--frames needs --denoise" in r.stderr, r.stderr


# ---- the projection against the oracle's camera rays ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell_box.fray", "forest.fray"])
def test_view_projects_the_oracle_rays_back(fray, abi, oracle, name):
    W, H = 96, 72
    s = open_scene(fray, name, W, H)
    s.camera.yaw += 13.0
    s.camera.pitch += -6.0
    s.camera.roll = 7.0
    s.camera.dof, s.camera.stereoSeparation = 0, 0.0
    view = fray.view_from_camera(s.camera, W, H)
    rng = np.random.default_rng(11)
    xy = rng.uniform((0, 0), (W, H), (300, 2))
    o, d = np.zeros(3), np.zeros(3)
    worst = 0.0
    for x, y in xy:
        oracle.lib.fray_oracle_camera_ray(C.byref(s.desc), float(x), float(y), o.ctypes.data, d.ctypes.data)
        for t in (1.0, 50.0, 1000.0):
            P = (o + t * d).astype(F)
            fx, fy, zc = temporal_ref.project(P, view)
            assert zc > 0
            worst = max(worst, abs(float(fx) - x), abs(float(fy) - y))
    print("%s: worst reprojection error %.3g pixel" % (name, worst))
    # the issue's bound; what is left is the FP32 rounding of the far points (about 3e-3 pixel at distance 1000)
    assert worst <= 1e-2, worst
    # a point behind the camera has no film position
    back = (o - 5.0 * d).astype(F)
    assert temporal_ref.project(back, view)[2] <= 0
    s.close()


# ---- the numpy restatement on synthetic inputs -------------------------------------------------------------------------------------------------

def _plane_frame(W, H, cam_x=0.0, depth=10.0, tan=0.5, normal=(0.0, 0.0, -1.0), albedo=(0.5, 0.5, 0.5), offset=0.5):
    """A fronto-parallel plane z = depth seen by a camera at (cam_x, 0, 0) looking along +z: (feat, view); pixel i sampled at film i + offset."""
    view = dict(pos=(cam_x, 0.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), front=(0.0, 0.0, 1.0), tan_x=tan, tan_y=tan * H / W, width=W, height=H)
    xs = (np.arange(W) + offset) / W * 2 - 1
    ys = 1 - (np.arange(H) + offset) / H * 2
    feat = np.zeros((H, W, 10), F)
    feat[..., 0] = cam_x + depth * tan * xs[None, :]
    feat[..., 1] = depth * (tan * H / W) * ys[:, None]
    feat[..., 2] = depth
    feat[..., 3:6] = normal
    feat[..., 6:9] = albedo
    feat[..., 9] = np.sqrt(((feat[..., 0:3] - np.array([cam_x, 0, 0], F)) ** 2).sum(-1))
    return feat, view


def test_restatement_constant_image_counts_up():
    W, H = 17, 11
    feat, view = _plane_frame(W, H)
    rgb = np.empty((H, W, 3), F)
    rgb[...] = (0.25, 0.5, 0.125)
    hist = None
    for k in range(7):
        hist, sig, var = temporal_ref.accumulate(rgb, feat, view if k else None, hist, max_history=5, demodulate=0)
        assert np.array_equal(sig, rgb) and np.array_equal(hist[..., 0:3], rgb), k
        # N is fetched like the colour, sum(b N_q) / sum(b): four FP32 roundings away from the integer until the clamp makes it exact
        want = min(k + 1, 5)
        assert np.abs(hist[..., 3] - want).max() <= 1e-6 * want, (k, np.unique(hist[..., 3]))
        assert k < 5 or np.all(hist[..., 3] == 5)
        assert var.max() <= 1e-6                      # zero but for the rounding of the window's 49-term sums (l * l is 0.085)
    assert sig.dtype == var.dtype == hist.dtype == F


def test_restatement_running_mean_and_population_variance():
    W, H, K = 12, 9, 10
    feat, view = _plane_frame(W, H)
    rng = np.random.default_rng(2)
    # m2 - m1 * m1 is a difference of two FP32 running means: its rounding error is about K / 2 ulps of m2 (1e-6 here), so a 1e-5 relative
    # bound on the variance needs a variance that is not small beside m2.  Each pixel's brightness runs through the same K levels 0 .. 2 in
    # an order of its own: noisy frames whose population variance is 0.41 beside m2 = 1.4 in every pixel.
    levels = np.linspace(0.0, 2.0, K)
    order = np.argsort(rng.uniform(size=(K, H, W)), axis=0)
    frames = (levels[order][..., None] * np.array([1.0, 0.8, 1.2])).astype(F)
    hist = None
    for k in range(K):
        hist, sig, var = temporal_ref.accumulate(frames[k], feat, view if k else None, hist, alpha_min=0.0, max_history=64, variance_history=1, demodulate=0)
    mean = frames.astype(np.float64).mean(0)
    lum = frames.astype(np.float64).mean(-1)
    assert np.abs(hist[..., 3] - K).max() <= 1e-6 * K
    assert np.abs(sig / mean - 1).max() <= 1e-5
    assert np.abs(var / lum.var(0) - 1).max() <= 1e-5
    # with demodulation the same in the signal's domain
    feat[..., 6:9] = (0.5, 0.25, 0.8)
    hist = None
    for k in range(K):
        hist, sig, var = temporal_ref.accumulate(frames[k], feat, view if k else None, hist, alpha_min=0.0, max_history=64, variance_history=1)
    assert np.abs(sig / (mean / np.array([0.5, 0.25, 0.8])) - 1).max() <= 1e-5


@pytest.mark.parametrize("k", [1, 3, -2])
def test_restatement_sideways_move_fetches_from_the_shifted_pixel(k):
    W, H, depth, tan = 32, 8, 10.0, 0.5
    pixel = 2 * depth * tan / W                       # the world width of one pixel on the plane
    f0, v0 = _plane_frame(W, H, 0.0, depth, tan)
    f1, _ = _plane_frame(W, H, k * pixel, depth, tan)          # the camera moved right by k pixels: the plane's points move left by k
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 1, (H, W, 3)).astype(F)
    h0, _, _ = temporal_ref.accumulate(a, f0, demodulate=0)
    zero = np.zeros((H, W, 3), F)
    h1, sig, _ = temporal_ref.accumulate(zero, f1, v0, h0, demodulate=0, alpha_min=0.0)
    xs = np.arange(W)
    src = xs + k                                      # pixel x of the new frame sees what pixel x + k of the old one saw
    ok = (src >= 1) & (src < W - 1)
    assert np.all(h1[:, ok, 3] == 2)
    # alpha = 1/2 of a zero frame: half the fetched history, which is the old pixel within the bilinear weights' rounding
    assert np.abs(sig[:, ok] * 2 - a[:, src[ok]]).max() <= 2e-4
    gone = (src < -1) | (src > W)
    assert np.all(h1[:, gone, 3] == 1)


def test_restatement_disocclusion_and_crease_restart():
    W, H = 24, 10
    back, view = _plane_frame(W, H, depth=20.0)
    near, _ = _plane_frame(W, H, depth=5.0)
    prev = back.copy()
    prev[:, 8:16] = near[:, 8:16]                     # an occluder in front of the middle columns ...
    rgb = np.full((H, W, 3), 0.5, F)
    h0, _, _ = temporal_ref.accumulate(rgb, prev)
    h1, _, _ = temporal_ref.accumulate(rgb, back, view, h0)  # ... gone in the next frame: the wall behind it was never seen
    N = h1[..., 3]
    assert np.all(N[:, 9:15] == 1) and np.all(N[:, :7] == 2) and np.all(N[:, 17:] == 2)
    # a 90 degree crease: the same positions with the normal turned take no history either
    turned = back.copy()
    turned[:, 12:, 3:6] = (1.0, 0.0, 0.0)
    h0, _, _ = temporal_ref.accumulate(rgb, back)
    h1, _, _ = temporal_ref.accumulate(rgb, turned, view, h0)
    assert np.all(h1[:, 12:, 3] == 1) and np.all(h1[:, :12, 3] == 2)
    # a miss (zero normal) neither takes nor gives history
    sky = back.copy()
    sky[:, :5, 0:6] = 0
    sky[:, :5, 9] = 0
    h0, _, _ = temporal_ref.accumulate(rgb, sky)
    h1, _, _ = temporal_ref.accumulate(rgb, sky, view, h0)
    assert np.all(h1[:, :5, 3] == 1) and np.all(h1[:, 6:, 3] == 2)
    h2, _, _ = temporal_ref.accumulate(rgb, back, view, h0)
    assert np.all(h2[:, :4, 3] == 1)


def test_restatement_spatial_variance_where_history_is_short():
    W, H = 20, 14
    feat, view = _plane_frame(W, H)
    rng = np.random.default_rng(8)
    hist = None
    for k in range(5):
        rgb = rng.uniform(0.1, 1.0, (H, W, 3)).astype(F)
        f = feat.copy()
        if k == 2:
            f[:, :6, 3:6] = (1.0, 0.0, 0.0)           # these columns lose their history in frame 2 (and again in 3, back on the old normal)
        hist, sig, var = temporal_ref.accumulate(rgb, f, view if k else None, hist, variance_history=3, demodulate=0)
        N, m1, m2 = hist[..., 3], hist[..., 7], hist[..., 11]
        temporal = np.maximum(F(0), m2 - m1 * m1)
        spatial = temporal_ref.spatial_variance(hist, f[..., 9], 0.02, 0.9) * (F(3) / N)
        old = N >= 3
        assert np.array_equal(var[old], temporal[old]) and np.array_equal(var[~old], spatial[~old]), k
        if k == 0:
            assert not old.any() and np.all(var > 0)
            # one frame: m2 - m1^2 is zero everywhere, the window's spread is what there is
            interior = spatial[3:-3, 3:-3]
            l = temporal_ref.lum(rgb).astype(np.float64)
            win = np.lib.stride_tricks.sliding_window_view(l, (7, 7))
            assert np.abs(interior / (win.var(axis=(2, 3)) * 3) - 1).max() <= 1e-4
        if k == 4:
            assert old[:, 8:].all() and not old[:, :5].any()
