"""Feature frames and the denoiser (include/frayhip.h "feature frames", "denoising"), what can be checked without a GPU: the four entry points
and the defaults entry are exported and mirrored, struct frayhip_denoise's layout and defaults match, every argument check that needs no
uploaded scene answers FRAYHIP_E_ARG with the entry's name before the device is touched, the CLI lists its flags and refuses --denoise with
--adaptive, and the numpy restatement of the filter (tests/denoise_ref.py) behaves as the header says on synthetic inputs."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref
from conftest import ROOT
from test_abi import header_functions

ENTRIES = ["frayhip_render_features", "frayhip_render_features_device", "frayhip_denoise", "frayhip_denoise_device", "frayhip_denoise_defaults"]


def test_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n


def test_denoise_struct_and_defaults(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_denoise") == C.sizeof(abi.Denoise) == 24
    assert abi.Denoise.sigma_luminance.offset == 8 and abi.Denoise.sigma_albedo.offset == 20
    p = abi.Denoise()
    assert fray.lib.frayhip_denoise_defaults(C.byref(p)) == abi.OK
    assert (p.levels, p.demodulate) == (5, 1)
    assert (p.sigma_luminance, p.sigma_normal, p.sigma_depth) == (4.0, 128.0, 1.0)
    assert p.sigma_albedo == np.float32(0.1)
    assert fray.lib.frayhip_denoise_defaults(None) == abi.E_ARG
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning
    # the Python side starts from the same defaults
    q = fray.denoise_params(levels=3)
    assert (q.levels, q.demodulate, q.sigma_normal) == (3, 1, 128.0)
    with pytest.raises(TypeError):
        fray.denoise_params(sigma=1.0)


@pytest.mark.parametrize("dev", [False, True])
def test_denoise_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    rgb = np.zeros((H, W, 3), np.float32)
    half = np.zeros((H, W, 3), np.float32)
    feat = np.zeros((H, W, 10), np.float32)
    out = np.zeros((H, W, 3), np.float32)
    who = "frayhip_denoise_device" if dev else "frayhip_denoise"

    def call(w=W, h=H, r=rgb.ctypes.data, hf=half.ctypes.data, f=feat.ctypes.data, p="default", o=out.ctypes.data, **over):
        prm = abi.Denoise()
        L.frayhip_denoise_defaults(C.byref(prm))
        for k, v in over.items():
            setattr(prm, k, v)
        pp = C.byref(prm) if p == "default" else None
        if dev:
            return L.frayhip_denoise_device(w, h, r, hf, f, pp, o, None, None)
        return L.frayhip_denoise(w, h, r, hf, f, pp, o, None)

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
    expect(call(o=None), "null out")
    expect(call(levels=0), "levels")
    expect(call(levels=11), "levels")
    expect(call(demodulate=2), "demodulate")
    for name in ("sigma_luminance", "sigma_normal", "sigma_depth", "sigma_albedo"):
        expect(call(**{name: math.nan}), name)
        expect(call(**{name: -1.0}), name)
        expect(call(**{name: math.inf}), name)
    for name in ("sigma_luminance", "sigma_depth", "sigma_albedo"):
        expect(call(**{name: 0.0}), name)
    # out aliasing an input, wholly or in part
    expect(call(o=rgb.ctypes.data), "overlap")
    expect(call(o=half.ctypes.data + 4), "overlap")
    expect(call(o=feat.ctypes.data + 40), "overlap")
    if dev:
        expect(call(r=rgb.ctypes.data + 2), "aligned")


@pytest.mark.parametrize("dev", [False, True])
def test_features_argument_checks(fray, abi, dev):
    L = fray.lib
    feat = np.zeros(10, np.float32)
    who = "frayhip_render_features_device" if dev else "frayhip_render_features"

    def call(f="render", n=1, out=feat.ctypes.data):
        fr = None if f is None else abi.Frame(mode=abi.MODE_RENDER if f == "render" else abi.MODE_PRIMARY_ID, seed=42)
        fp = C.byref(fr) if fr is not None else None
        if dev:
            return L.frayhip_render_features_device(None, fp, n, out, None, None)
        return L.frayhip_render_features(None, fp, n, out, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, rc
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    expect(call(f=None), "null frame")
    expect(call(out=None), "null feat")
    expect(call(f="primary"), "MODE_RENDER")
    expect(call(n=0), "n_samples")
    expect(call(n=-3), "n_samples")
    expect(call(), "null scene")
    if dev:
        expect(call(out=feat.ctypes.data + 1), "aligned")


def test_python_side_refuses_bad_inputs(fray):
    rgb = np.zeros((4, 5, 3), np.float32)
    feat = np.zeros((4, 5, 10), np.float32)
    with pytest.raises(TypeError):
        fray.denoise(rgb.astype(np.float64), feat)
    with pytest.raises(ValueError):
        fray.denoise(rgb, feat[:, :4])
    with pytest.raises(ValueError):
        fray.denoise(rgb, feat[..., :9])
    with pytest.raises(fray.FrayError, match="levels"):
        fray.denoise(rgb, feat, levels=11)
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_features(1)
    s.close()


def test_cli_lists_the_denoise_flags():
    env = dict(os.environ, FRAYHIP_NO_TORCH="1")
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr
    for flag in ("--denoise", "--features-out", "--feature-samples"):
        assert flag in out.stdout, flag
    from fray_amd.__main__ import build_parser
    a = build_parser().parse_args(["scene.fray", "--denoise", "--features-out", "f.npy"])
    assert a.denoise and a.features_out == "f.npy" and a.feature_samples == 4
    # refused before the scene is read: the scene file need not exist
    r = subprocess.run([sys.executable, "-m", "fray_amd", "missing.fray", "--denoise", "--adaptive", "0.1"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 2 and "--denoise cannot be combined with --adaptive" in r.stderr, r.stderr


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------

def _features(H, W, normal=(0, 1, 0), depth=2.0, albedo=(0.5, 0.5, 0.5)):
    f = np.zeros((H, W, 10), np.float32)
    f[..., 3:6] = normal
    f[..., 6:9] = albedo
    f[..., 9] = depth
    return f


def _ulps(a, b):
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64)).max()


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("with_half", [False, True])
def test_restatement_constant_image_stays_constant(demodulate, with_half):
    H, W = 23, 31
    rgb = np.empty((H, W, 3), np.float32)
    rgb[...] = (0.3, 0.7, 0.11)
    half = rgb.copy() if with_half else None
    feat = _features(H, W, albedo=(0.4, 0.9, 0.25))
    for levels in (1, 3, 5):
        out = denoise_ref.denoise(rgb, feat, half, levels=levels, demodulate=demodulate)
        assert _ulps(out, rgb) <= 1, levels


def test_restatement_orthogonal_half_planes_do_not_leak():
    H, W = 20, 40
    feat = _features(H, W)
    feat[:, W // 2:, 3:6] = (1, 0, 0)                   # the right half faces +x, the left half +y
    rgb = np.zeros((H, W, 3), np.float32)
    rgb[:, :W // 2] = 0.2
    rng = np.random.default_rng(3)
    rgb[:, W // 2:] = rng.uniform(0.5, 1.5, (H, W - W // 2, 3))
    half = rgb * np.float32(0.9)
    for h in (None, half):
        out = denoise_ref.denoise(rgb, feat, h, levels=5)
        assert np.array_equal(out[:, :W // 2], rgb[:, :W // 2] / np.maximum(feat[:, :W // 2, 6:9], np.float32(1e-3))
                              * np.maximum(feat[:, :W // 2, 6:9], np.float32(1e-3)))
        assert np.all(out[:, W // 2:] > 0.45) and np.all(out[:, W // 2:] < 1.55)


def test_restatement_one_tap_gives_the_input_back():
    rng = np.random.default_rng(5)
    rgb = rng.uniform(0, 2, (1, 1, 3)).astype(np.float32)
    feat = _features(1, 1, albedo=(0.3, 0.6, 0.9))
    for levels in (1, 5, 10):
        assert np.array_equal(denoise_ref.denoise(rgb, feat, None, levels=levels, demodulate=0), rgb)
        assert _ulps(denoise_ref.denoise(rgb, feat, rgb, levels=levels, demodulate=1), rgb) <= 1
    # every tap but the centre weighted 0 (each pixel's albedo far from all others' at a small sigma_albedo): each pixel is its own only tap
    H, W = 7, 9
    feat = _features(H, W)
    feat[..., 6] = np.arange(H * W, dtype=np.float32).reshape(H, W)
    img = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    for levels in (1, 4):
        assert np.array_equal(denoise_ref.denoise(img, feat, None, levels=levels, demodulate=0, sigma_albedo=1e-3), img)
        assert np.array_equal(denoise_ref.denoise(img, feat, img * np.float32(0.5), levels=levels, demodulate=0, sigma_albedo=1e-3), img)


def test_restatement_weights_follow_the_header():
    # two pixels, one tap apart: out = c_p + w (c_q - c_p) / (h_p + w) with w = h * w_n * w_z * w_a * w_l (no rgb_half: sigma_l * 2^-k)
    f = np.float32
    rgb = np.array([[[0.2, 0.2, 0.2], [0.8, 0.8, 0.8]]], np.float32)
    feat = _features(1, 2, albedo=(1, 1, 1))
    feat[0, 1, 6:9] = (0.9, 1.0, 1.0)
    feat[0, 1, 9] = 2.5
    out = denoise_ref.denoise(rgb, feat, None, levels=1, demodulate=0)
    hc, hn = f(0.375) * f(0.375), f(0.25) * f(0.375)
    gx = f(2.5) - f(2.0)
    wz = np.exp(-f(0.5) / (f(1.0) * abs(gx * f(1)) + f(1e-4)))
    wa = np.exp(-f(0.1) / f(0.1))
    wl = np.exp(-f(0.6) / f(4.0))
    w = (((hn * f(1)) * wz) * wa) * wl
    expect = f(0.2) + (w * (f(0.8) - f(0.2))) / (hc + w)
    assert abs(out[0, 0, 0] - expect) <= 2e-7
