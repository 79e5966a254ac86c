"""Motion frames (include/frayhip.h "motion frames"), what can be checked without a GPU: the four entry points are exported and mirrored, the
argument checks of frayhip_temporal_accumulate_motion (scene-free, refused before the device is touched), the scene-free refusals of
frayhip_render_features_motion, the Python side's own checks, the CLI flag, and the numpy restatement (tests/motion_ref.py) on synthetic
inputs: a motion frame that repeats the feature frame accumulates exactly as tests/temporal_ref.py does, and a plane that slid sideways finds
its history through the motion frame where the static rule finds another pixel's."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import motion_ref
import temporal_ref
from conftest import ROOT
from test_abi import header_functions
from test_temporal_abi import _plane_frame

F = np.float32
ENTRIES = ["frayhip_render_features_motion", "frayhip_render_features_motion_device", "frayhip_temporal_accumulate_motion",
           "frayhip_temporal_accumulate_motion_device"]


def test_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    assert abi.MOTION_CHANNELS == motion_ref.MOTION_CHANNELS == 8
    src = open(os.path.join(ROOT, "include", "frayhip.h")).read()
    assert "#define FRAYHIP_MOTION_CHANNELS 8" in src
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning


@pytest.mark.parametrize("dev", [False, True])
def test_accumulate_motion_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    rgb = np.zeros((H, W, 3), F)
    feat = np.zeros((H, W, 10), F)
    mot = np.zeros((H, W, 8), F)
    hin = np.zeros((H, W, 12), F)
    hout = np.zeros((H, W, 12), F)
    sig = np.zeros((H, W, 3), F)
    var = np.zeros((H, W), F)
    assert hin.ctypes.data % 16 == 0 and hout.ctypes.data % 16 == 0 and mot.ctypes.data % 16 == 0
    who = "frayhip_temporal_accumulate_motion_device" if dev else "frayhip_temporal_accumulate_motion"
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    view = fray.view_from_camera(s.camera, W, H)
    s.close()

    def call(w=W, h=H, r=rgb.ctypes.data, f=feat.ctypes.data, m=mot.ctypes.data, v="view", hi=hin.ctypes.data, p="default", ho=hout.ctypes.data,
             sg=sig.ctypes.data, va=var.ctypes.data, vw=None, **over):
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
            return L.frayhip_temporal_accumulate_motion_device(w, h, r, f, m, vp, hi, pp, ho, sg, va, None, None)
        return L.frayhip_temporal_accumulate_motion(w, h, r, f, m, vp, hi, pp, ho, sg, va, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, rc
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    # the list of frayhip_temporal_accumulate ...
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
    expect(call(vw=dict(pos0=math.nan)), "non-finite")
    expect(call(vw=dict(tan_y=0.0)), "tan_x and tan_y")
    expect(call(demodulate=2), "demodulate")
    for n in (0, 4097):
        expect(call(max_history=n), "max_history")
        expect(call(variance_history=n), "variance_history")
    for x in (-0.1, 1.5, math.nan):
        expect(call(alpha_min=x), "alpha_min")
    expect(call(film_offset=math.inf), "film_offset")
    for x in (-1.0, math.nan, math.inf):
        expect(call(plane_tolerance=x), "plane_tolerance")
    for x in (-1.5, 1.5, math.nan):
        expect(call(normal_min_dot=x), "normal_min_dot")
    expect(call(ho=hin.ctypes.data + 48), "overlap")
    expect(call(sg=rgb.ctypes.data), "overlap")
    # ... extended by the motion frame: NULL, aliased by an output wholly or in part, misaligned on the device
    expect(call(m=None), "null motion")
    expect(call(ho=mot.ctypes.data), "overlap")
    expect(call(sg=mot.ctypes.data + 32), "overlap")
    expect(call(va=mot.ctypes.data + 4 * 8 * W * H - 4), "overlap")
    expect(call(m=hout.ctypes.data), "overlap")
    if dev:
        expect(call(r=rgb.ctypes.data + 2), "aligned")
        expect(call(hi=hin.ctypes.data + 4), "16-byte")
        for off in (4, 8, 12):
            expect(call(m=mot.ctypes.data + off), "motion frame not 16-byte")


@pytest.mark.parametrize("dev", [False, True])
def test_features_motion_scene_free_refusals(fray, abi, dev):
    """What frayhip_render_features_motion refuses before it needs a scene: frayhip_render_features' own first checks, under its own name."""
    L = fray.lib
    feat = np.zeros((2, 2, 10), F)
    mot = np.zeros((2, 2, 8), F)
    T = (abi.Transform * 1)()
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_stride=1)
    who = "frayhip_render_features_motion_device" if dev else "frayhip_render_features_motion"

    def call(f=fr, n=1, ft=feat.ctypes.data):
        fp = C.byref(f) if f is not None else None
        if dev:
            return L.frayhip_render_features_motion_device(None, fp, n, T, 1, ft, mot.ctypes.data, None, None)
        return L.frayhip_render_features_motion(None, fp, n, T, 1, ft, mot.ctypes.data, None)

    for kw, words in ((dict(f=None), "null frame"), (dict(ft=None), "null feat"), (dict(n=0), "n_samples"), (dict(), "null scene"),
                      (dict(f=abi.Frame(mode=abi.MODE_PRIMARY_ID)), "mode must be")):
        assert call(**kw) == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg


def test_python_side(fray, abi):
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))       # parsed, not uploaded
    T = s.node_transforms()
    assert len(T) == s.desc.n_nodes and T._type_ is abi.Transform
    for i, n in enumerate(s.nodes):
        assert bytes(T[i]) == bytes(n.T)
    # a copy: editing a node afterwards leaves the snapshot alone, and the restatement sees exactly that node as moved
    before = bytes(T[5])
    fray.Transform(s.nodes[5]).translate(1.0, 2.0, 3.0).store(s.nodes[5])
    assert bytes(T[5]) == before and bytes(s.node_transforms()[5]) != before
    moved = motion_ref.moved_nodes(s.node_transforms(), T)
    assert moved.tolist() == [i == 5 for i in range(len(T))]
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_features_motion(T)
    s.close()
    rgb, feat = np.zeros((3, 4, 3), F), np.zeros((3, 4, 10), F)
    with pytest.raises(ValueError, match="motion"):
        fray.temporal_accumulate(rgb, feat, motion=np.zeros((3, 4, 7), F))
    with pytest.raises(TypeError, match="motion"):
        fray.temporal_accumulate(rgb, feat, motion=np.zeros((3, 4, 8), np.float64))


def test_cli_lists_the_motion_flag():
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, FRAYHIP_NO_TORCH="1"))
    assert out.returncode == 0 and "--motion-vectors" in out.stdout, out.stderr
    from fray_amd.__main__ import build_parser, check_args
    ap = build_parser()
    ok = ap.parse_args(["s.fray", "--denoise", "--frames", "3", "--move", "5", "1", "0", "0", "--motion-vectors"])
    check_args(ap, ok)
    assert ok.motion_vectors and not ap.parse_args(["s.fray"]).motion_vectors
    for argv in (["s.fray", "--motion-vectors"], ["s.fray", "--denoise", "--frames", "3", "--motion-vectors"],
                 ["s.fray", "--frames", "3", "--move", "5", "1", "0", "0", "--motion-vectors"]):
        with pytest.raises(SystemExit):
            check_args(ap, ap.parse_args(argv))


# ---- the numpy restatement on synthetic inputs -------------------------------------------------------------------------------------------------

def _identity(abi, fray, n):
    T = (abi.Transform * n)()
    for i in range(n):
        fray.lib.frayhip_transform_identity(C.byref(T[i]))
    return T


def test_motion_from_hits_order_and_rows(fray, abi):
    now, prev = _identity(abi, fray, 3), _identity(abi, fray, 3)
    fray.Transform().scale(2.0, 1.0, 0.5).rotate(30.0, 10.0, -5.0).translate(0.1, 0.2, 0.3).store(now[1])
    fray.Transform().rotate(7.0, 0.0, 0.0).translate(1.0 / 3.0, 0.0, -0.7).store(prev[1])
    ids = np.array([1, 0, -1, -2, 2], np.int32)
    rng = np.random.default_rng(1)
    rec = rng.uniform(-3, 3, (5, 9))
    m = motion_ref.motion_from_hits(ids, rec, now, prev)
    assert m.shape == (5, 8) and m.dtype == np.float64
    assert m[:, 3].tolist() == [1, 0, 0, 0, 0] and not m[:, 7].any()
    for k in (1, 3, 4):                                       # unmoved nodes and the light: the record's own point and normal
        assert np.array_equal(m[k, 0:3], rec[k, 1:4]) and np.array_equal(m[k, 4:7], rec[k, 4:7])
    assert not m[2].any()                                     # a miss
    # the moved row, scalar by scalar in the header's order
    o, inv, pm, po = list(now[1].offset), list(now[1].invM), list(prev[1].m), list(prev[1].offset)
    mul = lambda v, M: [(v[0] * M[j] + v[1] * M[3 + j]) + v[2] * M[6 + j] for j in range(3)]
    ip, nm = [float(x) for x in rec[0, 1:4]], [float(x) for x in rec[0, 4:7]]
    loc = mul([ip[k] - o[k] for k in range(3)], inv)
    want = [a + b for a, b in zip(mul(loc, pm), po)]
    assert m[0, 0:3].tolist() == want
    assert m[0, 4:7].tolist() == mul(mul(nm, inv), pm)
    # carried there and back, the point returns within rounding
    back = motion_ref.motion_from_hits(ids[:1], np.concatenate([[0.0], m[0, 0:3], m[0, 4:7], [0.0, 0.0]])[None], prev, now)
    assert np.abs(back[0, 0:3] - rec[0, 1:4]).max() <= 1e-12


@pytest.mark.parametrize("demodulate", [1, 0])
def test_restatement_with_nothing_moved_is_the_static_one(demodulate):
    W, H = 19, 13
    rng = np.random.default_rng(7)
    f0, v0 = _plane_frame(W, H, 0.0)
    f1, v1 = _plane_frame(W, H, 0.4)
    f1[2:5, 3:9, 3:6] = 0                                     # misses
    hist_s = hist_m = None
    view = None
    for k, feat in enumerate((f0, f1, f0)):
        rgb = rng.uniform(0, 1, (H, W, 3)).astype(F)
        mot = np.zeros((H, W, 8), F)
        mot[..., 0:3], mot[..., 4:7] = feat[..., 0:3], feat[..., 3:6]
        a = temporal_ref.accumulate(rgb, feat, view, hist_s, demodulate=demodulate)
        b = motion_ref.accumulate(rgb, feat, mot, view, hist_m, demodulate=demodulate)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), k
        hist_s, hist_m = a[0], b[0]
        view = (v0, v1, v0)[k]
    assert hist_m[..., 3].max() > 2 and (hist_m[..., 3] == 1).any()


def test_restatement_follows_a_plane_that_slid_sideways():
    """The camera stands still and the plane slides right by three pixels: P' = P - d fetches the pixel three to the left, where that surface
    point's history is; the static rule fetches the pixel's own (another point of the plane).  The CURRENT position goes to hist_out."""
    W, H, depth, tan, k = 32, 8, 10.0, 0.5, 3
    pixel = 2 * depth * tan / W
    feat, view = _plane_frame(W, H, 0.0, depth, tan)
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 1, (H, W, 3)).astype(F)
    h0, _, _ = temporal_ref.accumulate(a, feat, demodulate=0)
    mot = np.zeros((H, W, 8), F)
    mot[..., 0:3], mot[..., 4:7], mot[..., 3] = feat[..., 0:3], feat[..., 3:6], 1
    mot[..., 0] -= F(k * pixel)
    zero = np.zeros((H, W, 3), F)
    h1, sig, _ = motion_ref.accumulate(zero, feat, mot, view, h0, demodulate=0, alpha_min=0.0)
    xs = np.arange(W)
    src = xs - k
    ok = (src >= 1) & (src < W - 1)
    assert np.all(h1[:, ok, 3] == 2)
    assert np.abs(sig[:, ok] * 2 - a[:, src[ok]]).max() <= 2e-4
    assert np.all(h1[:, src < -1, 3] == 1)
    assert np.array_equal(h1[..., 4:7], feat[..., 0:3]) and np.array_equal(h1[..., 8:11], feat[..., 3:6])
    # a pixel whose n' is exactly zero takes no history, though its own normal is not zero
    mot[2, 10, 4:7] = 0
    h2, _, _ = motion_ref.accumulate(zero, feat, mot, view, h0, demodulate=0)
    assert h2[2, 10, 3] == 1 and h2[2, 11, 3] == 2
    # n' is scaled to unit length as the normal is: a mean of several samples' normals is shorter
    mot[..., 4:7] *= F(0.25)
    mot[2, 10, 4:7] = feat[2, 10, 3:6]
    h3, _, _ = motion_ref.accumulate(zero, feat, mot, view, h0, demodulate=0, alpha_min=0.0)
    assert np.array_equal(h3, h1)
