"""Adaptive frames (include/frayhip.h "adaptive frames"), what can be checked without a GPU: both entry points are exported and mirrored, the request
struct's layout matches the library's, every argument check that needs no uploaded scene answers FRAYHIP_E_ARG before the device is touched, the
Python side refuses bad values, the CLI lists its flags, and the numpy restatement of the ladder and stop rule (tests/adaptive_ladder.py) behaves as
the header says on synthetic frames."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from adaptive_ladder import expected, ladder, rung_error, rung1_threshold
from conftest import ROOT, SCENES
from test_abi import header_functions

ENTRIES = ["frayhip_render_adaptive", "frayhip_render_device_adaptive"]


def test_adaptive_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n


def test_adaptive_struct_layout(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_adaptive") == C.sizeof(abi.Adaptive) == 40
    assert abi.STRUCTS["frayhip_adaptive"] is abi.Adaptive
    assert abi.Adaptive.threshold.offset == 8 and abi.Adaptive.rungs.offset == 24 and abi.Adaptive.samples.offset == 32
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning


def _req(abi, **kw):
    a = abi.Adaptive(min_spp=4, threshold=0.05, err_floor=0.01)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("dev", [False, True])
def test_adaptive_argument_checks(fray, abi, dev):
    L = fray.lib
    rgb = (C.c_float * 3)()
    spp = (C.c_int32 * 1)()
    err = (C.c_float * 1)()
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)

    def call(f, a, out=rgb):
        fp = C.byref(f) if f is not None else None
        ap = C.byref(a) if a is not None else None
        if dev:
            return L.frayhip_render_device_adaptive(None, fp, ap, out, spp, err, None, None)
        return L.frayhip_render_adaptive(None, fp, ap, out, spp, err, None)

    def expect(rc, words):
        assert rc == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and "adaptive" in msg, msg

    ok = _req(abi)
    expect(call(None, ok), "null frame")
    expect(call(fr, None), "null request")
    expect(call(fr, ok, None), "null rgb")
    expect(call(abi.Frame(mode=abi.MODE_PRIMARY_ID, seed=42), ok), "mode must be")
    for m in (1, 0, -5):
        expect(call(fr, _req(abi, min_spp=m)), "min_spp must be >= 2")
    for t in (math.nan, -1e-9, -math.inf):
        expect(call(fr, _req(abi, threshold=t)), "threshold must be")
    for e in (0.0, -0.01, math.inf, math.nan):
        expect(call(fr, _req(abi, err_floor=e)), "err_floor must be")
    # the extreme legal values pass every check that needs no scene
    expect(call(fr, _req(abi, min_spp=2, threshold=math.inf, err_floor=1e-300)), "null scene")
    expect(call(fr, _req(abi, threshold=0.0)), "null scene")


def test_python_validation_needs_no_gpu(fray):
    s = fray.Scene.parseScene(os.path.join(SCENES, "cornell_box.fray"))       # parsed, not uploaded
    for kw in (dict(min_spp=1), dict(min_spp=-2), dict(threshold=math.nan), dict(threshold=-0.5), dict(err_floor=0.0), dict(err_floor=-1.0),
               dict(err_floor=math.inf), dict(err_floor=math.nan)):
        args = dict(threshold=0.05)
        args.update(kw)
        with pytest.raises(ValueError):
            s.render_adaptive(**args)
        with pytest.raises(ValueError):
            s.render_adaptive_device(0, **args)
    # good values get as far as the missing upload
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_adaptive(math.inf, min_spp=2)
    s.close()


def test_cli_lists_the_adaptive_flags():
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, FRAYHIP_NO_TORCH="1"))
    assert out.returncode == 0, out.stderr
    for flag in ("--adaptive", "--min-spp", "--adaptive-floor"):
        assert flag in out.stdout, flag
    from fray_amd.__main__ import build_parser
    a = build_parser().parse_args(["scene.fray", "--adaptive", "0.05", "--min-spp", "8", "--adaptive-floor", "0.02"])
    assert (a.adaptive, a.min_spp, a.adaptive_floor) == (0.05, 8, 0.02)
    assert build_parser().parse_args(["scene.fray"]).adaptive is None


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------

def test_ladder():
    assert ladder(16, 64) == [8, 16, 32, 64]
    assert ladder(4, 64) == [2, 4, 8, 16, 32, 64]
    assert ladder(4, 40) == [2, 4, 8, 16, 32, 40]           # the capped last rung
    assert ladder(3, 10) == [1, 3, 6, 10]
    assert ladder(2, 2) == [1, 2]
    assert ladder(64, 64) == [32, 64]                        # min_spp == spp: two rungs
    for bad in ((1, 8), (9, 8)):
        with pytest.raises(AssertionError):
            ladder(*bad)


def test_rung_error_order_and_widening():
    m = np.array([[0.5, 0.25, 0.125]], np.float32)
    h = np.array([[0.25, 0.5, 0.0]], np.float32)
    num = (0.25 + 0.25) + 0.125
    assert rung_error(m, h, 0.01)[0] == num / (0.01 + ((0.5 + 0.25) + 0.125))
    # widened before subtracting: float32 values whose difference float32 would round
    a = np.array([[1.0000001, 0, 0]], np.float32)
    b = np.array([[1.0, 0, 0]], np.float32)
    assert rung_error(a, b, 1.0)[0] == (np.float64(a[0, 0]) - 1.0) / (1.0 + np.float64(a[0, 0]))
    assert rung_error(m, m, 0.01)[0] == 0.0


def _synthetic(H=6, W=5, spp=40, min_spp=4, seed=3, nan=True):
    """Frames F_r of the ladder: a pixel's noise shrinks with r at its own rate; with `nan`, pixel (0, 0) is NaN from rung 1 on."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.1, 1.0, (H, W, 3)).astype(np.float32)
    noise = rng.uniform(0.0, 0.5, (H, W, 1)).astype(np.float32)
    frames = {}
    rs = ladder(min_spp, spp)
    for j, r in enumerate(rs):
        f = base + noise * rng.standard_normal((H, W, 3)).astype(np.float32) / np.float32(np.sqrt(r))
        if nan and j >= 1:
            f[0, 0] = np.nan
        frames[r] = f.astype(np.float32)
    return frames


def test_expected_stop_rule_on_synthetic_frames():
    spp, mn, fl = 40, 4, 0.01
    frames = _synthetic(spp=spp, min_spp=mn)
    rs = ladder(mn, spp)
    thr = rung1_threshold(frames, mn, spp, fl, 0.5)
    rgb, sm, em = expected(frames, mn, spp, thr, fl)
    assert set(np.unique(sm)) <= set(rs[1:]) and len(np.unique(sm)) >= 2
    for (y, x), r in np.ndenumerate(sm):
        j = rs.index(r)
        assert np.array_equal(rgb[y, x], frames[r][y, x], equal_nan=True)
        e = [rung_error(frames[rs[k]][y, x], frames[rs[k - 1]][y, x], fl) for k in range(1, len(rs))]
        assert em[y, x] == np.float32(e[j - 1]) or (np.isnan(em[y, x]) and np.isnan(e[j - 1]))
        # no earlier rung satisfied the rule; this one did, or it is the capped last rung
        assert not any(ek <= thr for ek in e[:j - 1])
        assert e[j - 1] <= thr or r == spp
    # the NaN pixel never stops early: it runs to the capped last rung with a NaN error
    assert sm[0, 0] == spp == 40 and np.isnan(em[0, 0]) and np.isnan(rgb[0, 0]).all()


def test_expected_infinite_threshold_and_min_equals_spp():
    frames = _synthetic(spp=32, min_spp=4, nan=False)
    rgb, sm, em = expected(frames, 4, 32, math.inf, 0.01)
    assert (sm == 4).all() and np.array_equal(rgb, frames[4]) and np.isfinite(em).all()
    # even an infinite threshold does not stop a NaN error
    rgb, sm, em = expected(_synthetic(spp=32, min_spp=4), 4, 32, math.inf, 0.01)
    assert sm[0, 0] == 32 and (sm.ravel()[1:] == 4).all()
    frames = _synthetic(spp=16, min_spp=16, nan=False)
    assert sorted(frames) == [8, 16]
    rgb, sm, em = expected(frames, 16, 16, 0.0, 0.01)
    assert (sm == 16).all() and np.array_equal(rgb, frames[16])
    # threshold 0: only pixels whose two means agree exactly stop early
    frames = _synthetic(spp=16, min_spp=4)
    frames[4][2, 3] = frames[2][2, 3]
    rgb, sm, em = expected(frames, 4, 16, 0.0, 0.01)
    assert sm[2, 3] == 4 and em[2, 3] == 0 and (np.delete(sm.ravel(), 2 * sm.shape[1] + 3) == 16).all()
