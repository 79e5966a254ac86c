"""Specular feature frames (include/frayhip.h "specular feature frames"), what can be checked without a GPU: the two entry points are exported,
declared and mirrored; every refusal that needs neither a scene nor the device, under the entry's own name; the Python side's own checks; the
CLI flag; and the kernel's source keeps to the state the header lists (no per-bounce array)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_abi import header_functions

F = np.float32
ENTRIES = ["frayhip_render_features_specular", "frayhip_render_features_specular_device"]


def test_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    src = open(os.path.join(ROOT, "include", "frayhip.h")).read()
    assert "#define FRAYHIP_SPECULAR_MAX_BOUNCES 8" in src and abi.SPECULAR_MAX_BOUNCES == 8
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additive: nothing existing changed layout or meaning
    # (scene, frame, n_samples, max_bounces, feat, bounces[, stream], stats)
    assert len(abi.SYMBOLS[ENTRIES[0]][1]) == 7 and len(abi.SYMBOLS[ENTRIES[1]][1]) == 8
    assert hasattr(fray.Scene, "render_features_specular")


@pytest.mark.parametrize("dev", [False, True])
def test_scene_free_refusals(fray, abi, dev):
    """frayhip_render_features' own first checks in its order, with max_bounces and the plane's alignment after n_samples and before the scene."""
    L = fray.lib
    feat = np.zeros((2, 2, 10), F)
    plane = np.zeros((2, 2), F)
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_stride=1)
    who = ENTRIES[1] if dev else ENTRIES[0]

    def call(f=fr, n=1, K=4, ft=feat.ctypes.data, bo=plane.ctypes.data):
        fp = C.byref(f) if f is not None else None
        if dev:
            return L.frayhip_render_features_specular_device(None, fp, n, K, ft, bo, None, None)
        return L.frayhip_render_features_specular(None, fp, n, K, ft, bo, None)

    cases = [(dict(f=None), "null frame"), (dict(ft=None), "null feat"), (dict(n=0), "n_samples"), (dict(), "null scene"),
             (dict(bo=None), "null scene"),                                                    # the plane may be NULL: the next check answers
             (dict(f=abi.Frame(mode=abi.MODE_PRIMARY_ID)), "mode must be")]
    cases += [(dict(K=k), "max_bounces must be 1 .. 8") for k in (0, -3, 9, 1 << 20)]
    cases += [(dict(K=k), "null scene") for k in (1, 8)]
    cases += [(dict(K=0, n=0), "n_samples")]                                                   # the order: n_samples first
    if dev:
        cases += [(dict(ft=feat.ctypes.data + 2), "aligned"), (dict(bo=plane.ctypes.data + 1), "aligned (bounces)"),
                  (dict(bo=plane.ctypes.data + 2, K=0), "max_bounces")]
    for kw, words in cases:
        assert call(**kw) == abi.E_ARG, kw
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, (kw, msg)


def test_python_side(fray, abi):
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))       # parsed, not uploaded
    with pytest.raises(fray.FrayError, match="beginRender"):
        s.render_features_specular(4)
    cams = [abi.Camera.from_buffer_copy(s.camera)]
    # what the arguments alone decide is refused before the device is asked for
    with pytest.raises(ValueError, match="first hits only"):
        next(s.render_sequence(cams, specular=4, edit=lambda k, scene: None))
    for k in (-1, 9):
        with pytest.raises(ValueError, match="specular must be 0 .. 8"):
            next(s.render_sequence(cams, specular=k))
    with pytest.raises(fray.FrayError, match="beginRender"):
        next(s.render_sequence(cams, specular=4))
    import inspect
    for m in (s.render_denoised, s.render_denoised_split, s.render_sequence):
        assert inspect.signature(m).parameters["specular"].default == 0
    sig = inspect.signature(s.render_features_specular).parameters
    assert [(k, sig[k].default) for k in sig] == [("max_bounces", 4), ("n_samples", 4), ("seed", 42), ("bucket_first", 0), ("bucket_stride", 1),
                                                  ("stats", False), ("out", None), ("bounces", False)]
    s.close()


def test_cli_lists_the_flag():
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, FRAYHIP_NO_TORCH="1"))
    assert out.returncode == 0 and "--specular-features" in out.stdout, out.stderr
    from fray_amd.__main__ import build_parser, check_args
    ap = build_parser()
    for argv in (["s.fray", "--denoise", "--specular-features", "4"], ["s.fray", "--features-out", "f.npy", "--specular-features", "1"],
                 ["s.fray", "--denoise", "--frames", "3", "--specular-features", "8"]):
        a = ap.parse_args(argv)
        check_args(ap, a)
        assert a.specular_features == int(argv[-1])
    assert ap.parse_args(["s.fray"]).specular_features == 0
    for argv in (["s.fray", "--specular-features", "4"], ["s.fray", "--denoise", "--specular-features", "9"],
                 ["s.fray", "--denoise", "--specular-features", "-1"],
                 ["s.fray", "--frames", "3", "--move", "5", "1", "0", "0", "--features-out", "f.npy", "--specular-features", "4"],
                 ["s.fray", "--denoise", "--frames", "3", "--move", "5", "1", "0", "0", "--motion-vectors", "--specular-features", "4"]):
        with pytest.raises(SystemExit):
            check_args(ap, ap.parse_args(argv))


def test_the_kernel_carries_no_per_bounce_array():
    """A tripwire only, not a proof: the kernel's source indexes nothing by the bounce count under the names it uses today (an array under another
    index name would pass; the scratch column of profiles/specular_features/README.md is the check), and the Makefile builds it per flag word."""
    src = open(os.path.join(ROOT, "fray_amd", "csrc", "features_specular_variant.hip")).read()
    body = src[src.index("void k_features_specular"):]
    assert not re.search(r"\[\s*b\s*\]", body) and "maxBounces]" not in body
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "specular:features_specular_variant" in mk
