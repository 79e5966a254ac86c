"""Ray queries (include/frayhip.h "ray queries"), what can be checked without a GPU: the six entry points are exported and mirrored, every
argument check answers FRAYHIP_E_ARG before the device is touched (each named in frayhip_last_error), and the CLI's --probe is parsed."""
import ctypes as C

import pytest

from test_abi import header_functions

ENTRIES = ["frayhip_camera_rays", "frayhip_camera_rays_device", "frayhip_trace_rays", "frayhip_trace_rays_device",
           "frayhip_visible", "frayhip_visible_device"]
# addresses that are never dereferenced: every call below fails its checks first
D8, D4, D1 = 0x10000, 0x10004, 0x10001


def test_query_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n


def _expect_arg(fray, abi, rc, words):
    assert rc == abi.E_ARG
    msg = fray.lib.frayhip_last_error().decode()
    assert words in msg, msg


def test_trace_rays_argument_checks(fray, abi):
    L = fray.lib
    st = abi.Stats()
    buf = (C.c_double * 64)()
    ids = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    for dev in (False, True):
        def call(s, n, o, d, i, dist, rec):
            if dev:
                return L.frayhip_trace_rays_device(s, n, o, d, 0, i, dist, rec, None, C.byref(st))
            return L.frayhip_trace_rays(s, n, o, d, 0, i, dist, rec, C.byref(st))
        o = D8 if dev else p
        _expect_arg(fray, abi, call(None, -1, o, o, o, o, o), "n must be")
        _expect_arg(fray, abi, call(None, 2 ** 31, o, o, o, o, o), "n must be")
        _expect_arg(fray, abi, call(None, 1, None, o, o, o, o), "null input")
        _expect_arg(fray, abi, call(None, 1, o, None, o, o, o), "null input")
        _expect_arg(fray, abi, call(None, 1, o, o, None, None, None), "no output")
        _expect_arg(fray, abi, call(None, 1, o, o, o, o, o), "null scene")
        _expect_arg(fray, abi, call(None, 0, None, None, o, None, None), "null scene")           # n == 0 still needs a scene
    _expect_arg(fray, abi, L.frayhip_trace_rays(None, 1, p, p, 0, C.cast(ids, C.c_void_p), None, None, None), "null scene")
    for bad in ((D1, D8, D8, D8, D8), (D8, D4, D8, D8, D8), (D8, D8, D8, D4, D8), (D8, D8, D8, D8, D4)):
        _expect_arg(fray, abi, L.frayhip_trace_rays_device(None, 1, bad[0], bad[1], 0, bad[2], bad[3], bad[4], None, None), "8-byte aligned")
    _expect_arg(fray, abi, L.frayhip_trace_rays_device(None, 1, D8, D8, 0, D1, None, None, None, None), "4-byte aligned")
    _expect_arg(fray, abi, L.frayhip_trace_rays_device(None, 1, D8, D8, 0, D4, None, None, None, None), "null scene")


def test_visible_argument_checks(fray, abi):
    L = fray.lib
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    _expect_arg(fray, abi, L.frayhip_visible(None, -5, p, p, 0, p, None), "n must be")
    _expect_arg(fray, abi, L.frayhip_visible(None, 1, None, p, 0, p, None), "null input")
    _expect_arg(fray, abi, L.frayhip_visible(None, 1, p, None, 0, p, None), "null input")
    _expect_arg(fray, abi, L.frayhip_visible(None, 1, p, p, 0, None, None), "no output")
    _expect_arg(fray, abi, L.frayhip_visible(None, 1, p, p, 0, p, None), "null scene")
    _expect_arg(fray, abi, L.frayhip_visible_device(None, 2 ** 40, D8, D8, 0, D1, None, None), "n must be")
    _expect_arg(fray, abi, L.frayhip_visible_device(None, 1, D4, D8, 0, D1, None, None), "8-byte aligned")
    _expect_arg(fray, abi, L.frayhip_visible_device(None, 1, D8, D1, 0, D1, None, None), "8-byte aligned")
    _expect_arg(fray, abi, L.frayhip_visible_device(None, 1, D8, D8, 0, D1, None, None), "null scene")     # a byte output has no alignment


def test_camera_rays_argument_checks(fray, abi):
    L = fray.lib
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    _expect_arg(fray, abi, L.frayhip_camera_rays(None, -1, p, 0, p, p), "n must be")
    for eye in (-1, 3):
        _expect_arg(fray, abi, L.frayhip_camera_rays(None, 1, p, eye, p, p), "eye must be")
        _expect_arg(fray, abi, L.frayhip_camera_rays_device(None, 1, D8, eye, D8, D8, None), "eye must be")
    _expect_arg(fray, abi, L.frayhip_camera_rays(None, 1, p, 0, None, None), "no output")
    _expect_arg(fray, abi, L.frayhip_camera_rays(None, 1, p, 2, p, None), "null scene")
    _expect_arg(fray, abi, L.frayhip_camera_rays(None, 4, None, 1, None, p), "null scene")        # xy NULL: every pixel
    _expect_arg(fray, abi, L.frayhip_camera_rays_device(None, 1, D4, 0, D8, D8, None), "8-byte aligned")
    _expect_arg(fray, abi, L.frayhip_camera_rays_device(None, 1, D8, 0, D8, D1, None), "8-byte aligned")
    _expect_arg(fray, abi, L.frayhip_camera_rays_device(None, 1, D8, 0, None, D8, None), "null scene")


def test_probe_is_a_cli_option():
    from fray_amd.__main__ import build_parser
    ap = build_parser()
    assert "--probe" in ap.format_help()
    a = ap.parse_args(["scene.fray", "--probe", "3", "4.5", "--width", "64", "--height", "48"])
    assert a.probe == [3.0, 4.5] and (a.width, a.height) == (64, 48)
    assert build_parser().parse_args(["scene.fray"]).probe is None
    with pytest.raises(SystemExit):
        ap.parse_args(["scene.fray", "--probe", "3"])
