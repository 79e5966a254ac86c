"""Radiance queries (include/frayhip.h "radiance queries"), what can be checked without a GPU: both entry points are exported and mirrored, the
request struct's layout matches the library's, every argument check answers FRAYHIP_E_ARG before the device is touched (each named in
frayhip_last_error), and the CLI's --shade is parsed."""
import ctypes as C

import pytest

from test_abi import header_functions

ENTRIES = ["frayhip_shade_rays", "frayhip_shade_rays_device"]
# addresses that are never dereferenced: every call below fails its checks first
D8, D4, D1 = 0x10000, 0x10004, 0x10001


def test_shade_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n


def test_shade_request_layout(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_shade_request") == C.sizeof(abi.ShadeRequest) == 32
    assert abi.STRUCTS["frayhip_shade_request"] is abi.ShadeRequest
    assert abi.ShadeRequest.keys.offset == 24


def _expect_arg(fray, abi, rc, words):
    assert rc == abi.E_ARG
    msg = fray.lib.frayhip_last_error().decode()
    assert words in msg and "frayhip_shade_rays" in msg, msg


def _req(abi, **kw):
    r = abi.ShadeRequest(seed=42, spp=1, sample_first=0, rng_skip=0, flags=0, keys=None)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


@pytest.mark.parametrize("dev", [False, True])
def test_shade_rays_argument_checks(fray, abi, dev):
    L = fray.lib
    st = abi.Stats()
    buf = (C.c_double * 64)()
    p = D8 if dev else C.cast(buf, C.c_void_p).value

    def call(n, o, d, req, rgb):
        r = C.byref(req) if req is not None else None
        if dev:
            return L.frayhip_shade_rays_device(None, n, o, d, r, rgb, None, C.byref(st))
        return L.frayhip_shade_rays(None, n, o, d, r, rgb, C.byref(st))

    ok = _req(abi)
    _expect_arg(fray, abi, call(1, p, p, None, p), "null request")
    _expect_arg(fray, abi, call(1, p, p, ok, None), "null rgb")
    _expect_arg(fray, abi, call(-1, p, p, ok, p), "n must be")
    _expect_arg(fray, abi, call(2 ** 31, p, p, ok, p), "n must be")
    _expect_arg(fray, abi, call(1, None, p, ok, p), "null input")
    _expect_arg(fray, abi, call(1, p, None, ok, p), "null input")
    for spp in (0, -3):
        _expect_arg(fray, abi, call(1, p, p, _req(abi, spp=spp), p), "spp must be")
    _expect_arg(fray, abi, call(1, p, p, _req(abi, sample_first=-1), p), "sample_first must be")
    _expect_arg(fray, abi, call(1, p, p, _req(abi, sample_first=2 ** 31 - 4, spp=4), p), "overflows")
    for skip in (-1, 9):
        _expect_arg(fray, abi, call(1, p, p, _req(abi, rng_skip=skip), p), "rng_skip must be")
    # the largest legal values pass every check but the scene's
    _expect_arg(fray, abi, call(1, p, p, _req(abi, sample_first=2 ** 31 - 5, spp=4, rng_skip=8), p), "null scene")
    _expect_arg(fray, abi, call(0, None, None, ok, p), "null scene")            # n == 0 still needs a scene
    _expect_arg(fray, abi, call(1, p, p, ok, p), "null scene")


def test_shade_rays_device_alignment(fray, abi):
    L = fray.lib
    ok = abi.ShadeRequest(seed=42, spp=1, sample_first=0, rng_skip=0, flags=0, keys=None)
    for o, d in ((D4, D8), (D8, D1)):
        _expect_arg(fray, abi, L.frayhip_shade_rays_device(None, 1, o, d, C.byref(ok), D4, None, None), "8-byte aligned")
    _expect_arg(fray, abi, L.frayhip_shade_rays_device(None, 1, D8, D8, C.byref(ok), D1, None, None), "4-byte aligned")
    keyed = abi.ShadeRequest(seed=42, spp=1, sample_first=0, rng_skip=0, flags=0, keys=D1)
    _expect_arg(fray, abi, L.frayhip_shade_rays_device(None, 1, D8, D8, C.byref(keyed), D4, None, None), "4-byte aligned")
    keyed.keys = D4
    _expect_arg(fray, abi, L.frayhip_shade_rays_device(None, 1, D8, D8, C.byref(keyed), D4, None, None), "null scene")


def test_shade_is_a_cli_option():
    from fray_amd.__main__ import build_parser
    ap = build_parser()
    assert "--shade" in ap.format_help()
    a = ap.parse_args(["scene.fray", "--probe", "3", "4", "--shade"])
    assert a.probe == [3.0, 4.0] and a.shade
    assert not ap.parse_args(["scene.fray", "--probe", "3", "4"]).shade
