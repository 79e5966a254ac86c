"""Progressive frames (include/frayhip.h): the entry points, struct mirrors and argument checks that need no GPU."""
import ctypes as C
import math
import os
import subprocess
import sys

from conftest import ROOT


def test_progressive_symbols_are_exported(fray, abi):
    for n in ("frayhip_render_progressive", "frayhip_render_device_progressive"):
        assert n in abi.SYMBOLS and hasattr(fray.lib, n), n


def test_progress_struct_mirrors(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_progress") == C.sizeof(abi.Progress)
    assert fray.lib.frayhip_sizeof(b"frayhip_progressive") == C.sizeof(abi.Progressive)
    assert abi.STRUCTS["frayhip_progress"] is abi.Progress and abi.STRUCTS["frayhip_progressive"] is abi.Progressive
    assert abi.E_CANCELLED == -7
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3         # nothing existing changed layout or meaning


def _never(_user, _p):
    raise AssertionError("the callback must not run on a rejected call")


def test_bad_arguments_are_rejected_without_a_gpu(fray, abi):
    fn = abi.PROGRESS_FN(_never)
    ok = abi.Progressive(fn=fn, user=None, preview_ms=0.0)
    nan = abi.Progressive(fn=fn, user=None, preview_ms=math.nan)
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
    rgb = (C.c_float * 3)()
    L = fray.lib
    # NULL scene, NULL frame
    assert L.frayhip_render_progressive(None, C.byref(fr), C.byref(ok), rgb, None, None, None) == abi.E_ARG
    assert L.frayhip_render_progressive(None, None, C.byref(ok), rgb, None, None, None) == abi.E_ARG
    assert L.frayhip_render_device_progressive(None, C.byref(fr), C.byref(ok), None, None, None, None, None) == abi.E_ARG
    assert L.frayhip_render_device_progressive(None, None, C.byref(ok), None, None, None, None, None) == abi.E_ARG
    # a NULL request and a NaN preview interval are refused before anything else is looked at
    assert L.frayhip_render_progressive(None, C.byref(fr), None, rgb, None, None, None) == abi.E_ARG
    assert b"progress request" in L.frayhip_last_error()
    for f in (lambda: L.frayhip_render_progressive(None, C.byref(fr), C.byref(nan), rgb, None, None, None),
              lambda: L.frayhip_render_device_progressive(None, C.byref(fr), C.byref(nan), None, None, None, None, None)):
        assert f() == abi.E_ARG
        assert b"preview_ms" in L.frayhip_last_error()


def test_cli_lists_the_progress_flags():
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, FRAYHIP_NO_TORCH="1"))
    assert out.returncode == 0, out.stderr
    assert "--progress" in out.stdout and "--time-limit" in out.stdout
