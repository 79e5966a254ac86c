"""The map from a state (include/frayhip.h "sample maps": frayhip_sample_map), what can be checked without a GPU: the entries are exported and
mirrored, the parameter struct's layout and defaults, every argument check answers FRAYHIP_E_ARG before the device is touched with the entry's name
in the message, the Python side refuses bad parameters, and the numpy restatement (tests/sample_map_ref.py) behaves as the header says on synthetic
states: the worked cases below are computed by hand from the formula, not taken from any implementation."""
import ctypes as C
import math

import numpy as np
import pytest

from sample_map_ref import sample_map_ref
from test_abi import header_functions

ENTRIES = ["frayhip_sample_map_defaults", "frayhip_sample_map", "frayhip_sample_map_device"]


def test_sample_map_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n


def test_sample_map_struct_layout_and_defaults(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_sample_map") == C.sizeof(abi.SampleMap) == 40
    assert abi.SampleMap.min_count.offset == 8 and abi.SampleMap.grow.offset == 20 and abi.SampleMap.pixels.offset == 24 and abi.SampleMap.samples.offset == 32
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3
    p = abi.SampleMap(pixels=9, samples=9)
    assert fray.lib.frayhip_sample_map_defaults(C.byref(p)) == 0
    assert (p.tolerance, p.lum_floor) == (np.float32(0.05), np.float32(0.01))
    assert (p.min_count, p.max_count, p.max_add, p.grow, p.pixels, p.samples) == (4, 0, 1 << 24, 2, 0, 0)      # max_count: the caller sets it
    assert fray.lib.frayhip_sample_map_defaults(None) == abi.E_ARG


def _params(abi, **kw):
    p = abi.SampleMap(tolerance=0.05, lum_floor=0.01, min_count=4, max_count=64, max_add=1 << 24, grow=2)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("dev", [False, True])
def test_sample_map_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 2
    buf = (C.c_float * (W * H * 6 + 8))()
    accum = (C.addressof(buf) + 15) & ~15
    count, add = accum + W * H * 16, accum + W * H * 20
    who = ENTRIES[2] if dev else ENTRIES[1]

    def call(p, W=W, H=H, accum=accum, count=count, add=add):
        pp = C.byref(p) if p is not None else None
        if dev:
            return L.frayhip_sample_map_device(W, H, accum, count, pp, add, None, None)
        return L.frayhip_sample_map(W, H, accum, count, pp, add, None)

    def expect(rc, words):
        assert rc == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and msg.startswith(who + ":"), msg

    ok = _params(abi)
    expect(call(ok, W=0), "width and height")
    expect(call(ok, H=-1), "width and height")
    expect(call(ok, W=1 << 16, H=(1 << 14) + 1), "2^30")
    expect(call(ok, accum=None), "null accum")
    expect(call(ok, count=None), "null count")
    expect(call(None), "null parameters")
    expect(call(ok, add=None), "null add")
    for t in (0.0, -0.05, math.inf, math.nan):
        expect(call(_params(abi, tolerance=t)), "tolerance must be")
        expect(call(_params(abi, lum_floor=t)), "lum_floor must be")
    for m in (0, -3):
        expect(call(_params(abi, min_count=m)), "min_count must be")
    expect(call(_params(abi, min_count=8, max_count=7)), "max_count must be >= min_count")
    expect(call(_params(abi, max_count=0)), "max_count must be >= min_count")          # the default: the caller has to set it
    expect(call(_params(abi, max_count=(1 << 24) + 1)), "2^24")
    for m in (0, -1):
        expect(call(_params(abi, max_add=m)), "max_add must be")
    for g in (1, 0, 17, -2):
        expect(call(_params(abi, grow=g)), "grow must be")
    expect(call(ok, add=accum), "add must not overlap")
    expect(call(ok, add=count + 4), "add must not overlap")
    expect(call(ok, count=accum + 16), "count must not overlap accum")
    if dev:
        expect(call(ok, accum=accum + 8, count=count + 8, add=add + 8), "16-byte aligned")
        expect(call(ok, count=count + 2, add=add + 8), "4-byte aligned")
        expect(call(ok, add=add + 2), "4-byte aligned")


def test_python_refuses_bad_parameters(fray):
    good = dict(tolerance=0.05, max_count=64)
    p = fray.sample_map_params(**good)
    assert (p.min_count, p.max_count, p.grow, p.max_add) == (4, 64, 2, 1 << 24)
    for bad in (dict(tolerance=0.0), dict(tolerance=math.nan), dict(tolerance=math.inf), dict(lum_floor=-1.0), dict(min_count=0), dict(max_count=3),
                dict(max_count=(1 << 24) + 1), dict(max_add=0), dict(grow=1), dict(grow=17)):
        with pytest.raises(ValueError):
            fray.sample_map_params(**dict(good, **bad))
    with pytest.raises(ValueError, match="max_count"):
        fray.sample_map_params(tolerance=0.05)
    with pytest.raises(TypeError):
        fray.sample_map_params(max_count=8, sigma=1.0)
    with pytest.raises(TypeError):
        fray.sample_map(np.zeros((2, 2, 4), np.float32), max_count=8)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------------------

def row(lum, N, var):
    """The state row of N samples of grey `lum` whose luminances have biased variance `var`: sum = N * lum per channel, m2 = N * (var + lum^2)."""
    return [N * lum, N * lum, N * lum, N * (var + lum * lum)]


def one(r, N, **kw):
    add, pixels, samples = sample_map_ref(np.array([[r]], np.float32), np.array([[N]], np.int32), **kw)
    assert pixels == int(add[0, 0] > 0) and samples == int(add[0, 0])
    return int(add[0, 0])


def test_ref_counts_below_min_and_at_max():
    kw = dict(tolerance=0.5, lum_floor=0.01, min_count=4, max_count=64)
    assert one([math.nan] * 4, 0, **kw) == 4                  # N = 0: the row is not looked at
    assert one(row(1.0, 1, 0.0), 1, **kw) == 3
    assert one(row(1.0, 3, 0.0), 3, **kw) == 1
    assert one(row(1.0, 64, 100.0), 64, **kw) == 0            # N = max_count
    assert one(row(1.0, 70, 100.0), 70, **kw) == 0            # and past it
    assert one([math.nan] * 4, 2, max_add=1, **kw) == 1       # max_add binds below min_count too


def test_ref_quiet_pixel_stops_at_min_count():
    # v = 0: need = 0, target = N, add = 0
    assert one(row(0.5, 4, 0.0), 4, tolerance=0.05, min_count=4, max_count=64) == 0


def test_ref_need_from_the_variance():
    # N = 8, lbar = 1, v = 0.5: noise = 0.5 / 7; t = 0.25 -> need = ceil(8 * (0.5 / 7) / 0.0625) = ceil(9.142..) = 10 -> add 2
    assert one(row(1.0, 8, 0.5), 8, tolerance=0.25, min_count=4, max_count=64) == 2
    # the same with grow binding: tolerance 0.125 -> need = ceil(36.57) = 37 > 2 * 8 -> target 16 -> add 8; grow 4 -> 32 -> 24; grow 8 -> 37 -> 29
    assert one(row(1.0, 8, 0.5), 8, tolerance=0.125, min_count=4, max_count=64) == 8
    assert one(row(1.0, 8, 0.5), 8, tolerance=0.125, min_count=4, max_count=64, grow=4) == 24
    assert one(row(1.0, 8, 0.5), 8, tolerance=0.125, min_count=4, max_count=64, grow=8) == 29
    # max_count binding before grow: grow 8 with max_count 20 -> 12; and max_add binding: 5
    assert one(row(1.0, 8, 0.5), 8, tolerance=0.125, min_count=4, max_count=20, grow=8) == 12
    assert one(row(1.0, 8, 0.5), 8, tolerance=0.125, min_count=4, max_count=64, grow=8, max_add=5) == 5


def test_ref_dark_pixel_is_measured_against_the_floor():
    # lbar = 0.001 < lum_floor = 0.5: t = 0.5 * 0.5; N = 4, v = 0.25: noise = 0.25 / 3, need = ceil(4 * (0.25 / 3) / 0.0625) = ceil(5.33) = 6 -> add 2
    assert one(row(0.001, 4, 0.25), 4, tolerance=0.5, lum_floor=0.5, min_count=4, max_count=64) == 2
    # without the floor the same pixel asks for everything grow allows
    assert one(row(0.001, 4, 0.25), 4, tolerance=0.5, lum_floor=1e-6, min_count=4, max_count=64) == 4


def test_ref_single_sample_is_as_uncertain_as_its_value():
    # N = 1 (min_count 1): noise = lbar^2 = 1, t = 0.5: need = ceil(1 / 0.25) = 4, grow 2 -> target 2 -> add 1
    assert one(row(1.0, 1, 0.0), 1, tolerance=0.5, min_count=1, max_count=64) == 1
    assert one(row(1.0, 1, 0.0), 1, tolerance=0.5, min_count=1, max_count=64, grow=16) == 3


def test_ref_nan_and_huge_needs_ask_for_max_count():
    kw = dict(tolerance=0.05, min_count=4, max_count=1000, grow=16)
    # a NaN row at N = 1 (min_count 1): noise = NaN, need = NaN -> max_count, then grow
    assert one([math.nan] * 4, 1, tolerance=0.05, min_count=1, max_count=1000, grow=16) == 15
    # an infinite second moment: need = inf -> max_count (grow 16 * 100 > 1000)
    assert one([100.0, 100.0, 100.0, math.inf], 100, **kw) == 900
    # a need far above max_count (and above what an int holds): v = 1e30
    assert one(row(1.0, 100, 1e30), 100, **kw) == 900
    # a NaN row at N >= 2: fmaxf(0, NaN) = 0, so the variance reads 0 and the pixel asks for nothing (the formula as written)
    assert one([math.nan] * 4, 8, **kw) == 0


def test_ref_totals_over_a_plane():
    state = np.array([[row(1.0, 8, 0.5), row(1.0, 8, 0.0)], [row(1.0, 2, 0.0), row(1.0, 64, 9.0)]], np.float32)
    count = np.array([[8, 8], [2, 64]], np.int32)
    add, pixels, samples = sample_map_ref(state, count, tolerance=0.25, min_count=4, max_count=64)
    assert add.tolist() == [[2, 0], [2, 0]] and pixels == 2 and samples == 4 and add.dtype == np.int32
