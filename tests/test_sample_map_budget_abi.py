"""The budgeted sample map (include/frayhip.h "sample maps": frayhip_sample_map_budget), what can be checked without a GPU: the entries are
exported and mirrored, the budget struct's layout, every argument check answers FRAYHIP_E_ARG before the device is touched with the entry's name
in the message, the Python side refuses bad budgets, and the restatement (tests/sample_map_budget_ref.py) does what the header says: worked cases
computed by hand on one- and two-pixel planes, and the definition's properties on the synthetic plane of tests/test_gpu_samples_map.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import SCENES
from sample_map_budget_ref import TOL_MAX, bits_of, float_of, sample_map_budget_ref
from sample_map_ref import sample_map_ref
from test_abi import header_functions
from test_sample_map_abi import _params, row

ENTRIES = ["frayhip_sample_map_budget", "frayhip_sample_map_budget_device"]
PARAMS = [dict(tolerance=0.05, max_count=64), dict(tolerance=0.2, max_count=64, grow=16, max_add=5),
          dict(tolerance=0.5, lum_floor=0.5, min_count=1, max_count=48, grow=3)]           # test_sample_map_equals_its_restatement's three
IDS = ["defaults", "caps", "floor"]


def budgets_of(D, F):
    """The budgets of the issue for a plane whose map sums to D at the caller's tolerance and to F at FLT_MAX."""
    return [D, D - 1, D // 2, (D + F) // 2, F + 1, F, F - 1, F // 2, 1, 0]


def test_budget_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n


def test_budget_struct_layout(fray, abi):
    B = abi.SampleBudget
    assert fray.lib.frayhip_sizeof(b"frayhip_sample_budget") == C.sizeof(B) == 32
    assert [getattr(B, f).offset for f in ("budget", "demand", "tolerance_used", "cap_used", "stage", "reserved")] == [0, 8, 16, 20, 24, 28]
    assert fray.lib.frayhip_sizeof(b"frayhip_sample_map") == C.sizeof(abi.SampleMap) == 40          # unchanged
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3


@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_budget_argument_checks(fray, abi, dev, pair):
    L = fray.lib
    W, H = 4, 2
    n = W * H
    buf = (C.c_float * (n * 10 + 8))()
    accum = (C.addressof(buf) + 15) & ~15
    accum2 = accum + n * 16
    count, add = accum + n * 32, accum + n * 36
    who = ENTRIES[1] if dev else ENTRIES[0]
    second = accum2 if pair else None

    def call(p, W=W, H=H, accum=accum, accum2=second, count=count, add=add, b=abi.SampleBudget(budget=5)):
        pp = C.byref(p) if p is not None else None
        bb = C.byref(b) if b is not None else None
        if dev:
            return L.frayhip_sample_map_budget_device(W, H, accum, accum2, count, pp, bb, add, None, None)
        return L.frayhip_sample_map_budget(W, H, accum, accum2, count, pp, bb, add, None)

    def expect(rc, words):
        assert rc == abi.E_ARG
        msg = L.frayhip_last_error().decode()
        assert words in msg and msg.startswith(who + ":"), msg

    ok = _params(abi)
    expect(call(ok, W=0), "width and height")
    expect(call(ok, H=-1), "width and height")
    expect(call(ok, W=1 << 16, H=(1 << 14) + 1), "2^30")
    expect(call(ok, accum=None), "null accum_direct" if pair else "null accum")
    expect(call(ok, count=None), "null count")
    expect(call(None), "null parameters")
    expect(call(ok, add=None), "null add")
    for t in (0.0, -0.05, math.inf, math.nan):
        expect(call(_params(abi, tolerance=t)), "tolerance must be")
        expect(call(_params(abi, lum_floor=t)), "lum_floor must be")
    for m in (0, -3):
        expect(call(_params(abi, min_count=m)), "min_count must be")
    expect(call(_params(abi, min_count=8, max_count=7)), "max_count must be >= min_count")
    expect(call(_params(abi, max_count=0)), "max_count must be >= min_count")
    expect(call(_params(abi, max_count=(1 << 24) + 1)), "2^24")
    for m in (0, -1):
        expect(call(_params(abi, max_add=m)), "max_add must be")
    for g in (1, 0, 17, -2):
        expect(call(_params(abi, grow=g)), "grow must be")
    expect(call(ok, add=accum), "add must not overlap")
    expect(call(ok, add=count + 4), "add must not overlap")
    expect(call(ok, count=accum + 16), "count must not overlap accum")
    if pair:
        expect(call(ok, add=accum2 + 16), "add must not overlap")
        expect(call(ok, accum2=accum + 16), "accum_indirect must not overlap accum_direct")
        expect(call(ok, count=accum2 + 16), "count must not overlap accum_indirect")
    if dev:
        expect(call(ok, accum=accum + 8, count=count + 8, add=add + 8), "16-byte aligned")
        expect(call(ok, count=count + 2, add=add + 8), "4-byte aligned")
        expect(call(ok, add=add + 2), "4-byte aligned")
        if pair:
            expect(call(ok, accum2=accum2 + 8), "16-byte aligned")
    # the two checks of the budget itself, after the map's
    expect(call(ok, b=None), "null budget")
    expect(call(ok, b=abi.SampleBudget(budget=5, reserved=1)), "reserved must be 0")
    expect(call(_params(abi, grow=1), b=None), "grow must be")


def test_python_refuses_bad_budgets(fray):
    W, H = 4, 2
    st = fray.Accumulation(np.zeros((H, W, 4), np.float32), 4, 42, (W, H))
    for bad in (-1, -(1 << 70), 1 << 64):
        with pytest.raises(ValueError, match="budget"):
            fray.sample_map(st, budget=bad, max_count=8)
    for bad in (2.5, 3.0, "3", True, [3]):
        with pytest.raises(TypeError, match="budget"):
            fray.sample_map(st, budget=bad, max_count=8)
    share = fray.Accumulation.empty((96, 96), 42, 1, 2)
    with pytest.raises(ValueError, match="bucket share"):
        fray.sample_map(share, budget=10, max_count=8)
    with pytest.raises(ValueError, match="bucket share"):
        fray.sample_map((share, fray.Accumulation.empty((96, 96), 42, 1, 2)), budget=10, max_count=8)
    s = fray.Scene.parseScene(os.path.join(SCENES, "cornell_box.fray"))
    with pytest.raises(ValueError, match="bucket share"):
        s.refine(None, 0.1, 8, budget=10, bucket_first=1, bucket_stride=2)
    with pytest.raises(ValueError, match="budget"):
        s.refine(None, 0.1, 8, budget=-1)
    with pytest.raises(TypeError, match="budget"):
        s.refine(None, 0.1, 8, budget=1.5)
    with pytest.raises(ValueError, match="budget needs refine"):
        s.render_denoised_split(budget=10)


# ---- the restatement: worked cases -----------------------------------------------------------------------------------------------------------

# Two pixels of N = 8 and lbar = 1 at tolerance 0.25 (t * t = 0.0625), grow 8, max_count 64:
#   A: v = 0.5,  noise = 0.5 / 7:   need = ceil(8 * (0.5 / 7) / 0.0625)  = ceil(9.142..)  = 10 -> add 2   (test_ref_need_from_the_variance's pixel)
#   B: v = 0.75, noise = 0.75 / 7:  need = ceil(8 * (0.75 / 7) / 0.0625) = ceil(13.714..) = 14 -> add 6
# A's need drops to 9 where 8 * (0.5 / 7) / tau^2 <= 9, tau >= sqrt(4 / 63) = 0.2519763..; B's drops to 13 at sqrt(6 / 91) = 0.2567763..
TWO = np.array([[row(1.0, 8, 0.5), row(1.0, 8, 0.75)]], np.float32)
TWO_N = np.array([[8, 8]], np.int32)
TWO_KW = dict(tolerance=0.25, min_count=4, max_count=64, grow=8)


def test_ref_two_pixels_at_and_one_under_their_demand():
    add, info = sample_map_budget_ref(TWO, TWO_N, 8, **TWO_KW)
    assert add.tolist() == [[2, 6]] and (info["stage"], info["demand"], info["samples"], info["cap_used"]) == (0, 8, 8, -1)
    assert info["tolerance_used"] == np.float32(0.25) and info["pixels"] == 2
    add, info = sample_map_budget_ref(TWO, TWO_N, 7, **TWO_KW)
    assert add.tolist() == [[1, 6]] and (info["stage"], info["demand"], info["samples"], info["cap_used"]) == (1, 8, 7, -1)


def test_ref_the_tolerance_at_which_the_first_ceil_drops():
    _, info = sample_map_budget_ref(TWO, TWO_N, 7, **TWO_KW)
    tau = info["tolerance_used"]
    assert abs(float(tau) - math.sqrt(4.0 / 63.0)) < 2e-7                      # float32 steps here are 3e-8; the roundings of t * t, the quotient and the product move it by a few
    below = float_of(bits_of(tau) - 1)
    assert sample_map_ref(TWO, TWO_N, **dict(TWO_KW, tolerance=tau))[0].tolist() == [[1, 6]]
    assert sample_map_ref(TWO, TWO_N, **dict(TWO_KW, tolerance=below))[0].tolist() == [[2, 6]]
    # and the second pixel's: a budget of 6 needs B at 13 (add 5) with A at 9
    _, info = sample_map_budget_ref(TWO, TWO_N, 6, **TWO_KW)
    assert info["stage"] == 1 and info["samples"] == 6 and abs(float(info["tolerance_used"]) - math.sqrt(6.0 / 91.0)) < 2e-7


def test_ref_empty_plane_under_two_and_a_half_samples_a_pixel():
    W, H = 7, 5
    rows = np.full((H, W, 4), np.nan, np.float32)
    count = np.zeros((H, W), np.int32)
    add, info = sample_map_budget_ref(rows, count, (5 * W * H) // 2, tolerance=0.05, min_count=4, max_count=32)
    assert (add == 2).all() and (info["stage"], info["cap_used"], info["samples"], info["demand"]) == (2, 2, 2 * W * H, 4 * W * H)
    assert info["tolerance_used"] == TOL_MAX and info["pixels"] == W * H
    add, info = sample_map_budget_ref(rows, count, W * H - 1, tolerance=0.05, min_count=4, max_count=32)
    assert (add == 0).all() and (info["stage"], info["cap_used"], info["samples"], info["pixels"]) == (2, 0, 0, 0)


# ---- the restatement: the definition's properties on the synthetic plane ---------------------------------------------------------------------

@pytest.mark.parametrize("params", PARAMS, ids=IDS)
def test_ref_properties_on_the_synthetic_plane(params):
    from test_gpu_samples_map import synthetic_state
    state, count = synthetic_state()
    total = lambda **kw: sample_map_ref(state, count, **dict(params, **kw))[2]
    D, F = total(), total(tolerance=TOL_MAX)
    assert D > F > 3
    stages, caps, last = [], [], None
    for budget in sorted(set(budgets_of(D, F))):
        add, info = sample_map_budget_ref(state, count, budget, **params)
        assert info["samples"] <= budget and info["demand"] == D and info["samples"] == int(add.sum()) and (add >= 0).all()
        if info["stage"] == 0:
            assert budget >= D and add.tobytes() == sample_map_ref(state, count, **params)[0].tobytes()
        elif info["stage"] == 1:
            tau = info["tolerance_used"]
            assert F <= budget < D and np.float32(params["tolerance"]) < tau <= TOL_MAX and info["cap_used"] == -1
            assert add.tobytes() == sample_map_ref(state, count, **dict(params, tolerance=tau))[0].tobytes()
            assert total(tolerance=float_of(bits_of(tau) - 1)) > budget                     # no smaller tolerance fits
        else:
            cap = info["cap_used"]
            at_max = sample_map_ref(state, count, **dict(params, tolerance=TOL_MAX))[0]
            assert budget < F and 0 <= cap < params.get("max_add", 1 << 24) and info["tolerance_used"] == TOL_MAX
            assert add.tobytes() == np.minimum(at_max, cap).astype(np.int32).tobytes()
            assert int(np.minimum(at_max, cap + 1).sum()) > budget                          # no larger cap fits
            caps.append(cap)
        assert last is None or info["samples"] >= last or info["stage"] != stages[-1]       # within a stage a larger budget buys no less
        last = info["samples"]
        stages.append(info["stage"])
    assert stages.count(1) >= 3 and stages.count(2) >= 3 and len(set(caps)) >= 3 and stages.count(0) == 1, (stages, caps)
