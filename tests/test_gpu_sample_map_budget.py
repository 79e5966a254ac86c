"""Budgeted sample maps on a real MI355X (include/frayhip.h "sample maps": frayhip_sample_map_budget).  The kernels' 16-way search and the two-way
bisection of tests/sample_map_budget_ref.py must give the same plane, the same bits of tolerance_used, the same cap, stage and totals, through the
host entry and the device entry, for one state and for a pair; and Scene.refine under a budget must hold exactly the counts a simulation from the
uniform snapshots predicts, each pixel the frame of its count bit for bit.  All comparisons are of bits."""
import json
import os
import re
import sys

import numpy as np
import pytest

import test_gpu_components_map as pairs
from conftest import ROOT, run_in_clean_child
from sample_map_budget_ref import TOL_MAX, bits_of, float_of, sample_map_budget_ref
from sample_map_pair_ref import sample_map_pair_ref
from sample_map_ref import sample_map_ref
from samples_ref import mean_and_noise
from test_gpu_samples_map import cornell, expectation, same, synthetic_state
from test_sample_map_budget_abi import IDS, PARAMS, budgets_of

pytestmark = pytest.mark.gpu

KEYS = ("pixels", "samples", "budget", "demand", "cap_used", "stage")


def states_of(fray, rows, count, device):
    """The Accumulation (a pair: the tuple of two) of rows and per-pixel counts, numpy or on the GPU."""
    import torch
    H, W = count.shape
    uniform = count.min() == count.max()
    put = (lambda a: torch.from_numpy(a.copy()).cuda()) if device else (lambda a: a.copy())
    make = lambda r: fray.Accumulation(put(r), int(count.min()), 42, (W, H), counts=None if uniform else put(count))
    return tuple(make(r) for r in rows) if isinstance(rows, tuple) else make(rows)


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def check_against(fray, rows, count, budget, params, device, want=None, **kw):
    """One budgeted map through the host or the device entry against the restatement; returns (add, info, the restatement's pair)."""
    want = want or sample_map_budget_ref(rows, count, budget, **params)
    add, info = fray.sample_map(states_of(fray, rows, count, device), budget=budget, **dict(params, **kw))
    print("budget %d: stage %d tolerance %r cap %d samples %d of demand %d" % (budget, info["stage"], info["tolerance_used"], info["cap_used"], info["samples"],
                                                                               info["demand"]))
    w_add, w = want
    assert {k: info[k] for k in KEYS} == {k: w[k] for k in KEYS}, (info, w)
    assert bits_of(info["tolerance_used"]) == bits_of(w["tolerance_used"]), (info["tolerance_used"], w["tolerance_used"])
    got = host(add)
    assert same(got, w_add), (np.argwhere(got != w_add)[:5], got[got != w_add][:5], w_add[got != w_add][:5])
    assert info["samples"] <= budget
    return got, info, want


def pair_rows(state):
    return (state * np.float32(0.75), state[::-1].copy() * np.float32(0.3125))           # test_pair_sample_map_equals_its_restatement's planes


# ---- 1: the restatement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("params", PARAMS, ids=IDS)
def test_budgeted_map_equals_its_restatement(fray, gpu, params, pair):
    state, count = synthetic_state()
    rows = pair_rows(state) if pair else state
    plain = (lambda **kw: sample_map_pair_ref(rows[0], rows[1], count, **dict(params, **kw))) if pair else (
        lambda **kw: sample_map_ref(rows, count, **dict(params, **kw)))
    D, F = plain()[2], plain(tolerance=TOL_MAX)[2]
    print("D %d, F %d" % (D, F))
    stages, caps = [], []
    for budget in budgets_of(D, F):
        add, info, want = check_against(fray, rows, count, budget, params, False)
        dadd, dinfo, _ = check_against(fray, rows, count, budget, params, True, want=want)
        assert same(add, dadd) and info == dinfo
        stages.append(info["stage"])
        st = states_of(fray, rows, count, False)
        if info["stage"] == 0:
            assert same(add, fray.sample_map(st, **params)[0]) and info["cap_used"] == -1
            assert bits_of(info["tolerance_used"]) == bits_of(params["tolerance"])
        elif info["stage"] == 1:
            at, at_info = fray.sample_map(st, **dict(params, tolerance=info["tolerance_used"]))
            assert same(add, at) and at_info["samples"] == info["samples"]
            below = float_of(bits_of(info["tolerance_used"]) - 1)
            assert fray.sample_map(st, **dict(params, tolerance=below))[1]["samples"] > budget
        else:
            caps.append(info["cap_used"])
    assert stages.count(1) >= 3 and stages.count(2) >= 3 and len(set(caps)) >= 3, (stages, caps)


# ---- 2: shapes where the kernels can go wrong -----------------------------------------------------------------------------------------------------
def tiled(W, H):
    state, count = synthetic_state()
    ry, rx = -(-H // count.shape[0]), -(-W // count.shape[1])
    return np.ascontiguousarray(np.tile(state, (ry, rx, 1))[:H, :W]), np.ascontiguousarray(np.tile(count, (ry, rx))[:H, :W])


def test_a_single_pixel(fray, gpu):
    nan = np.full((1, 1, 4), np.nan, np.float32)
    zero = np.zeros((1, 1), np.int32)
    kw = dict(tolerance=0.05, min_count=4, max_count=64)
    for device in (False, True):
        for budget, stage, cap, samples in ((4, 0, -1, 4), (5, 0, -1, 4), (3, 2, 3, 3), (1, 2, 1, 1), (0, 2, 0, 0)):
            add, info, _ = check_against(fray, nan, zero, budget, kw, device)
            assert (info["stage"], info["cap_used"], info["samples"]) == (stage, cap, samples)
        # N = 8, lbar = 1, v = 0.5 at tolerance 0.25, grow 8: add 2; one sample fewer needs the tolerance of tests/test_sample_map_budget_abi.py
        rows = np.array([[[8, 8, 8, 12]]], np.float32)
        eight = np.full((1, 1), 8, np.int32)
        add, info, _ = check_against(fray, rows, eight, 1, dict(tolerance=0.25, min_count=4, max_count=64, grow=8), device)
        assert info["stage"] == 1 and add[0, 0] == 1 and abs(float(info["tolerance_used"]) - (4.0 / 63.0) ** 0.5) < 2e-7
        add, info, _ = check_against(fray, rows, eight, 0, dict(tolerance=0.25, min_count=4, max_count=64, grow=8), device)
        assert info["stage"] == 1 and add[0, 0] == 0             # need <= 8: tolerance sqrt(4 / 56)
        assert abs(float(info["tolerance_used"]) - (4.0 / 56.0) ** 0.5) < 2e-7


@pytest.mark.parametrize("shape", [(257, 3), (1024, 513)], ids=["block-edge", "second-trip"])
def test_block_edge_and_the_grid_strides_second_trip(fray, gpu, shape):
    """257 x 3: one thread past a block's edge, three blocks and a ragged fourth.  1024 x 513: 525312 pixels, the smallest plane of this width past
    the 2048 blocks x 256 threads of the launch, so that some threads take a second trip through the grid-stride loop."""
    W, H = shape
    rows, count = tiled(W, H)
    params = PARAMS[0]
    D, F = sample_map_ref(rows, count, **params)[2], sample_map_ref(rows, count, **dict(params, tolerance=TOL_MAX))[2]
    assert (W * H > 2048 * 256) == (shape == (1024, 513))
    seen = []
    for budget, device in ((D // 2, True), (F // 2, True), (D // 2, False), (D, True)):
        _, info, _ = check_against(fray, rows, count, budget, params, device)
        seen.append(info["stage"])
    assert seen == [1, 2, 1, 0]


# ---- 3: sums past 2^32 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64), (1024, 513)], ids=["64x64", "second-trip"])
def test_sums_past_two_to_the_32(fray, gpu, shape):
    """Every pixel asks for 2^24 - 2^20 samples.  64 x 64: the frame's total is fifteen times 2^32, and a block's 256 pixels come to
    0.94 * 2^32: just under it, a block never holds more than 256 pixels of a plane this small.  1024 x 513: the four blocks whose threads take
    a second trip hold 512 pixels, 1.9 * 2^32 a block."""
    W, H = shape
    N = 1 << 20
    count = np.full((H, W), N, np.int32)
    rows = np.empty((H, W, 4), np.float32)
    rows[..., :3] = np.float32(N) * np.float32(0.5)
    rows[..., 3] = np.inf
    params = dict(tolerance=0.05, max_count=1 << 24, grow=16)
    D, F = sample_map_ref(rows, count, **params)[2], sample_map_ref(rows, count, **dict(params, tolerance=TOL_MAX))[2]
    each = (1 << 24) - N
    assert D == F == W * H * each and D >= 15 << 32 and (shape == (64, 64) or 512 * each > 1 << 32)
    for budget in (D // 2, F // 3):
        for device in (False, True) if shape == (64, 64) else (True,):
            add, info, _ = check_against(fray, rows, count, budget, params, device)
            assert info["stage"] == 2 and info["cap_used"] == budget // (W * H) and info["samples"] == W * H * info["cap_used"] > 1 << 32


# ---- 4: the control block is the call's own -------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_on_a_stream(fray, gpu):
    import torch
    state, count = synthetic_state()
    params = PARAMS[0]
    D, F = sample_map_ref(state, count, **params)[2], sample_map_ref(state, count, **dict(params, tolerance=TOL_MAX))[2]
    stream = torch.cuda.Stream()
    dev = states_of(fray, state, count, True)
    torch.cuda.synchronize()
    results = []
    for budget in (D // 2, F // 2, D // 2, D, D // 2):
        add, info = fray.sample_map(dev, budget=budget, stream=stream, **params)
        results.append((budget, add.cpu().numpy(), info))
    first = results[0]
    for budget, add, info in results:
        w_add, w = sample_map_budget_ref(state, count, budget, **params)
        assert same(add, w_add) and {k: info[k] for k in KEYS} == {k: w[k] for k in KEYS}
        if budget == first[0]:
            assert same(add, first[1]) and info == first[2]
    assert [r[2]["stage"] for r in results] == [1, 2, 1, 0, 1]


# ---- 5: refine under a budget ---------------------------------------------------------------------------------------------------------------------
def simulate(rows_at, shape, passes, budget, **params):
    """Scene.refine(budget=) from the snapshots alone: the counts after each pass of the budget restatement, the passes and the last map's info."""
    counts = np.zeros(shape, np.int32)
    left, done, info = budget, 0, None
    for _ in range(passes):
        if left == 0:
            break
        add, info = sample_map_budget_ref(rows_at(counts), counts, left, **params)
        if info["pixels"] == 0:
            break
        counts = counts + add
        left -= info["samples"]
        done += 1
    return counts, done, info


def rows_from(S):
    def at(counts):
        rows = np.zeros(counts.shape + (4,), np.float32)
        for n in np.unique(counts):
            if n > 0:
                rows[counts == n] = S[n][counts == n]
        return rows
    return at


def refine_params(S4_noise_over_ref):
    tau = S4_noise_over_ref[np.isfinite(S4_noise_over_ref) & (S4_noise_over_ref > 0)]
    return dict(tolerance=float(np.quantile(tau, 0.5)), min_count=4, max_count=32)


def lum(rgb):
    return ((rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]) / np.float32(3)


def test_refine_under_a_budget_reaches_the_simulated_counts(fray, gpu):
    s, S = cornell(fray, 64, 48, top=32)
    H, W = 48, 64
    rgb4, noise4 = mean_and_noise(S[4], 4)
    params = refine_params(np.sqrt(noise4) / np.maximum(lum(rgb4), np.float32(0.01)))
    _, _, _, free = s.refine(None, passes=8, **params)
    budget = free["samples"] // 2
    want, passes, last = simulate(rows_from(S), (H, W), 8, budget, **params)
    rgb, st, noise, info = s.refine(None, passes=8, budget=budget, **params)
    print("unbudgeted %d samples; budget %d: %d spent in %d passes, tolerance reached %r, stage %d" % (free["samples"], budget, info["samples"], info["passes"],
                                                                                                      info["tolerance_reached"], info["stage"]))
    assert same(st.count_plane(), want), (np.unique(st.count_plane(), return_counts=True), np.unique(want, return_counts=True))
    assert int(st.count_plane().sum()) == info["samples"] <= budget
    rows, want_rgb, want_noise = expectation(S, want, np.zeros((H, W, 4), np.float32))
    assert same(st.state, rows) and same(rgb, want_rgb) and same(noise, want_noise)
    assert info["passes"] == passes and info["budget"] == budget and info["stage"] == last["stage"]
    assert bits_of(info["tolerance_reached"]) == bits_of(last["tolerance_used"])
    assert info["stage"] >= 1 and info["tolerance_reached"] > np.float32(params["tolerance"])            # the budget did bind
    assert len(np.unique(want)) >= 3


def test_refine_on_a_pair_under_a_budget(fray, gpu):
    s, DI = pairs.cornell(fray, 64, 48, top=32)
    H, W = 48, 64
    (rd, nd), (ri, ni) = mean_and_noise(DI[0][4], 4), mean_and_noise(DI[1][4], 4)
    params = refine_params(np.sqrt(nd + ni) / np.maximum(lum(rd) + lum(ri), np.float32(0.01)))
    free = s.refine(None, passes=8, split=True, **params)[-1]
    budget = free["samples"] // 2
    at_d, at_i = rows_from(DI[0]), rows_from(DI[1])
    want, passes, last = simulate(lambda c: (at_d(c), at_i(c)), (H, W), 8, budget, **params)
    d_rgb, i_rgb, st, d_noise, i_noise, info = s.refine(None, passes=8, split=True, budget=budget, **params)
    assert same(st[0].count_plane(), want) and same(st[1].count_plane(), want)
    assert int(want.sum()) == info["samples"] <= budget
    for a, S, rgb, noise in zip(st, DI, (d_rgb, i_rgb), (d_noise, i_noise)):
        rows, want_rgb, want_noise = expectation(S, want, np.zeros((H, W, 4), np.float32))
        assert same(a.state, rows) and same(rgb, want_rgb) and same(noise, want_noise)
    assert info["passes"] == passes and info["budget"] == budget and info["stage"] == last["stage"] >= 1
    assert bits_of(info["tolerance_reached"]) == bits_of(last["tolerance_used"])
    # the same keyword through the split filter
    out, raw, dinfo = s.render_denoised_split(refine=params["tolerance"], max_count=32, budget=budget)
    assert same(dinfo["refine"]["counts"], want) and dinfo["refine"]["budget"] == budget and np.isfinite(out).all()


def test_two_and_a_half_samples_a_pixel_from_an_empty_state(fray, gpu):
    s, S = cornell(fray, 64, 48, top=32)
    H, W = 48, 64
    rgb, st, noise, info = s.refine(None, 0.05, 32, budget=(5 * W * H) // 2)
    assert st.counts is None and st.samples_done == 2 and same(st.state, S[2])
    want_rgb, want_noise = mean_and_noise(S[2], 2)
    assert same(rgb, want_rgb) and same(noise, want_noise)
    assert (info["passes"], info["samples"], info["stage"]) == (1, 2 * W * H, 2) and info["tolerance_reached"] == TOL_MAX


# ---- 6: the command line --------------------------------------------------------------------------------------------------------------------------
def test_cli_sample_budget(fray, gpu, tmp_path):
    sc = os.path.join(ROOT, "scenes", "cornell_box.fray")
    bmp = str(tmp_path / "budget.bmp")
    N = 64 * 48 * 6
    out = run_in_clean_child([sys.executable, "-m", "fray_amd", sc, "--width", "64", "--height", "48", "--refine", "0.1", "--max-spp", "32", "--sample-budget",
                              str(N), "--denoise", "-o", bmp], str(tmp_path / "budget.log"), timeout=300)
    assert "[exit code 0]" in out, out[-2000:]
    line = json.loads(re.search(r'^\{"passes".*\}$', out, re.M).group(0))
    assert 0 < line["samples"] <= N == line["budget"] and line["stage"] in (0, 1, 2) and line["tolerance_reached"] >= 0.1 - 1e-6
    assert line["min_spp"] >= 4                                   # 6 a pixel pays for min_count everywhere
    data = open(bmp, "rb").read()
    assert len(data) >= 54 + 64 * 48 * 3 and any(data[54:])
    px = np.frombuffer(data[54:54 + 64 * 48 * 3], np.uint8)
    assert px.size == 64 * 48 * 3                                 # 8-bit pixels: finite by construction once the file is whole
