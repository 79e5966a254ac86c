"""Component states under a sample map on a real MI355X (include/frayhip.h "sample maps": frayhip_render_components_map, frayhip_sample_map_pair).

After a pair map call each state's row of a pixel that holds N samples must be the row frayhip_render_components leaves for samples 0 .. N-1, bit
for bit, however the samples were cut.  So every check is built from the uniform pair states D_1 .. D_8 and I_1 .. I_8 (.. 32 for refine) that
render_components leaves, one sample at a time, snapshotted once per scene and never written to.  All comparisons are of bits unless said
otherwise."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, bucket_xy, run_in_clean_child
from sample_map_pair_ref import sample_map_pair_ref
from samples_ref import mean_and_noise
from test_gpu_adaptive import CSG, scene, textured_scene
from test_gpu_progressive import COUNTERS
from test_gpu_samples_map import NAN, VALUES, expectation, forced_map, same, synthetic_state

pytestmark = pytest.mark.gpu


def snapshots(s, top=8):
    """([None, D_1 .. D_top], [None, I_1 .. I_top]): the uniform pair states, render_components one sample at a time."""
    D, I, st = [None], [None], None
    for k in range(1, top + 1):
        _, _, st = s.render_components(1, st)
        assert st[0].samples_done == st[1].samples_done == k
        D.append(st[0].state.copy())
        I.append(st[1].state.copy())
    return D, I


_CACHE = {}


def cornell(fray, W, H, top=8):
    """The cornell scene at W x H and its pair snapshots, made once and shared."""
    key = (W, H, top)
    if key not in _CACHE:
        s = scene(fray, "cornell_box.fray", W, H, wantAA=0, numPaths=8)
        _CACHE[key] = (s, snapshots(s, top))
    return _CACHE[key]


def rows_of(S, counts):
    """The rows whose pixel p holds S_{counts[p]}'s, NaN where it holds nothing."""
    rows = np.full(counts.shape + (4,), NAN, np.float32)
    for n in np.unique(counts):
        if n > 0:
            rows[counts == n] = S[n][counts == n]
    return rows


def pair_of(fray, DI, counts, seed=42, share=(0, 1)):
    H, W = counts.shape
    uniform = int(counts.min()) == int(counts.max())
    return tuple(fray.Accumulation(rows_of(S, counts), int(counts.min()), seed, (W, H), share[0], share[1],
                                   None if uniform else counts.astype(np.int32).copy()) for S in DI)


def check_pair(fray, s, DI, add, before=None, **kw):
    """One pair map call from `before` (per-pixel counts; None: empty states of NaN rows) against the snapshots; returns (states, stats)."""
    H, W = add.shape
    before = np.zeros((H, W), np.int32) if before is None else before
    st = pair_of(fray, DI, before)
    rows0 = [a.state.copy() for a in st]
    d_rgb, i_rgb, st, d_noise, i_noise, info = s.render_components_map(add, st, stats=True, noise=True, **kw)
    after = before + add
    for a, S, r0, rgb, noise in zip(st, DI, rows0, (d_rgb, i_rgb), (d_noise, i_noise)):
        rows, want_rgb, want_noise = expectation(S, after, r0)
        assert same(a.count_plane(), after)
        assert same(a.state, rows)                  # NaN sentinels where add == 0 on an empty pixel included
        assert same(rgb, want_rgb) and same(noise, want_noise)
        assert a.samples_done == int(after.min()) and (a.counts is None) == (after.min() == after.max())
    assert st[0].counts is None or st[0].counts is not st[1].counts          # each state carries its own plane
    assert info["samples"] == int(add.sum())
    return st, info


def same_pair(a, b):
    return same(a[0].state, b[0].state) and same(a[1].state, b[1].state) and same(a[0].count_plane(), b[0].count_plane())


# ---- 1: per-pixel equality ------------------------------------------------------------------------------------------------------------------------
def test_every_pixel_equals_the_component_frames_of_its_count(fray, gpu):
    s, DI = cornell(fray, 96, 72)                   # ragged edge buckets; 6912 pixels: a list of several 2048-entry compaction tiles
    add = forced_map(96, 72)
    assert len(np.unique(add)) == 6 and (add[8:16, 16:24] == 0).all() and (add[36] == 0).all() and add[24:35, 40:51].sum() == 8
    st, info = check_pair(fray, s, DI, add)
    for a in st:
        assert np.isnan(a.state[add == 0]).all() and np.isfinite(a.state[add > 0]).all()
    assert (st[1].state[add > 0][:, :3] != 0).any()          # the box has indirect light: the second state is not trivially empty
    assert s.get_option("contracted_launches") == 0


# ---- 2: cutting does not matter -------------------------------------------------------------------------------------------------------------------
def test_cuts_chunks_and_lanes_do_not_matter(fray, gpu):
    s, DI = cornell(fray, 96, 72)
    add = forced_map(96, 72, seed=2)
    H, W = add.shape
    one, _ = check_pair(fray, s, DI, add)
    # two calls, A then B
    A = np.minimum(add, VALUES[np.random.default_rng(3).integers(0, len(VALUES), (H, W))]).astype(np.int32)
    first, _ = check_pair(fray, s, DI, A)
    two = s.render_components_map(add - A, first)[2]
    assert same_pair(two, one) and same(two[0].count_plane(), add)
    # a uniform render_components of 2, then the map on top of it
    uni = s.render_components(2)[2]
    assert same(uni[0].state, DI[0][2]) and same(uni[1].state, DI[1][2])
    more = np.maximum(add - 2, 0).astype(np.int32)
    uni = s.render_components_map(more, uni)[2]
    for a, S in zip(uni, DI):
        assert same(a.state, expectation(S, 2 + more, S[2])[0]) and same(a.count_plane(), 2 + more)
    # a map from counts that are already non-uniform
    before = np.minimum(add, 3).astype(np.int32)
    check_pair(fray, s, DI, add - before, before=before)
    # spp_chunk: a layer boundary at add == cn and at add == cn + 1
    for chunk in (0, 1, 3):
        st, _ = check_pair(fray, s, DI, add, spp_chunk=chunk)
        assert same_pair(st, one)
    cn = 3
    edge = np.where(np.indices(add.shape)[1] % 2 == 0, cn, cn + 1).astype(np.int32)
    check_pair(fray, s, DI, edge, spp_chunk=cn)
    # one lane against four
    default_lanes = s.get_option("pt_lanes")
    for lanes in (1, 4):
        s.set_option("pt_lanes", lanes)
        st, _ = check_pair(fray, s, DI, add)
        assert same_pair(st, one)
    s.set_option("pt_lanes", default_lanes)


def test_a_small_budget_splits_the_list_into_pixel_ranges(fray, gpu):
    s = scene(fray, "cornell_box.fray", 640, 480, wantAA=0, numPaths=2)
    DI = snapshots(s, 2)
    add = (1 + np.random.default_rng(6).integers(0, 2, (480, 640))).astype(np.int32)
    one, info_one = check_pair(fray, s, DI, add, spp_chunk=1)
    s.set_option("pt_budget_mib", 1)
    st, info = check_pair(fray, s, DI, add, spp_chunk=1)
    assert same_pair(st, one)
    assert info["trace_launches"] > info_one["trace_launches"], (info["trace_launches"], info_one["trace_launches"])
    s.close()


# ---- 3: a uniform map is render_components --------------------------------------------------------------------------------------------------------
def test_uniform_map_equals_render_components(fray, gpu):
    s, DI = cornell(fray, 96, 72)
    n, k = 3, 4
    H, W = 72, 96
    fresh = lambda: tuple(fray.Accumulation(S[n].copy(), n, 42, (W, H)) for S in DI)
    _, _, want, want_nd, want_ni, want_info = s.render_components(k, fresh(), stats=True, noise=True)
    full = np.full((H, W), k, np.int32)
    _, _, got, nd, ni, info = s.render_components_map(full, fresh(), stats=True, noise=True)
    assert same_pair(got, want) and same(got[0].state, DI[0][n + k]) and same(got[1].state, DI[1][n + k])
    assert same(nd, want_nd) and same(ni, want_ni)
    assert all(a.counts is None and a.samples_done == n + k for a in got)
    for c in COUNTERS:
        assert info[c] == want_info[c], (c, info[c], want_info[c])
    assert info["samples"] == k * W * H and info["closest_rays"] > 0
    # the same rays as the single-state map of the same add
    add = forced_map(W, H, seed=5)
    _, _, _, pinfo = s.render_components_map(add, None, stats=True)
    _, _, sinfo = s.render_samples_map(add, None, stats=True)
    for c in COUNTERS:
        assert pinfo[c] == sinfo[c], (c, pinfo[c], sinfo[c])
    assert pinfo["samples"] == sinfo["samples"] == int(add.sum())


# ---- 4: kernel families ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = [
    ("smallpt", "smallpt.fray", dict(wantAA=0, numPaths=8)),
    ("boxed-kd", "boxed.fray", dict(wantAA=0, gi=1, numPaths=8)),
    ("csg", CSG, dict(wantAA=0, gi=1, numPaths=8)),
    ("cornell-dof", "cornell_box.fray", dict(wantAA=0, numPaths=8, dof=1, numDOFSamples=2, fNumber=2.0, focalPlaneDist=800.0)),
]


def raw_pair(fray, s, add, rows, count, counting=False, share=(0, 1), outs=None, expect=0):
    """frayhip_render_components_map itself, with or without FRAYHIP_FRAME_STATS; rows: the two states, written in place."""
    abi = fray.abi
    H, W = add.shape
    outs = outs or [np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)]
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=share[0], bucket_stride=share[1], spp_chunk=0, flags=abi.FRAME_STATS if counting else 0)
    req, st = abi.SamplesMap(), abi.Stats()
    rc = fray.lib.frayhip_render_components_map(s._dev, C.byref(fr), C.byref(req), rows[0].ctypes.data, rows[1].ctypes.data, count.ctypes.data,
                                                add.ctypes.data, outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data,
                                                C.byref(st))
    assert rc == expect, fray.lib.frayhip_last_error()
    return outs, req, st.as_dict()


def check_family(fray, s, counting, DI=None):
    DI = DI or snapshots(s)
    add = forced_map(64, 48)
    rows = [np.full((48, 64, 4), NAN, np.float32) for _ in range(2)]
    count = np.zeros((48, 64), np.int32)
    want = [expectation(S, add, r) for S, r in zip(DI, rows)]
    outs, req, info = raw_pair(fray, s, add, rows, count, counting)
    assert same(count, add)
    for k in range(2):
        assert same(rows[k], want[k][0]) and same(outs[k], want[k][1]) and same(outs[2 + k], want[k][2])
    assert info["samples"] == int(add.sum()) == req.samples and (req.count_min, req.count_max) == (0, 8)
    assert (info["closest_rays"] > 0 and info["shadow_rays"] > 0) if counting else info["closest_rays"] == 0
    return DI


@pytest.mark.parametrize("case", FAMILIES, ids=[c[0] for c in FAMILIES])
def test_kernel_families(fray, gpu, case):
    _, name, over = case
    s = scene(fray, name, 64, 48, **over)
    DI = check_family(fray, s, False)
    check_family(fray, s, True, DI)
    s.close()


def test_textured_family(fray, gpu, tmp_path):
    s = textured_scene(fray, tmp_path, 64, 48, 8)                                      # flag words 8 / 9
    DI = check_family(fray, s, False)
    check_family(fray, s, True, DI)
    s.close()


# ---- 5, 6: the shortest term lists ---------------------------------------------------------------------------------------------------------------
def test_depth_zero_has_no_indirect_light(fray, gpu):
    """maxTraceDepth = 0: nBounce = 2, the fold's destination is the last term plane."""
    s = scene(fray, "cornell_box.fray", 64, 48, wantAA=0, numPaths=8, maxTraceDepth=0)
    add = forced_map(64, 48)
    d_rgb, i_rgb, st, nd, ni = s.render_components_map(add, None, noise=True)
    rgb, one, noise = s.render_samples_map(add, None, noise=True)
    assert same(st[0].count_plane(), add) and same(one.count_plane(), add)
    assert (st[1].state == 0).all() and (i_rgb == 0).all() and (ni == 0).all()
    assert np.array_equal(st[0].state, one.state) and np.array_equal(d_rgb, rgb) and np.array_equal(nd, noise)          # by value
    assert (st[0].state[add > 0][:, :3] != 0).any()
    DI = snapshots(s)
    check_pair(fray, s, DI, add)
    s.close()


def test_black_frames_add_zero_to_both_states_and_count_once(fray, gpu):
    s = scene(fray, "cornell_box.fray", 64, 48, wantAA=0, numPaths=8, maxTraceDepth=-1)
    add = forced_map(64, 48)
    d_rgb, i_rgb, st, nd, ni, info = s.render_components_map(add, None, stats=True, noise=True)
    assert info["samples"] == int(add.sum())
    for a, rgb, noise in zip(st, (d_rgb, i_rgb), (nd, ni)):
        assert same(a.count_plane(), add) and (a.state == 0).all() and (rgb == 0).all() and (noise == 0).all()
    s.close()


# ---- 7: per-sample identity -----------------------------------------------------------------------------------------------------------------------
def test_single_sample_is_direct_plus_indirect(fray, gpu):
    s, _ = cornell(fray, 96, 72)
    H, W = 72, 96
    count = np.random.default_rng(11).integers(0, 8, (H, W)).astype(np.int32)
    one = np.ones((H, W), np.int32)
    zero = lambda: fray.Accumulation(np.zeros((H, W, 4), np.float32), 0, 42, (W, H), counts=count.copy())
    pair = s.render_components_map(one, (zero(), zero()))[2]
    single = s.render_samples_map(one, zero())[1]
    assert same(pair[0].count_plane(), count + 1) and same(single.count_plane(), count + 1)
    assert same(single.state[..., :3], pair[0].state[..., :3] + pair[1].state[..., :3])
    assert len(np.unique(count)) == 8 and (pair[1].state[..., :3] != 0).any()


# ---- 8: buckets -----------------------------------------------------------------------------------------------------------------------------------
def test_other_buckets_are_untouched_in_all_seven_buffers(fray, gpu):
    s, DI = cornell(fray, 96, 72)
    W, H = 96, 72
    mine = np.zeros((H, W), bool)
    for b in range(1, 4, 2):                                  # buckets 1 and 3 of the frame's 2 x 2
        bx, by = bucket_xy(W, b)
        mine[by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48] = True
    assert mine.any() and not mine.all()
    add = forced_map(W, H)
    add[~mine] = -7                                           # not read: a negative value there is not an error
    rows = [np.full((H, W, 4), NAN, np.float32) for _ in range(2)]
    count = np.full((H, W), 5, np.int32)
    count[mine] = 0
    outs = [np.full((H, W, 3), 7.0, np.float32), np.full((H, W, 3), 8.0, np.float32), np.full((H, W), 9.0, np.float32), np.full((H, W), 10.0, np.float32)]
    before = [o.copy() for o in outs]
    outs, req, info = raw_pair(fray, s, add, rows, count, share=(1, 2), outs=outs)
    after = np.where(mine, add, 0)
    assert same(count, np.where(mine, add, 5).astype(np.int32))
    for k in range(2):
        want_rows, want_rgb, want_noise = expectation(DI[k], after, np.full((H, W, 4), NAN, np.float32))
        assert same(rows[k], want_rows)
        assert same(outs[k][mine], want_rgb[mine]) and same(outs[2 + k][mine], want_noise[mine])
        assert same(outs[k][~mine], before[k][~mine]) and same(outs[2 + k][~mine], before[2 + k][~mine])
    assert info["samples"] == int(add[mine].sum()) == req.samples
    # inside the share the planes are checked
    bad = np.where(mine, -1, 0).astype(np.int32)
    with pytest.raises(fray.FrayError, match="frayhip_render_components_map:.*add < 0"):
        s.render_components_map(bad, tuple(fray.Accumulation.empty((W, H), 42, 1, 2) for _ in range(2)), bucket_first=1, bucket_stride=2)


# ---- 9: the device entry --------------------------------------------------------------------------------------------------------------------------
def test_device_entry_equals_host_entry_and_checks_in_its_first_kernel(fray, gpu):
    import torch
    s, DI = cornell(fray, 96, 72)
    add = forced_map(96, 72)
    host, _ = check_pair(fray, s, DI, add)
    dev = tuple(fray.Accumulation(torch.full((72, 96, 4), float("nan"), dtype=torch.float32, device="cuda"), 0, 42, (96, 72)) for _ in range(2))
    d_rgb, i_rgb, dev, nd, ni, info = s.render_components_map(torch.from_numpy(add).cuda(), dev, stats=True, noise=True)
    for k, (rgb, noise) in enumerate(((d_rgb, nd), (i_rgb, ni))):
        assert same(dev[k].state.cpu().numpy(), host[k].state) and same(dev[k].count_plane().cpu().numpy(), add)
        _, want_rgb, want_noise = expectation(DI[k], add, host[k].state)
        assert same(rgb.cpu().numpy(), want_rgb) and same(noise.cpu().numpy(), want_noise)
    assert info["samples"] == int(add.sum())
    # a bad plane: E_ARG from the first kernel, nothing written
    bad = torch.from_numpy(add).cuda()
    bad[5, 5] = -1
    before = [a.state.clone() for a in dev]
    counts = [a.count_plane().clone() for a in dev]
    with pytest.raises(fray.FrayError, match="frayhip_render_components_map_device.*add < 0") as e:
        s.render_components_map(bad, dev)
    assert e.value.code == fray.abi.E_ARG
    for k in range(2):
        assert torch.equal(dev[k].count_plane(), counts[k]) and same(dev[k].state.cpu().numpy(), before[k].cpu().numpy())
    over = torch.zeros_like(bad)
    over[0, 0] = (1 << 24) - int(counts[0][0, 0]) + 1
    with pytest.raises(fray.FrayError, match="2\\^24"):
        s.render_components_map(over, dev)


# ---- 10: side effects -----------------------------------------------------------------------------------------------------------------------------
def test_empty_map_frames_before_and_after_and_fp_contract(fray, gpu):
    s, DI = cornell(fray, 96, 72)
    figures = lambda: [s.get_option(k) for k in ("seed_table_bytes", "seed_launches", "seed_planes_reused")]
    s.render(seed=42)                                         # the frame that fills the seed table
    frame0, _ = s.render(seed=42)
    table = figures()
    add = forced_map(96, 72)
    # an all-zero map: OK, no sample, no tracing kernel; the component frames of what the states hold
    st = tuple(fray.Accumulation(S[4].copy(), 4, 42, (96, 72)) for S in DI)
    d_rgb, i_rgb, st, nd, ni, info = s.render_components_map(np.zeros_like(add), st, stats=True, noise=True)
    assert info["samples"] == 0 and info["trace_launches"] == 0 and info["shadow_launches"] == 0
    for a, S, rgb, noise in zip(st, DI, (d_rgb, i_rgb), (nd, ni)):
        want_rgb, want_noise = mean_and_noise(S[4], 4)
        assert same(a.state, S[4]) and a.samples_done == 4 and a.counts is None and same(rgb, want_rgb) and same(noise, want_noise)
    one, _ = check_pair(fray, s, DI, add)
    frame1, _ = s.render(seed=42)
    assert same(frame0, frame1)
    assert figures() == table                                 # the map call neither read nor altered the table
    s.set_option("fp_contract", 1)
    two, _ = check_pair(fray, s, DI, add)
    assert s.get_option("contracted_launches") == 0 and same_pair(two, one)
    s.set_option("fp_contract", 0)


# ---- 11: the pair sample_map ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [dict(tolerance=0.05, max_count=64), dict(tolerance=0.2, max_count=64, grow=16, max_add=5),
                                    dict(tolerance=0.5, lum_floor=0.5, min_count=1, max_count=48, grow=3)], ids=["defaults", "caps", "floor"])
def test_pair_sample_map_equals_its_restatement(fray, gpu, params):
    import torch
    state, count = synthetic_state()
    s, DI = cornell(fray, 96, 72)
    rendered = forced_map(96, 72, seed=4)
    rendered[rendered == 0] = 6
    cases = [(state * np.float32(0.75), state[::-1].copy() * np.float32(0.3125), count),
             (rows_of(DI[0], rendered), rows_of(DI[1], rendered), rendered)]
    for d, i, cnt in cases:
        H, W = cnt.shape
        want, pixels, samples = sample_map_pair_ref(d, i, cnt, **params)
        uniform = cnt.min() == cnt.max()
        st = tuple(fray.Accumulation(r.copy(), int(cnt.min()), 42, (W, H), counts=None if uniform else cnt.copy()) for r in (d, i))
        add, info = fray.sample_map(st, **params)
        assert same(add, want), (np.argwhere(add != want)[:5], add[add != want][:5], want[add != want][:5])
        assert info == {"pixels": pixels, "samples": samples}
        dev = tuple(fray.Accumulation(torch.from_numpy(r.copy()).cuda(), int(cnt.min()), 42, (W, H),
                                      counts=None if uniform else torch.from_numpy(cnt).cuda()) for r in (d, i))
        dadd, dinfo = fray.sample_map(dev, **params)
        assert same(dadd.cpu().numpy(), want) and dinfo == info
    assert len(np.unique(sample_map_pair_ref(cases[0][0], cases[0][1], count, **params)[0])) >= 4


# ---- 12: refine -----------------------------------------------------------------------------------------------------------------------------------
def simulate_refine(DI, shape, passes, **params):
    """Scene.refine on a pair from the snapshots alone: the counts after each pass of sample_map_pair_ref."""
    counts = np.zeros(shape, np.int32)
    rows = [np.zeros(shape + (4,), np.float32) for _ in range(2)]
    done = 0
    for _ in range(passes):
        for n in np.unique(counts):
            if n > 0:
                for r, S in zip(rows, DI):
                    r[counts == n] = S[n][counts == n]
        add, pixels, _ = sample_map_pair_ref(rows[0], rows[1], counts, **params)
        if pixels == 0:
            break
        counts = counts + add
        done += 1
    return counts, done


def test_refine_on_a_pair_reaches_the_simulated_counts(fray, gpu):
    s, DI = cornell(fray, 64, 48, top=32)
    H, W = 48, 64
    # the tolerance at which a pixel of the pair at 4 samples asks for exactly the samples it has; a quantile of it splits the frame
    lum = lambda rgb: ((rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]) / np.float32(3)
    (rd, nd), (ri, ni) = mean_and_noise(DI[0][4], 4), mean_and_noise(DI[1][4], 4)
    tau = np.sqrt(nd + ni) / np.maximum(lum(rd) + lum(ri), np.float32(0.01))
    tau = tau[np.isfinite(tau) & (tau > 0)]
    for q in (0.5, 0.35, 0.65, 0.2, 0.8, 0.1, 0.9):
        params = dict(tolerance=float(np.quantile(tau, q)), min_count=4, max_count=32)
        want, passes = simulate_refine(DI, (H, W), 8, **params)
        if len(np.unique(want)) >= 3:
            break
    else:
        pytest.fail("no quantile of the first pass's need leaves three distinct final counts")
    d_rgb, i_rgb, st, d_noise, i_noise, info = s.refine(None, passes=8, split=True, **params)
    assert same(st[0].count_plane(), want), (np.unique(st[0].count_plane(), return_counts=True), np.unique(want, return_counts=True))
    assert same(st[1].count_plane(), want)
    for a, S, rgb, noise in zip(st, DI, (d_rgb, i_rgb), (d_noise, i_noise)):
        rows, want_rgb, want_noise = expectation(S, want, np.zeros((H, W, 4), np.float32))
        assert same(a.state, rows) and same(rgb, want_rgb) and same(noise, want_noise)
    assert info["passes"] == passes and info["samples"] == int(want.sum())
    assert want.min() >= 4 and want.max() <= 32 and len(np.unique(want)) >= 3
    # a pair handed in is continued: nothing more is asked of it unless the passes ran out
    again, more = fray.sample_map(st, **params)
    assert more["pixels"] == 0 or info["passes"] == 8


# ---- 13: the split filter on a refined pair -------------------------------------------------------------------------------------------------------
def test_render_denoised_split_with_refine(fray, gpu):
    s, _ = cornell(fray, 64, 48, top=32)
    out, raw, info = s.render_denoised_split(refine=0.1, max_count=32)
    assert out.shape == raw.shape == (48, 64, 3) and np.isfinite(out).all() and np.isfinite(raw).all()
    assert same(raw, info["direct_rgb"] + info["indirect_rgb"])
    held = info["refine"]["counts"]
    assert held.shape == (48, 64) and held.min() >= 4 and held.max() <= 32
    assert info["refine"]["samples"] == int(held.sum()) and info["refine"]["passes"] >= 1
    assert np.isfinite(info["noise_direct"]).all() and np.isfinite(info["noise_indirect"]).all()
    plain = s.render_denoised_split()
    assert "refine" not in plain[2] and np.isfinite(plain[0]).all()


def test_cli_refine_split_denoise_writes_a_finite_image(fray, gpu, tmp_path):
    sc = os.path.join(ROOT, "scenes", "cornell_box.fray")
    comp, bmp = str(tmp_path / "components.npz"), str(tmp_path / "refined.bmp")
    out = run_in_clean_child([sys.executable, "-m", "fray_amd", sc, "--width", "64", "--height", "48", "--refine", "0.1", "--max-spp", "32", "--denoise",
                              "--split", "--components-out", comp, "-o", bmp], str(tmp_path / "refine_split.log"), timeout=300)
    assert "[exit code 0]" in out, out[-2000:]
    with np.load(comp) as z:
        for k in ("direct", "indirect", "noise_direct", "noise_indirect"):
            assert np.isfinite(z[k]).all(), k
        assert z["direct"].shape == (48, 64, 3) and 4 <= int(z["samples"]) <= 32
    held = re.search(r'"min_spp": (\d+), "max_spp": (\d+)', out)
    assert held and 4 <= int(held.group(1)) <= int(held.group(2)) <= 32, out[-2000:]
    data = open(bmp, "rb").read()
    assert len(data) >= 54 + 64 * 48 * 3 and any(data[54:])
