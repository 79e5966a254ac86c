"""Sample maps on a real MI355X (include/frayhip.h "sample maps"): per-pixel sample counts on a resumable frame.

After a map call a pixel that holds N samples must be that pixel of the N-sample frame, bit for bit, however the samples were cut into map calls,
uniform calls and batches.  So every check here is built from the uniform states S_1 .. S_8 (S_32 for refine) that render_samples leaves, one
sample at a time, snapshotted once per scene: the expected row, rgb and noise of pixel p come from S_{count[p]}.  All comparisons are of bits."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, bucket_xy, run_in_clean_child
from sample_map_ref import sample_map_ref
from samples_ref import mean_and_noise
from test_gpu_adaptive import CSG, scene, textured_scene
from test_gpu_progressive import COUNTERS

pytestmark = pytest.mark.gpu

VALUES = np.array([0, 1, 2, 3, 5, 8], np.int32)
NAN = np.float32(np.nan)


def snapshots(s, top=8):
    """[None, S_1, ..., S_top]: the uniform states, render_samples one sample at a time."""
    out, st = [None], None
    for k in range(1, top + 1):
        _, st = s.render_samples(1, st)
        assert st.samples_done == k
        out.append(st.state.copy())
    return out


_CACHE = {}


def cornell(fray, W, H, top=8):
    """The cornell scene at W x H and its snapshots, made once and shared (the snapshots are never written to)."""
    key = (W, H, top)
    if key not in _CACHE:
        s = scene(fray, "cornell_box.fray", W, H, wantAA=0, numPaths=8)
        _CACHE[key] = (s, snapshots(s, top))
    return _CACHE[key]


def forced_map(W, H, seed=1):
    """add over {0, 1, 2, 3, 5, 8} from a fixed generator, with a whole 8x8 tile of zeros, a whole row of zeros and one pixel of 8 among zeros."""
    add = VALUES[np.random.default_rng(seed).integers(0, len(VALUES), (H, W))]
    add[8:16, 16:24] = 0
    add[H // 2, :] = 0
    add[24:35, 40:51] = 0
    add[29, 45] = 8
    return np.ascontiguousarray(add, np.int32)


def state_of(fray, S, counts, seed=42, share=(0, 1)):
    """The state whose pixel p holds S_{counts[p]}'s row, NaN where it holds nothing."""
    H, W = counts.shape
    rows = np.full((H, W, 4), NAN, np.float32)
    for n in np.unique(counts):
        if n > 0:
            rows[counts == n] = S[n][counts == n]
    uniform = int(counts.min()) == int(counts.max())
    return fray.Accumulation(rows, int(counts.min()), seed, (W, H), share[0], share[1], None if uniform else counts.astype(np.int32).copy())


def expectation(S, counts, rows_before):
    """(rows, rgb, noise) of a frame whose pixel p holds counts[p] samples; pixels that hold none keep their row and show (0, 0, 0), noise 0."""
    rows = rows_before.copy()
    rgb = np.zeros(counts.shape + (3,), np.float32)
    noise = np.zeros(counts.shape, np.float32)
    for n in np.unique(counts):
        if n > 0:
            m = counts == n
            r, v = mean_and_noise(S[n], int(n))
            rows[m], rgb[m], noise[m] = S[n][m], r[m], v[m]
    return rows, rgb, noise


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_map(fray, s, S, add, before=None, **kw):
    """One map call from `before` (per-pixel counts; None: an empty state of NaN rows) against the snapshots; returns (state, stats)."""
    H, W = add.shape
    before = np.zeros((H, W), np.int32) if before is None else before
    st = state_of(fray, S, before)
    rows0 = st.state.copy()
    rgb, st, noise, info = s.render_samples_map(add, st, stats=True, noise=True, **kw)
    after = before + add
    rows, want_rgb, want_noise = expectation(S, after, rows0)
    assert same(st.count_plane(), after)
    assert same(st.state, rows)                     # NaN sentinels where add == 0 on an empty pixel included
    assert same(rgb, want_rgb) and same(noise, want_noise)
    assert info["samples"] == int(add.sum())
    assert st.samples_done == int(after.min())
    assert (st.counts is None) == (after.min() == after.max())
    return st, info


# ---- 1: per-pixel equality ------------------------------------------------------------------------------------------------------------------------
def test_every_pixel_equals_the_frame_of_its_count(fray, gpu):
    s, S = cornell(fray, 96, 72)                    # ragged edge buckets; 6912 pixels: a list of several 2048-entry compaction tiles
    add = forced_map(96, 72)
    assert len(np.unique(add)) == 6 and (add[8:16, 16:24] == 0).all() and (add[36] == 0).all() and add[24:35, 40:51].sum() == 8
    st, info = check_map(fray, s, S, add)
    assert np.isnan(st.state[add == 0]).all() and np.isfinite(st.state[add > 0]).all()
    assert s.get_option("contracted_launches") == 0


# ---- 2: cutting does not matter -------------------------------------------------------------------------------------------------------------------
def test_cuts_chunks_budgets_and_lanes_do_not_matter(fray, gpu):
    s, S = cornell(fray, 96, 72)
    add = forced_map(96, 72, seed=2)
    H, W = add.shape
    one, info_one = check_map(fray, s, S, add)
    # two calls, A then B
    A = np.minimum(add, VALUES[np.random.default_rng(3).integers(0, len(VALUES), (H, W))]).astype(np.int32)
    first, _ = check_map(fray, s, S, A)
    rgb, two, noise = s.render_samples_map(add - A, first, noise=True)
    assert same(two.state, one.state) and same(two.count_plane(), add)
    # a uniform render_samples of 2, then the map on top of it
    _, uni = s.render_samples(2)
    assert same(uni.state, S[2])
    more = np.maximum(add - 2, 0).astype(np.int32)
    _, uni = s.render_samples_map(more, uni)
    want, _, _ = expectation(S, 2 + more, S[2])
    assert same(uni.state, want) and same(uni.count_plane(), 2 + more)
    # a map from counts that are already non-uniform
    before = np.minimum(add, 3).astype(np.int32)
    check_map(fray, s, S, add - before, before=before)
    # spp_chunk: a layer boundary at add == cn and at add == cn + 1 (values 1, 2 / 3 and 5 / 8 lie on either side of 1 and of 3)
    for chunk in (0, 1, 3):
        st, _ = check_map(fray, s, S, add, spp_chunk=chunk)
        assert same(st.state, one.state)
    cn = 3
    assert (add == cn).any() and (add == cn - 1).any() and (add > cn).any()
    edge = np.where(np.indices(add.shape)[1] % 2 == 0, cn, cn + 1).astype(np.int32)
    check_map(fray, s, S, edge, spp_chunk=cn)
    # one lane against four
    default_lanes = s.get_option("pt_lanes")
    for lanes in (1, 4):
        s.set_option("pt_lanes", lanes)
        st, _ = check_map(fray, s, S, add)
        assert same(st.state, one.state)
    s.set_option("pt_lanes", default_lanes)


def test_a_small_budget_splits_the_list_into_pixel_ranges(fray, gpu):
    """The smallest budget a frame plans with (64 MiB) holds some 200 000 paths: a list of 640 x 480 pixels is cut into several ranges."""
    s = scene(fray, "cornell_box.fray", 640, 480, wantAA=0, numPaths=2)
    S = snapshots(s, 2)
    add = (1 + np.random.default_rng(6).integers(0, 2, (480, 640))).astype(np.int32)
    one, info_one = check_map(fray, s, S, add, spp_chunk=1)
    s.set_option("pt_budget_mib", 1)
    st, info = check_map(fray, s, S, add, spp_chunk=1)
    assert same(st.state, one.state)
    assert info["trace_launches"] > info_one["trace_launches"], (info["trace_launches"], info_one["trace_launches"])
    s.close()


# ---- 3: a uniform map is render_samples ----------------------------------------------------------------------------------------------------------
def test_uniform_map_equals_render_samples(fray, gpu):
    s, S = cornell(fray, 96, 72)
    n, k = 3, 4
    H, W = 72, 96
    base = fray.Accumulation(S[n].copy(), n, 42, (W, H))
    _, want, want_noise, want_info = s.render_samples(k, base, stats=True, noise=True)
    got = fray.Accumulation(S[n].copy(), n, 42, (W, H))
    rgb, got, noise, info = s.render_samples_map(np.full((H, W), k, np.int32), got, stats=True, noise=True)
    assert same(got.state, want.state) and same(got.state, S[n + k]) and same(noise, want_noise)
    assert got.counts is None and got.samples_done == n + k
    for c in COUNTERS:
        assert info[c] == want_info[c], (c, info[c], want_info[c])
    assert info["samples"] == k * W * H and info["closest_rays"] > 0


# ---- 4: kernel families ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = [
    ("smallpt", "smallpt.fray", dict(wantAA=0, numPaths=8), False),
    ("boxed-kd", "boxed.fray", dict(wantAA=0, gi=1, numPaths=8), False),
    ("csg", CSG, dict(wantAA=0, gi=1, numPaths=8), False),
    ("cornell-dof", "cornell_box.fray", dict(wantAA=0, numPaths=8, dof=1, numDOFSamples=2, fNumber=2.0, focalPlaneDist=800.0), False),
    ("cornell-stats", "cornell_box.fray", dict(wantAA=0, numPaths=8), True),
    ("csg-stats", CSG, dict(wantAA=0, gi=1, numPaths=8), True),
]


def raw_map(fray, s, add, rows, count, counting):
    """frayhip_render_samples_map itself, with or without FRAYHIP_FRAME_STATS (the Python call sets the flag whenever it returns the stats)."""
    import ctypes as C
    abi = fray.abi
    H, W = add.shape
    rgb, noise = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, flags=abi.FRAME_STATS if counting else 0)
    req, st = abi.SamplesMap(), abi.Stats()
    rc = fray.lib.frayhip_render_samples_map(s._dev, C.byref(fr), C.byref(req), rows.ctypes.data, count.ctypes.data, add.ctypes.data, rgb.ctypes.data,
                                             noise.ctypes.data, C.byref(st))
    assert rc == 0, fray.lib.frayhip_last_error()
    return rgb, noise, req, st.as_dict()


def check_family(fray, s, counting):
    S = snapshots(s)
    add = forced_map(64, 48)
    rows = np.full((48, 64, 4), NAN, np.float32)
    count = np.zeros((48, 64), np.int32)
    want_rows, want_rgb, want_noise = expectation(S, add, rows)
    rgb, noise, req, info = raw_map(fray, s, add, rows, count, counting)
    assert same(rows, want_rows) and same(count, add) and same(rgb, want_rgb) and same(noise, want_noise)
    assert info["samples"] == int(add.sum()) == req.samples and (req.count_min, req.count_max) == (0, 8)
    assert (info["closest_rays"] > 0 and info["shadow_rays"] > 0) if counting else info["closest_rays"] == 0


@pytest.mark.parametrize("case", FAMILIES, ids=[c[0] for c in FAMILIES])
def test_kernel_families(fray, gpu, case):
    _, name, over, counting = case
    s = scene(fray, name, 64, 48, **over)
    check_family(fray, s, counting)
    s.close()


def test_textured_family(fray, gpu, tmp_path):
    s = textured_scene(fray, tmp_path, 64, 48, 8)                                      # flag words 8 / 9
    for counting in (False, True):
        check_family(fray, s, counting)
    s.close()


# ---- 5: buckets and entries -----------------------------------------------------------------------------------------------------------------------
def test_other_buckets_are_untouched_and_their_add_is_not_read(fray, gpu):
    s, S = cornell(fray, 96, 72)
    W, H = 96, 72
    mine = np.zeros((H, W), bool)
    for b in range(1, 4, 2):                                  # buckets 1 and 3 of the frame's 2 x 2
        bx, by = bucket_xy(W, b)
        mine[by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48] = True
    assert mine.any() and not mine.all()
    add = forced_map(W, H)
    add[~mine] = -7                                           # not read: a negative value there is not an error
    rows = np.full((H, W, 4), NAN, np.float32)
    count = np.full((H, W), 5, np.int32)
    count[mine] = 0
    st = fray.Accumulation(rows.copy(), 0, 42, (W, H), 1, 2, count.copy())
    rgb, st, noise, info = s.render_samples_map(add, st, bucket_first=1, bucket_stride=2, stats=True, noise=True)
    after = np.where(mine, add, 0)
    want_rows, want_rgb, want_noise = expectation(S, after, rows)
    assert same(st.state, want_rows)
    assert same(st.counts, np.where(mine, add, 5).astype(np.int32))
    assert same(rgb[mine], want_rgb[mine]) and same(noise[mine], want_noise[mine])
    assert (rgb[~mine] == 0).all() and (noise[~mine] == 0).all()          # the zeros the Python side allocated
    assert info["samples"] == int(add[mine].sum())
    # inside the share the planes are checked
    bad = np.where(mine, -1, 0).astype(np.int32)
    with pytest.raises(fray.FrayError, match="add < 0"):
        s.render_samples_map(bad, fray.Accumulation.empty((W, H), 42, 1, 2), bucket_first=1, bucket_stride=2)


def test_device_entry_equals_host_entry_and_checks_in_its_first_kernel(fray, gpu):
    import torch
    s, S = cornell(fray, 96, 72)
    add = forced_map(96, 72)
    host, _ = check_map(fray, s, S, add)
    dev = fray.Accumulation(torch.full((72, 96, 4), float("nan"), dtype=torch.float32, device="cuda"), 0, 42, (96, 72))
    rgb, dev, noise, info = s.render_samples_map(torch.from_numpy(add).cuda(), dev, stats=True, noise=True)
    assert same(dev.state.cpu().numpy(), host.state) and same(dev.count_plane().cpu().numpy(), add)
    _, want_rgb, want_noise = expectation(S, add, host.state)
    assert same(rgb.cpu().numpy(), want_rgb) and same(noise.cpu().numpy(), want_noise)
    assert info["samples"] == int(add.sum())
    # a bad plane: E_ARG from the first kernel, nothing written
    bad = torch.from_numpy(add).cuda()
    bad[5, 5] = -1
    before = dev.state.clone()
    counts = dev.count_plane().clone()
    with pytest.raises(fray.FrayError, match="frayhip_render_samples_map_device.*add < 0") as e:
        s.render_samples_map(bad, dev)
    assert e.value.code == fray.abi.E_ARG
    assert torch.equal(dev.count_plane(), counts) and same(dev.state.cpu().numpy(), before.cpu().numpy())
    over = torch.zeros_like(bad)
    over[0, 0] = (1 << 24) - int(counts[0, 0]) + 1
    with pytest.raises(fray.FrayError, match="2\\^24"):
        s.render_samples_map(over, dev)


def test_empty_map_frames_before_and_after_and_fp_contract(fray, gpu):
    s, S = cornell(fray, 96, 72)
    figures = lambda: [s.get_option(k) for k in ("seed_table_bytes", "seed_launches", "seed_planes_reused")]
    s.render(seed=42)                                         # the frame that fills the seed table
    frame0, _ = s.render(seed=42)
    table = figures()
    add = forced_map(96, 72)
    # an all-zero map: OK, no sample, no tracing kernel; the frame of what the state holds
    st = fray.Accumulation(S[4].copy(), 4, 42, (96, 72))
    rgb, st, noise, info = s.render_samples_map(np.zeros_like(add), st, stats=True, noise=True)
    want_rgb, want_noise = mean_and_noise(S[4], 4)
    assert info["samples"] == 0 and info["trace_launches"] == 0 and info["shadow_launches"] == 0
    assert same(st.state, S[4]) and st.samples_done == 4 and st.counts is None and same(rgb, want_rgb) and same(noise, want_noise)
    one, _ = check_map(fray, s, S, add)
    assert s.get_option("seed_table_bytes") == table[0]
    frame1, _ = s.render(seed=42)
    assert same(frame0, frame1) and same(frame0, mean_and_noise(S[8], 8)[0])
    assert figures() == table                                 # the map call neither read nor altered the table
    s.set_option("fp_contract", 1)
    two, _ = check_map(fray, s, S, add)
    assert s.get_option("contracted_launches") == 0 and same(two.state, one.state)
    s.set_option("fp_contract", 0)


def test_black_frames_add_zero_and_count(fray, gpu):
    s = scene(fray, "cornell_box.fray", 64, 48, wantAA=0, numPaths=8, maxTraceDepth=-1)
    add = forced_map(64, 48)
    rgb, st, noise, info = s.render_samples_map(add, None, stats=True, noise=True)
    assert info["samples"] == int(add.sum()) and same(st.count_plane(), add)
    assert (st.state == 0).all() and (rgb == 0).all() and (noise == 0).all()
    s.close()


# ---- 6: sample_map on the GPU ---------------------------------------------------------------------------------------------------------------------
def synthetic_state(W=37, H=29):
    """Every case of tests/test_sample_map_abi.py in one plane: counts 0, 1, min_count, max_count and past it; v = 0; lbar below the floor; NaN rows;
    needs far above max_count; rows where grow and where max_add binds; over a random background."""
    rng = np.random.default_rng(9)
    count = rng.integers(0, 70, (H, W)).astype(np.int32)
    lum = rng.random((H, W), dtype=np.float32) * np.float32(2.0)
    var = rng.random((H, W), dtype=np.float32) ** 4
    n = count.astype(np.float32)
    state = np.stack([n * lum, n * lum * np.float32(0.5), n * lum * np.float32(1.5), n * (var + lum * lum)], axis=-1).astype(np.float32)
    count[0, :8] = [0, 1, 4, 64, 65, 2, 3, 63]
    state[1, :] = np.float32(0.25) * np.stack([n[1], n[1], n[1], n[1] * np.float32(0.25)], axis=-1)          # v = 0
    state[2, :, :3] *= np.float32(1e-4)                                                                   # lbar below the floor
    state[3, ::2] = NAN
    state[4, :, 3] = np.float32(1e30)
    state[5, :, 3] = np.inf
    state[6, :] = 0
    return state, count


@pytest.mark.parametrize("params", [dict(tolerance=0.05, max_count=64), dict(tolerance=0.2, max_count=64, grow=16, max_add=5),
                                    dict(tolerance=0.5, lum_floor=0.5, min_count=1, max_count=48, grow=3)], ids=["defaults", "caps", "floor"])
def test_sample_map_equals_its_restatement(fray, gpu, params):
    import torch
    state, count = synthetic_state()
    s, S = cornell(fray, 96, 72)
    rendered = forced_map(96, 72, seed=4)
    rendered[rendered == 0] = 6
    cases = [(state, count), (state_of(fray, S, rendered).state, rendered)]
    for rows, cnt in cases:
        H, W = cnt.shape
        want, pixels, samples = sample_map_ref(rows, cnt, **params)
        uniform = cnt.min() == cnt.max()
        st = fray.Accumulation(rows.copy(), int(cnt.min()), 42, (W, H), counts=None if uniform else cnt.copy())
        add, info = fray.sample_map(st, **params)
        assert same(add, want), (np.argwhere(add != want)[:5], add[add != want][:5], want[add != want][:5])
        assert info == {"pixels": pixels, "samples": samples}
        dev = fray.Accumulation(torch.from_numpy(rows).cuda(), int(cnt.min()), 42, (W, H), counts=None if uniform else torch.from_numpy(cnt).cuda())
        dadd, dinfo = fray.sample_map(dev, **params)
        assert same(dadd.cpu().numpy(), want) and dinfo == info
    assert len(np.unique(sample_map_ref(state, count, **params)[0])) >= 4


# ---- 7: refine ------------------------------------------------------------------------------------------------------------------------------------
def simulate_refine(S, shape, passes, **params):
    """Scene.refine from the snapshots alone: the counts after each pass of sample_map_ref."""
    counts = np.zeros(shape, np.int32)
    rows = np.zeros(shape + (4,), np.float32)
    done = 0
    for _ in range(passes):
        for n in np.unique(counts):
            if n > 0:
                rows[counts == n] = S[n][counts == n]
        add, pixels, _ = sample_map_ref(rows, counts, **params)
        if pixels == 0:
            break
        counts = counts + add
        done += 1
    return counts, done


def test_refine_reaches_the_simulated_counts(fray, gpu):
    s, S = cornell(fray, 64, 48, top=32)
    H, W = 48, 64
    # the tolerance at which a pixel of S_4 asks for exactly the samples it has: sqrt(noise) / max(lbar, floor); a quantile of it splits the frame
    rgb4, noise4 = mean_and_noise(S[4], 4)
    lbar = ((rgb4[..., 0] + rgb4[..., 1]) + rgb4[..., 2]) / np.float32(3)
    tau = np.sqrt(noise4) / np.maximum(lbar, np.float32(0.01))
    tau = tau[np.isfinite(tau) & (tau > 0)]
    for q in (0.5, 0.35, 0.65, 0.2, 0.8, 0.1, 0.9):
        params = dict(tolerance=float(np.quantile(tau, q)), min_count=4, max_count=32)
        want, passes = simulate_refine(S, (H, W), 8, **params)
        if len(np.unique(want)) >= 3:
            break
    else:
        pytest.fail("no quantile of the first pass's need leaves three distinct final counts")
    rgb, st, noise, info = s.refine(None, passes=8, **params)
    assert same(st.count_plane(), want), (np.unique(st.count_plane(), return_counts=True), np.unique(want, return_counts=True))
    rows, want_rgb, want_noise = expectation(S, want, np.zeros((H, W, 4), np.float32))
    assert same(st.state, rows) and same(rgb, want_rgb) and same(noise, want_noise)
    assert info["passes"] == passes and info["samples"] == int(want.sum())
    assert want.min() >= 4 and want.max() <= 32 and len(np.unique(want)) >= 3
    again, more = fray.sample_map(st, **params)
    assert more["pixels"] == 0 or info["passes"] == 8
    # the refined frame is what the denoiser takes: its own noise estimate as the variance
    feat = s.render_features(4)
    out = fray.denoise_signal(rgb, noise, feat, demodulate=0)
    assert out.shape == rgb.shape and np.isfinite(out).all()


def test_cli_refine_denoise_writes_a_finite_image(fray, gpu, tmp_path):
    sc = os.path.join(ROOT, "scenes", "cornell_box.fray")
    state, bmp, noise = (str(tmp_path / n) for n in ("state.npz", "refined.bmp", "noise.npy"))
    out = run_in_clean_child([sys.executable, "-m", "fray_amd", sc, "--width", "64", "--height", "48", "--refine", "0.1", "--max-spp", "32", "--denoise",
                              "--accumulate", state, "--noise-out", noise, "-o", bmp], str(tmp_path / "refine.log"), timeout=300)
    assert "[exit code 0]" in out, out[-2000:]
    st = fray.Accumulation.load(state)
    held = st.count_plane()
    assert held.min() >= 4 and held.max() <= 32 and np.isfinite(st.state).all()
    n = np.load(noise)
    assert n.shape == (48, 64) and np.isfinite(n).all() and (n >= 0).all()
    data = open(bmp, "rb").read()
    assert len(data) >= 54 + 64 * 48 * 3 and any(data[54:])
