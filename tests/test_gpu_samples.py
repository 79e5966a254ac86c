"""Resumable frames on a real MI355X (include/frayhip.h "resumable frames"): samples added to a frame that is already rendered.

Sample i of a pixel does not depend on the frame's spp and the state's FP32 sum runs in sample order, so however samples [0, N) are cut into calls
and batches the state is the same and state / N IS the N-sample frame: every comparison here is bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, bucket_xy, run_in_clean_child
from samples_ref import accumulate, mean_and_noise
from test_gpu_progressive import CASES, COUNTERS, Recorder, scene_for
from test_gpu_shade import AA_OFFSETS, jitter, pixel_grid, sample_seed
from test_oracle_vs_ref import load_case

pytestmark = pytest.mark.gpu

CHUNK = 2
# test_gpu_progressive's cases with the mono path tracer's shrunk (its frame there is 640 x 480 x 80: kept once below, where four lanes run)
SMALL = [("pt-mono", "cornell_box.fray", 96, 72, dict(numPaths=12, wantAA=0), CHUNK, "numPaths")] + [c for c in CASES if c[0] != "pt-mono-4lanes"]
MONO = SMALL[0]


def add_samples(s, cuts, N, state=None, **kw):
    """render_samples over [0, c_0), [c_0, c_1), ..., [c_last, N) into one state; (rgb of the last call, state)."""
    rgb = None
    for a, b in zip((0,) + tuple(cuts), tuple(cuts) + (N,)):
        out = s.render_samples(b - a, state, spp_chunk=CHUNK, **kw)
        rgb, state = out[0], out[1]
        assert state.samples_done == b
    return rgb, state


def splits_of(N):
    return [(), (2,)] if N == 5 else [(), (1, 2), (3, 5)]          # the five AA samples: one call, and 2 + 3


# ---- 1: splits equal the frame -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c[0])
def test_splits_equal_the_frame(fray, gpu, case):
    _, name, W, H, over, _, _ = case
    s = scene_for(fray, name, W, H, over)
    N = s.samples_per_pixel()
    frame, _ = s.render(spp_chunk=CHUNK)
    states = []
    for cuts in splits_of(N):
        rgb, st = add_samples(s, cuts, N)
        assert np.array_equal(rgb, frame), cuts
        assert np.array_equal(st.state[..., :3] / np.float32(N), frame), cuts
        states.append(st.state)
    for other in states[1:]:
        assert other.tobytes() == states[0].tobytes()
    if case is MONO:
        assert s.get_option("batch_lanes") > 1              # the last call's batches ran side by side
    s.close()


def test_four_lanes_equal_the_frame(fray, gpu):
    """A frame the planner gives four batch lanes (read from it below, not assumed): test_gpu_progressive's 640 x 480 x 80."""
    _, name, W, H, over, chunk, _ = CASES[0]
    s = scene_for(fray, name, W, H, over)
    N = s.samples_per_pixel()
    frame, _ = s.render(spp_chunk=chunk)
    assert s.get_option("batch_lanes") == 4
    rgb, one = s.render_samples(N, spp_chunk=chunk)
    assert s.get_option("batch_lanes") == 4
    assert np.array_equal(rgb, frame)
    two = None
    for count in (16, 64):
        rgb, two = s.render_samples(count, two, spp_chunk=chunk)
    assert s.get_option("batch_lanes") > 1
    assert np.array_equal(rgb, frame) and two.state.tobytes() == one.state.tobytes()
    s.close()


def test_contracted_splits_equal_the_contracted_frame(fray, gpu):
    _, name, W, H, over, _, _ = MONO
    s = scene_for(fray, name, W, H, over)
    s.set_option("fp_contract", 1)
    frame, _ = s.render(spp_chunk=CHUNK)
    assert s.get_option("contracted_launches") > 0
    rgb, st = add_samples(s, (3, 5), 12)
    assert s.get_option("contracted_launches") > 0
    assert np.array_equal(rgb, frame)
    rgb1, st1 = add_samples(s, (), 12)
    assert np.array_equal(rgb1, frame) and st1.state.tobytes() == st.state.tobytes()
    s.close()


def test_lanes_do_not_change_the_state(fray, gpu):
    _, name, W, H, over, _, _ = MONO
    s = scene_for(fray, name, W, H, over)
    s.set_option("pt_lanes", 1)
    _, one = add_samples(s, (3, 5), 12)
    assert s.get_option("batch_lanes") == 1
    s.set_option("pt_lanes", 4)
    _, four = add_samples(s, (3, 5), 12)
    assert s.get_option("batch_lanes") > 1
    assert one.state.tobytes() == four.state.tobytes()
    s.close()


# ---- 2: moments --------------------------------------------------------------------------------------------------------------------------------
def check_moments(s, colours):
    N = len(colours)
    want = accumulate(colours)
    want_rgb, want_noise = mean_and_noise(want, N)
    for cuts in ((), (1,), (N - 1,)):
        rgb, st, noise = None, None, None
        for a, b in zip((0,) + cuts, cuts + (N,)):
            rgb, st, noise = s.render_samples(b - a, st, spp_chunk=CHUNK, noise=True)
        assert st.state.tobytes() == want.tobytes(), cuts
        assert rgb.tobytes() == want_rgb.tobytes() and noise.tobytes() == want_noise.tobytes(), cuts
    # one sample: "as uncertain as the value"
    rgb, st, noise = s.render_samples(1, noise=True)
    r1, n1 = mean_and_noise(accumulate(colours[:1]), 1)
    assert rgb.tobytes() == r1.tobytes() and noise.tobytes() == n1.tobytes()
    return want_noise


def test_moments_of_a_path_traced_frame(fray, gpu):
    W, H, N = 32, 24, 6
    s = scene_for(fray, "cornell_box.fray", W, H, dict(gi=1, numPaths=N, wantAA=0))
    xs, ys = pixel_grid(W, H)
    p = np.arange(W * H, dtype=np.uint32)
    colours = np.empty((N, H, W, 3), np.float32)
    for k in range(N):          # test_gpu_shade.pt_by_samples' samples, kept apart
        j = jitter(fray, sample_seed(42, p, k)).reshape(H, W, 2)
        xy = np.stack([(xs + j[..., 0]).astype(np.float64), (ys + j[..., 1]).astype(np.float64)], axis=-1)
        o, d = s.camera_rays(xy)
        colours[k] = s.shade_rays(o, d, seed=42, sample_first=k, rng_skip=2)
    noise = check_moments(s, colours)
    assert (noise > 0).mean() > 0.5            # a path-traced frame of six samples is noisy nearly everywhere
    s.close()


def test_moments_of_a_whitted_aa_frame(fray, gpu):
    z, s = load_case(fray, os.path.join(ROOT, "tests", "golden", "ref_boxed_aa.npz"))
    assert s.settings.wantAA and not s.settings.gi and not s.camera.dof and not s.camera.stereoSeparation > 0
    s.beginRender()
    W, H = s.frame_size
    xs, ys = pixel_grid(W, H)
    colours = np.empty((5, H, W, 3), np.float32)
    for i, (ox, oy) in enumerate(AA_OFFSETS):
        xy = np.stack([(xs + np.float32(ox)).astype(np.float64), (ys + np.float32(oy)).astype(np.float64)], axis=-1)
        o, d = s.camera_rays(xy)
        colours[i] = s.shade_rays(o, d, seed=42, sample_first=i, keys=np.arange(W * H, dtype=np.uint32).reshape(H, W))
    check_moments(s, colours)
    s.close()


# ---- 3: cancel and resume ------------------------------------------------------------------------------------------------------------------------
def samples_call(fray, abi, s, first, count, accum, rgb=None, noise=None, progressive=None, bucket_first=0, bucket_stride=1, flags=0):
    """frayhip_render_samples itself: (return code, samples_done)."""
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=bucket_first, bucket_stride=bucket_stride, spp_chunk=CHUNK, flags=flags)
    req = abi.Samples(sample_first=first, sample_count=count)
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = fray.lib.frayhip_render_samples(s._dev, C.byref(fr), C.byref(req), C.byref(progressive) if progressive is not None else None, ptr(accum),
                                         ptr(rgb), ptr(noise), None)
    return rc, req.samples_done


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_cancel_and_resume(fray, abi, gpu, device):
    W, H, N = 96, 64, 12
    s = scene_for(fray, "cornell_box.fray", W, H, dict(numPaths=N, wantAA=0))
    frame, _ = s.render(spp_chunk=CHUNK)
    host = (lambda a: a.cpu().numpy()) if device else (lambda a: a)
    state = fray.Accumulation.empty((W, H), device="cuda") if device else None
    rec = Recorder(cancel_at=1)
    rgb, state, st = s.render_samples(N, state, spp_chunk=CHUNK, progress=rec)
    k = state.samples_done
    last = rec.check_sequence()
    assert st["cancelled"] and st["samples_done"] == k == last["samples_done"] and last["samples_total"] == N
    assert 0 < k < N and k % CHUNK == 0
    low = scene_for(fray, "cornell_box.fray", W, H, dict(numPaths=k, wantAA=0))
    low_frame, _ = low.render(spp_chunk=CHUNK)
    low.close()
    assert np.array_equal(host(rgb), low_frame)
    rec = Recorder()
    rgb, state, st = s.render_samples(N - k, state, spp_chunk=CHUNK, progress=rec, preview_ms=0)
    last = rec.check_sequence()
    assert not st["cancelled"] and state.samples_done == N == last["samples_done"] == last["samples_total"]
    assert rec.calls[0]["samples_done"] == k + CHUNK           # counted from sample 0
    assert np.array_equal(host(rgb), frame)
    if not device:
        assert np.array_equal(last["image"], frame)
        # the C entry's own answer
        calls = []

        def cb(_user, p):
            calls.append(p.contents.as_dict())
            return 1
        req = abi.Progressive(fn=abi.PROGRESS_FN(cb), user=None, preview_ms=-1.0)
        acc, out = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 3), np.float32)
        rc, done = samples_call(fray, abi, s, 0, N, acc, out, progressive=req)
        assert rc == abi.E_CANCELLED and b"frayhip_render_samples" in fray.lib.frayhip_last_error()
        assert done == k and calls[-1]["final"] == 1 and calls[-1]["samples_done"] == k
        assert np.array_equal(out, low_frame)
        rc, done = samples_call(fray, abi, s, k, N - k, acc, out)
        assert (rc, done) == (0, N) and np.array_equal(out, frame)
    s.close()


# ---- 4: shares -------------------------------------------------------------------------------------------------------------------------------------
def test_two_shares_make_the_whole_state(fray, abi, gpu):
    W, H, N = 96, 72, 4                     # 2 x 2 buckets, the right column ragged
    s = scene_for(fray, "cornell_box.fray", W, H, dict(numPaths=N, wantAA=0))
    _, whole, whole_noise = s.render_samples(N, spp_chunk=CHUNK, noise=True)
    frame, _ = s.render(spp_chunk=CHUNK)
    mine = np.zeros((H, W), bool)
    for b in (0, 2):
        bx, by = bucket_xy(W, b)
        mine[by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48] = True
    acc, rgb, noise = (np.full((H, W, c), -7.0, np.float32) for c in (4, 3, 1))
    assert samples_call(fray, abi, s, 0, 2, acc, rgb, noise, bucket_first=0, bucket_stride=2) == (0, 2)
    assert samples_call(fray, abi, s, 2, 2, acc, rgb, noise, bucket_first=0, bucket_stride=2) == (0, N)
    for a in (acc, rgb, noise):
        assert np.all(a[~mine] == -7.0)
    assert np.array_equal(acc[mine], whole.state[mine]) and np.array_equal(rgb[mine], frame[mine])
    assert samples_call(fray, abi, s, 0, N, acc, rgb, noise, bucket_first=1, bucket_stride=2) == (0, N)
    assert acc.tobytes() == whole.state.tobytes() and np.array_equal(rgb, frame) and np.array_equal(noise[..., 0], whole_noise)
    # and through Scene.render_samples: two states of two shares over one array
    arr = np.full((H, W, 4), -7.0, np.float32)
    for first in (0, 1):
        s.render_samples(N, fray.Accumulation(arr, 0, 42, (W, H), bucket_first=first, bucket_stride=2), bucket_first=first, bucket_stride=2, spp_chunk=CHUNK)
    assert arr.tobytes() == whole.state.tobytes()
    s.close()


# ---- 5: counters -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in SMALL if c[0] in ("pt-mono", "wavefront-dof-kd", "black")], ids=lambda c: c[0])
def test_counters_of_the_calls_add_up_to_the_frames(fray, gpu, case):
    _, name, W, H, over, _, field = case
    N = 6 if case[0] == "black" else 8
    s = scene_for(fray, name, W, H, dict(over, **{field or "numPaths": N}))
    assert s.samples_per_pixel() == N
    _, want = s.render(spp_chunk=CHUNK, stats=True)
    _, state, a = s.render_samples(N // 2, spp_chunk=CHUNK, stats=True)
    _, state, b = s.render_samples(N - N // 2, state, spp_chunk=CHUNK, stats=True)
    assert want["samples"] > 0
    for k in COUNTERS:
        assert a[k] + b[k] == want[k], k
    s.close()


# ---- 6: the seed table ---------------------------------------------------------------------------------------------------------------------------------
def test_seed_table_is_used_from_sample_0_and_left_alone_after(fray, gpu):
    s = scene_for(fray, "cornell_box.fray", 96, 64, dict(numPaths=8, wantAA=0))
    frame, _ = s.render(spp_chunk=CHUNK)
    assert s.get_option("seed_launches") > 0
    held = s.get_option("seed_table_bytes")
    assert held > 0
    rgb, state = s.render_samples(8, spp_chunk=CHUNK)
    assert s.get_option("seed_launches") == 0 and s.get_option("seed_planes_reused") == 8
    assert np.array_equal(rgb, frame)
    s.render_samples(4, state, spp_chunk=CHUNK)                 # [8, 12): seeds into the workspace
    assert s.get_option("seed_launches") > 0 and s.get_option("seed_planes_reused") == 0
    assert s.get_option("seed_table_bytes") == held
    again, _ = s.render(spp_chunk=CHUNK)
    assert s.get_option("seed_launches") == 0 and s.get_option("seed_table_bytes") == held
    assert np.array_equal(again, frame)
    s.close()


# ---- 7: refusals on a live scene -----------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_scene(fray, abi, gpu):
    import torch
    # a frame without jittered samples has only its five
    s = scene_for(fray, "boxed.fray", 64, 48, dict(wantAA=1))
    assert s.samples_per_pixel() == 5 and not s.settings.gi and not s.camera.dof
    frame, _ = s.render()
    rgb, state = s.render_samples(5)
    assert np.array_equal(rgb, frame)
    for args in ((1, state), (6, None)):
        with pytest.raises(fray.FrayError) as e:
            s.render_samples(*args)
        assert e.value.code == abi.E_ARG and "frayhip_render_samples" in str(e.value)
    assert state.samples_done == 5
    s.close()
    # from inside a progress callback; a misaligned device state
    s = scene_for(fray, "cornell_box.fray", 64, 48, dict(numPaths=8, wantAA=0))
    frame, _ = s.render(spp_chunk=CHUNK)
    codes = []

    def inside(info):
        if not info["final"]:
            with pytest.raises(fray.FrayError) as e:
                s.render_samples(2)
            codes.append((e.value.code, str(e.value)))
    rgb, state, st = s.render_samples(8, spp_chunk=CHUNK, progress=Recorder(inside=inside))
    assert codes and all(c == abi.E_ARG and "rendering" in m for c, m in codes)
    assert not st["cancelled"] and np.array_equal(rgb, frame)
    flat = torch.zeros(48 * 64 * 4 + 1, dtype=torch.float32, device="cuda")
    off = flat[1:].view(48, 64, 4)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(fray.FrayError) as e:
        s.render_samples(2, fray.Accumulation(off, 0, 42, (64, 48)))
    assert e.value.code == abi.E_ARG and "16-byte" in str(e.value)
    # overlapping outputs
    acc = np.zeros((48, 64, 4), np.float32)
    rc, _ = samples_call(fray, abi, s, 0, 2, acc, rgb=acc.reshape(-1)[4:4 + 48 * 64 * 3])          # a view that begins at the state's second row
    assert rc == abi.E_ARG and b"overlap" in fray.lib.frayhip_last_error()
    s.close()


# ---- 8: the existing entries are as they were -------------------------------------------------------------------------------------------------------------
def test_existing_entries_before_and_after(fray, gpu):
    s = scene_for(fray, "cornell_box.fray", 96, 64, dict(numPaths=8, wantAA=0))

    def pictures():
        a, _ = s.render(spp_chunk=CHUNK)
        rec = Recorder()
        b, st = s.render(spp_chunk=CHUNK, progress=rec, preview_ms=0)
        c, spp, err, _ = s.render_adaptive(0.05, min_spp=4, spp_chunk=CHUNK)
        return [a, b, c, spp, err] + [r["image"] for r in rec.calls if r["preview"]]
    before = pictures()
    _, state = s.render_samples(3, spp_chunk=CHUNK)
    s.render_samples(7, state, spp_chunk=CHUNK, progress=Recorder(cancel_at=1))
    after = pictures()
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
    s.close()


# ---- 9: the CLI ------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_two_runs_of_4_write_the_picture_of_8(fray, gpu, tmp_path):
    scene = os.path.join(ROOT, "scenes", "cornell_box.fray")
    base = [sys.executable, "-m", "fray_amd", scene, "--width", "64", "--height", "48"]
    state, acc_bmp, one_bmp, noise = (str(tmp_path / n) for n in ("state.npz", "acc.bmp", "one.bmp", "noise.npy"))
    for run in range(2):
        out = run_in_clean_child(base + ["--spp", "4", "--accumulate", state, "--noise-out", noise, "-o", acc_bmp], str(tmp_path / ("acc%d.log" % run)), timeout=300)
        assert "[exit code 0]" in out, out[-2000:]
        assert fray.Accumulation.load(state).samples_done == 4 * (run + 1)
    out = run_in_clean_child(base + ["--spp", "8", "-o", one_bmp], str(tmp_path / "one.log"), timeout=300)
    assert "[exit code 0]" in out, out[-2000:]
    assert open(acc_bmp, "rb").read() == open(one_bmp, "rb").read()
    n = np.load(noise)
    assert n.shape == (48, 64) and n.dtype == np.float32 and (n >= 0).all()
