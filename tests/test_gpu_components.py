"""Component frames on a real MI355X (include/frayhip.h "component frames"): direct and indirect light of a path-traced frame as two resumable
states.

A sample's direct light is its path's first term and its indirect light the fold of the others, so one FP32 addition of the two IS the sample's
colour in frayhip_render_samples, the direct mean IS the frame of the same scene with maxTraceDepth = 0, and both states are the numpy
restatement's (tests/components_ref.py over tests/samples_ref.py) however the samples are cut into calls, batches and lanes: every comparison here
is bit for bit but the one the fp_contract option bounds by RMS."""
import ctypes as C
import os

import numpy as np
import pytest

from components_ref import accumulate, mean_and_noise
from conftest import bucket_xy
from test_gpu_progressive import Recorder, scene_for

pytestmark = pytest.mark.gpu

CHUNK = 2
N = 12
MAIN = ("cornell_box.fray", 96, 72, dict(numPaths=N, wantAA=0))          # 2 x 2 buckets, the right column ragged; six batches of two samples
CSG = os.path.join("..", "tests", "scenes", "csg_nested.fray")


def pair(fray, W, H, done=0, device=None, **kw):
    """Two zero states that say they hold `done` samples."""
    states = (fray.Accumulation.empty((W, H), device=device, **kw), fray.Accumulation.empty((W, H), device=device, **kw))
    for a in states:
        a.samples_done = done
    return states


def per_sample(fray, s, n):
    """(d, n, c), each float32 [n, H, W, 3]: sample i alone, rendered into zero states that say they hold i samples -- by render_components and by
    render_samples.  A row is then 0 + the sample's value, which is the value (but for the sign of a zero)."""
    W, H = s.frame_size
    d, ind, c = (np.empty((n, H, W, 3), np.float32) for _ in range(3))
    for i in range(n):
        _, _, (sd, si) = s.render_components(1, pair(fray, W, H, i), spp_chunk=CHUNK)
        one = fray.Accumulation.empty((W, H))
        one.samples_done = i
        _, one = s.render_samples(1, one, spp_chunk=CHUNK)
        assert sd.samples_done == si.samples_done == one.samples_done == i + 1
        d[i], ind[i], c[i] = sd.state[..., :3], si.state[..., :3], one.state[..., :3]
    return d, ind, c


def add_components(s, cuts, n, state=None, **kw):
    """render_components over [0, c_0), [c_0, c_1), ..., [c_last, n) into one pair of states; the last call's result."""
    out = None
    for a, b in zip((0,) + tuple(cuts), tuple(cuts) + (n,)):
        out = s.render_components(b - a, state, spp_chunk=CHUNK, **kw)
        state = out[2]
        assert state[0].samples_done == state[1].samples_done == b
    return out


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def check_states(state, d, ind):
    assert host(state[0].state).tobytes() == accumulate(d).tobytes()
    assert host(state[1].state).tobytes() == accumulate(ind).tobytes()


@pytest.fixture(scope="module")
def main(fray, gpu):
    """The main case's samples one by one and its one-shot call, rendered once for the tests below (which leave them as they are)."""
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    d, ind, c = per_sample(fray, s, N)
    rgb_d, rgb_i, state, noise_d, noise_i = s.render_components(N, spp_chunk=CHUNK, noise=True)
    lanes = s.get_option("batch_lanes")
    s.close()
    out = dict(d=d, n=ind, c=c, rgb_d=rgb_d, rgb_i=rgb_i, state=(state[0].state, state[1].state), noise_d=noise_d, noise_i=noise_i, lanes=lanes)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


# ---- 1: per sample, direct + indirect is the sample -----------------------------------------------------------------------------------------------
def test_direct_plus_indirect_is_the_sample(main):
    assert main["lanes"] > 1                                    # the one-shot call's six batches ran side by side
    for i in range(N):
        assert main["c"][i].tobytes() == (main["d"][i] + main["n"][i]).tobytes(), i
    # guards: both components are there to be compared, nearly everywhere
    assert (main["rgb_d"].max(axis=2) > 0).mean() > 1 / 3
    assert (main["rgb_i"].max(axis=2) > 0).mean() > 1 / 3


# ---- 2: direct light is the frame of depth 0 ----------------------------------------------------------------------------------------------------
def test_direct_is_the_depth_0_frame(fray, abi, oracle, main):
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, dict(over, maxTraceDepth=0))
    frame, _ = s.render(spp_chunk=CHUNK)
    ref, _ = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
    s.close()
    # values, not bytes: the frame adds t[0] + 0 per sample, which loses a -0 that the direct state's t[0] keeps until it is summed
    assert np.array_equal(main["rgb_d"], frame)
    assert np.array_equal(main["rgb_d"], ref)
    assert frame.max() > 0


# ---- 3: the states are the restatement's -----------------------------------------------------------------------------------------------------------
def test_one_shot_states_and_outputs(main):
    sd, si = accumulate(main["d"]), accumulate(main["n"])
    assert main["state"][0].tobytes() == sd.tobytes() and main["state"][1].tobytes() == si.tobytes()
    for state, rgb, noise in ((sd, main["rgb_d"], main["noise_d"]), (si, main["rgb_i"], main["noise_i"])):
        want_rgb, want_noise = mean_and_noise(state, N)
        assert rgb.tobytes() == want_rgb.tobytes() and noise.tobytes() == want_noise.tobytes()


@pytest.mark.parametrize("cuts", [(1, 2), (3, 5)])
def test_cuts_do_not_change_the_states(fray, gpu, main, cuts):
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    rgb_d, rgb_i, state, noise_d, noise_i = add_components(s, cuts, N, noise=True)
    s.close()
    check_states(state, main["d"], main["n"])
    for got, key in ((rgb_d, "rgb_d"), (rgb_i, "rgb_i"), (noise_d, "noise_d"), (noise_i, "noise_i")):
        assert got.tobytes() == main[key].tobytes(), key


def test_lanes_do_not_change_the_states(fray, gpu, main):
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    for lanes in (1, 4):
        s.set_option("pt_lanes", lanes)
        _, _, state = add_components(s, (3, 5), N)
        assert (s.get_option("batch_lanes") == 1) if lanes == 1 else (s.get_option("batch_lanes") > 1)
        check_states(state, main["d"], main["n"])
    s.close()


def test_states_on_the_gpu_equal_the_numpy_states(fray, gpu, main):
    import torch
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    side = torch.cuda.Stream()
    out = add_components(s, (3,), N, pair(fray, W, H, device="cuda"), noise=True, stream=side)
    s.close()
    assert all(torch.is_tensor(v) and v.is_cuda for v in out[:2] + out[3:]) and out[2][0].on_device and out[2][1].on_device
    check_states(out[2], main["d"], main["n"])
    for got, key in zip(out[:2] + out[3:], ("rgb_d", "rgb_i", "noise_d", "noise_i")):
        assert host(got).tobytes() == main[key].tobytes(), key


# ---- 4: term lists longer than eight, and long generators ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [12, 22])
def test_long_term_lists(fray, gpu, depth):
    W, H, n = 48, 48, 4
    s = scene_for(fray, "cornell_box.fray", W, H, dict(numPaths=n, wantAA=0, maxTraceDepth=depth))
    d, ind, c = per_sample(fray, s, n)
    for i in range(n):
        assert c[i].tobytes() == (d[i] + ind[i]).tobytes(), i
    for cuts in ((), (1, 2)):
        rgb_d, rgb_i, state, noise_d, noise_i = add_components(s, cuts, n, noise=True)
        check_states(state, d, ind)
        for st, rgb, noise in ((state[0].state, rgb_d, noise_d), (state[1].state, rgb_i, noise_i)):
            want_rgb, want_noise = mean_and_noise(st, n)
            assert rgb.tobytes() == want_rgb.tobytes() and noise.tobytes() == want_noise.tobytes()
    # the same samples seen through fewer bounces are another picture: the deep terms are there and are folded
    shallow = scene_for(fray, "cornell_box.fray", W, H, dict(numPaths=n, wantAA=0, maxTraceDepth=6))
    _, ind6, _ = shallow.render_components(n, spp_chunk=CHUNK)
    shallow.close()
    s.close()
    assert not np.array_equal(ind6, rgb_i)
    assert (rgb_d.max(axis=2) > 0).mean() > 1 / 3 and (rgb_i.max(axis=2) > 0).mean() > 1 / 3


def test_mirror_and_glass_first_hits_have_no_direct_light(fray, gpu):
    s = scene_for(fray, "smallpt.fray", 64, 48, dict(gi=1, numPaths=4, wantAA=0))
    rgb_d, rgb_i, _ = s.render_components(4, spp_chunk=CHUNK)
    s.close()
    dark = (rgb_d == 0).all(axis=2) & (rgb_i > 0).any(axis=2)
    assert dark.any()
    assert (rgb_d > 0).any()


# ---- 5: options that move where a term is written --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", ["certified_segments", "segment_planes", "skip_null_segments"])
def test_segment_options_do_not_change_the_states(fray, gpu, main, option):
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    assert s.get_option(option) != 0
    s.set_option(option, 0)
    _, _, state = s.render_components(N, spp_chunk=CHUNK)
    assert s.get_option(option) == 0
    s.close()
    assert state[0].state.tobytes() == main["state"][0].tobytes() and state[1].state.tobytes() == main["state"][1].tobytes()


# ---- 6: contracted arithmetic ----------------------------------------------------------------------------------------------------------------------
def test_contracted_frames_keep_the_direct_state(fray, gpu, main):
    """Measured on an MI355X: see the figures printed below (the direct state's differing rows, the indirect mean's RMS per channel)."""
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    s.set_option("fp_contract", 1)
    rgb_d, rgb_i, state = s.render_components(N, spp_chunk=CHUNK)
    launches = s.get_option("contracted_launches")
    s.close()
    differ = int((state[0].state != main["state"][0]).any(axis=2).sum())
    rms = np.sqrt(((rgb_i.astype(np.float64) - main["rgb_i"]) ** 2).mean(axis=(0, 1)))
    print("fp_contract: %d contracted launches, %d of %d direct rows differ, indirect RMS per channel %s" % (launches, differ, W * H, rms))
    assert launches > 0
    assert state[0].state.tobytes() == main["state"][0].tobytes()
    assert np.all(rms <= 1e-4), rms                               # the option's stated bound


# ---- 7: other kernel families feeding the same resolve ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["boxed.fray", CSG], ids=["kd", "csg"])
def test_kd_and_csg_scenes(fray, gpu, name):
    n = 4
    s = scene_for(fray, name, 64, 48, dict(gi=1, numPaths=n, wantAA=0))
    d, ind, c = per_sample(fray, s, n)
    s.close()
    for i in range(n):
        assert c[i].tobytes() == (d[i] + ind[i]).tobytes(), i
    assert (c > 0).any()


# ---- 8: shares -------------------------------------------------------------------------------------------------------------------------------------
def components_call(fray, abi, s, first, count, bufs, progressive=None, bucket_first=0, bucket_stride=1):
    """frayhip_render_components itself; bufs: accum_direct, accum_indirect, rgb_direct, rgb_indirect, noise_direct, noise_indirect (numpy or
    None).  (return code, samples_done)."""
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=bucket_first, bucket_stride=bucket_stride, spp_chunk=CHUNK)
    req = abi.Samples(sample_first=first, sample_count=count)
    ptrs = [a.ctypes.data if a is not None else None for a in bufs]
    rc = fray.lib.frayhip_render_components(s._dev, C.byref(fr), C.byref(req), C.byref(progressive) if progressive is not None else None, *ptrs, None)
    return rc, req.samples_done


def test_two_shares_make_the_whole_states(fray, abi, gpu, main):
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    mine = np.zeros((H, W), bool)
    for b in (0, 2):
        bx, by = bucket_xy(W, b)
        mine[by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48] = True
    assert mine.any() and not mine.all()
    bufs = [np.full((H, W, c), -7.0, np.float32) for c in (4, 4, 3, 3, 1, 1)]
    assert components_call(fray, abi, s, 0, 5, bufs, bucket_first=0, bucket_stride=2) == (0, 5)
    assert components_call(fray, abi, s, 5, N - 5, bufs, bucket_first=0, bucket_stride=2) == (0, N)
    want = [main["state"][0], main["state"][1], main["rgb_d"], main["rgb_i"], main["noise_d"][..., None], main["noise_i"][..., None]]
    for got, whole in zip(bufs, want):
        assert np.all(got[~mine] == -7.0)                       # pixels outside the share keep the sentinel in all six buffers
        assert got[mine].tobytes() == whole[mine].tobytes()
    assert components_call(fray, abi, s, 0, N, bufs, bucket_first=1, bucket_stride=2) == (0, N)
    for got, whole in zip(bufs, want):
        assert got.tobytes() == np.ascontiguousarray(whole).tobytes()
    s.close()


# ---- 9: the black frame, and refusals on a live scene ------------------------------------------------------------------------------------------------
def test_black_frame_counts_its_samples_once(fray, gpu):
    W, H, n = 61, 47, 3
    s = scene_for(fray, "cornell_box.fray", W, H, dict(numPaths=n, wantAA=0, maxTraceDepth=-1))
    _, want = s.render(stats=True)
    state = tuple(fray.Accumulation(np.full((H, W, 4), 3.0, np.float32), 0, 42, (W, H)) for _ in range(2))          # ignored: the call begins at sample 0
    rgb_d, rgb_i, state, noise_d, noise_i, st = s.render_components(n, state, noise=True, stats=True)
    s.close()
    for a in (state[0].state, state[1].state, rgb_d, rgb_i, noise_d, noise_i):
        assert a.tobytes() == np.zeros_like(a).tobytes()
    assert st["samples"] == want["samples"] == W * H * n


def test_refusals_on_a_live_scene(fray, abi, gpu):
    W, H = 64, 48
    for over, device, entry in ((dict(gi=0, wantAA=0), None, "frayhip_render_components:"),
                                (dict(numPaths=4, wantAA=0, stereoSeparation=12.0), None, "frayhip_render_components:"),
                                (dict(gi=0, wantAA=0), "cuda", "frayhip_render_components_device:")):
        s = scene_for(fray, "cornell_box.fray", W, H, over)
        state = pair(fray, W, H, device=device)
        with pytest.raises(fray.FrayError) as e:
            s.render_components(2, state)
        assert e.value.code == abi.E_UNSUPPORTED and entry in str(e.value), str(e.value)
        assert state[0].samples_done == state[1].samples_done == 0
        s.close()
    s = scene_for(fray, "cornell_box.fray", W, H, dict(numPaths=4, wantAA=0))
    bufs = [np.zeros((H, W, c), np.float32) for c in (4, 4, 3, 3, 1, 1)]
    for ms in (0.0, 5.0):
        rc, _ = components_call(fray, abi, s, 0, 2, bufs, progressive=abi.Progressive(preview_ms=ms))
        assert rc == abi.E_ARG and fray.lib.frayhip_last_error().startswith(b"frayhip_render_components: previews are not offered")
    # ranges that intersect without beginning at one address: a view into the indirect state's second row as rgb_direct
    inside = bufs[1].reshape(-1)[4:4 + H * W * 3]
    rc, _ = components_call(fray, abi, s, 0, 2, bufs[:2] + [inside] + bufs[3:])
    assert rc == abi.E_ARG and b"rgb_direct must not overlap accum_indirect" in fray.lib.frayhip_last_error()
    rc, _ = components_call(fray, abi, s, 0, 2, bufs[:5] + [bufs[0].reshape(-1)[8:8 + H * W]])
    assert rc == abi.E_ARG and b"noise_indirect must not overlap accum_direct" in fray.lib.frayhip_last_error()
    # a numpy state beside one on the GPU
    with pytest.raises(ValueError, match="numpy"):
        s.render_components(2, (fray.Accumulation.empty((W, H)), fray.Accumulation.empty((W, H), device="cuda")))
    # and the call that is refused nothing
    assert components_call(fray, abi, s, 0, 2, bufs, progressive=abi.Progressive(preview_ms=-1.0)) == (0, 2)
    s.close()


# ---- 10: cancel and resume ---------------------------------------------------------------------------------------------------------------------------
def test_cancel_and_resume(fray, abi, gpu, main):
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    rec = Recorder(cancel_at=1)
    rgb_d, rgb_i, state, st = s.render_components(N, spp_chunk=CHUNK, progress=rec)
    last = rec.check_sequence()
    k = state[0].samples_done
    assert st["cancelled"] and st["samples_done"] == k == state[1].samples_done == last["samples_done"] and last["samples_total"] == N
    assert 0 < k < N and k % CHUNK == 0
    assert all(not c["preview"] and "image" not in c for c in rec.calls)          # no previews
    check_states(state, main["d"][:k], main["n"][:k])
    assert rgb_d.tobytes() == mean_and_noise(state[0].state, k)[0].tobytes() and rgb_i.tobytes() == mean_and_noise(state[1].state, k)[0].tobytes()
    rec = Recorder()
    rgb_d, rgb_i, state, st = s.render_components(N - k, state, spp_chunk=CHUNK, progress=rec)
    last = rec.check_sequence()
    assert not st["cancelled"] and state[0].samples_done == state[1].samples_done == N == last["samples_done"] == last["samples_total"]
    assert rec.calls[0]["samples_done"] == k + CHUNK           # counted from sample 0
    assert state[0].state.tobytes() == main["state"][0].tobytes() and state[1].state.tobytes() == main["state"][1].tobytes()
    assert rgb_d.tobytes() == main["rgb_d"].tobytes() and rgb_i.tobytes() == main["rgb_i"].tobytes()
    # the C entry's own answer
    calls = []

    def cb(_user, p):
        calls.append(p.contents.as_dict())
        return 1
    bufs = [np.zeros((H, W, c), np.float32) for c in (4, 4, 3, 3, 1, 1)]
    rc, done = components_call(fray, abi, s, 0, N, bufs, progressive=abi.Progressive(fn=abi.PROGRESS_FN(cb), user=None, preview_ms=-1.0))
    assert rc == abi.E_CANCELLED and fray.lib.frayhip_last_error().startswith(b"frayhip_render_components:")
    assert done == k and calls[-1]["final"] == 1 and calls[-1]["samples_done"] == k and not any(c["preview"] for c in calls)
    assert bufs[0].tobytes() == accumulate(main["d"][:k]).tobytes() and bufs[1].tobytes() == accumulate(main["n"][:k]).tobytes()
    s.close()


# ---- 11: the split filter ----------------------------------------------------------------------------------------------------------------------------
def test_render_denoised_split(fray, gpu, main):
    name, W, H, over = MAIN
    s = scene_for(fray, name, W, H, over)
    out, raw, info = s.render_denoised_split(seed=42, feature_samples=4, sigma_luminance=3.0)
    with pytest.raises(ValueError, match="demodulate"):
        s.render_denoised_split(demodulate=1)
    s.close()
    # its inputs are the components of the frame's samples, whatever batches the call chose
    for key, want in (("direct_rgb", "rgb_d"), ("indirect_rgb", "rgb_i"), ("noise_direct", "noise_d"), ("noise_indirect", "noise_i")):
        assert info[key].tobytes() == main[want].tobytes(), key
    assert raw.tobytes() == (main["rgb_d"] + main["rgb_i"]).tobytes()
    feat = info["features_frame"]
    direct = fray.denoise_signal(info["direct_rgb"], info["noise_direct"], feat, demodulate=0, sigma_luminance=3.0)
    indirect = fray.denoise_signal(info["indirect_rgb"], info["noise_indirect"], feat, demodulate=0, sigma_luminance=3.0)
    assert info["direct"].tobytes() == direct.tobytes() and info["indirect"].tobytes() == indirect.tobytes()
    assert out.tobytes() == (direct + indirect).tobytes()
    assert out.dtype == np.float32 and out.shape == (H, W, 3)
    for a in (out, raw, direct, indirect):
        assert np.all(np.isfinite(a))
    assert not np.array_equal(out, raw)                         # the filter did something
