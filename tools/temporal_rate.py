"""Temporal accumulation on one GPU (include/frayhip.h "temporal accumulation"): its cost at 1080p beside the a-trous filter measured in the same
run.  Times are the library's own (frayhip_stats.ms_kernels: HIP events around the call's device work; ms_total: the call's wall time), medians
over --rounds rounds after --warmup, every call on one torch stream with all buffers resident on the device.  Inputs: cornell_box at
1920x1080, 4 spp, a chain of --frames views whose yaw turns by --yaw-step degrees, seeds 42, 43, ...

  accumulate_first            frayhip_temporal_accumulate_device without history (k_tp_accumulate + k_tp_variance on every pixel)
  accumulate_frame1           frame 1 onto frame 0's history: every pixel has N <= 2, so k_tp_variance takes its 7x7 window everywhere
  accumulate_frame1_novar     the same with variance_history 1: k_tp_accumulate alone (the difference is k_tp_variance at full work)
  accumulate_steady           the last frame of the chain onto the history before it: k_tp_variance works only where history was lost
  accumulate_steady_novar     the same with variance_history 1
  denoise_L<levels>_half      frayhip_denoise_device on frame 1 with its half-spp frame (the yardstick: one level = (L5 - L3) / 2)
  denoise_signal_L5           frayhip_denoise_signal_device on the steady frame's signal and variance
  bytes                       per pixel from the shapes, and the share of --copy-rate (TB/s) each kernel's time amounts to

    python tools/temporal_rate.py [--rounds 7] [--warmup 2] [--frames 6] [--yaw-step 1] [--copy-rate 6.3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
# bytes per pixel from the shapes: k_tp_accumulate reads rgb 12 + feat 40 and four taps of 48 (mostly the neighbours' cache lines: counted
# once), writes the history 48, the signal 12 and the variance 4; k_tp_variance reads 49 taps of 32 (each texel counted once: 32) plus its
# own N and depth and writes the variance 4; a filter level reads guides, gradient and signal 56 and writes 16
BYTES = {"k_tp_accumulate": 12 + 40 + 48 + 48 + 12 + 4, "k_tp_variance": 32 + 16 + 4 + 4, "k_dn_level": 16 + 16 + 8 + 16 + 16}


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--yaw-step", type=float, default=1.0)
    ap.add_argument("--copy-rate", type=float, default=6.3, help="TB/s of a device copy, for the shares")
    ap.add_argument("--out")
    a = ap.parse_args()
    import ctypes as C
    import torch
    import fray_amd
    from fray_amd import abi
    from conftest import open_scene

    L = fray_amd.lib
    L.frayhip_init(0)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    res = {}

    s = open_scene(fray_amd, "cornell_box.fray", W, H, wantAA=0, numPaths=4)
    s.beginRender()
    base = abi.Camera.from_buffer_copy(s.camera)
    frames = []
    with torch.cuda.stream(stream):
        for k in range(a.frames):
            cam = abi.Camera.from_buffer_copy(base)
            cam.yaw += k * a.yaw_step
            C.memmove(C.byref(s.desc.camera), C.byref(cam), C.sizeof(cam))
            s.beginFrame()
            rgb, feat = new(H, W, 3), new(H, W, 10)
            fr = abi.Frame(mode=abi.MODE_RENDER, seed=42 + k)
            s.render_device(rgb.data_ptr(), seed=42 + k, stream=h)
            assert L.frayhip_render_features_device(s._dev, C.byref(fr), 4, feat.data_ptr(), h, None) == 0, L.frayhip_last_error()
            frames.append((rgb, feat, fray_amd.view_from_camera(cam, W, H)))
        # frame 1's half-spp frame, the filter's noise estimate
        s.settings.numPaths = 2
        half = new(H, W, 3)
        cam = abi.Camera.from_buffer_copy(base)
        cam.yaw += a.yaw_step
        C.memmove(C.byref(s.desc.camera), C.byref(cam), C.sizeof(cam))
        s.beginFrame()
        s.render_device(half.data_ptr(), seed=43, stream=h)
        hist_out, signal, variance, out = new(H, W, 12), new(H, W, 3), new(H, W), new(H, W, 3)
    s.close()
    torch.cuda.synchronize()

    def accumulate(k, hist_in, dst, **params):
        rgb, feat, _ = frames[k]
        p = fray_amd.temporal_params(**params)
        st = abi.Stats()
        view = C.byref(frames[k - 1][2]) if hist_in is not None else None
        rc = L.frayhip_temporal_accumulate_device(W, H, rgb.data_ptr(), feat.data_ptr(), view, hist_in.data_ptr() if hist_in is not None else None,
                                                  C.byref(p), dst.data_ptr(), signal.data_ptr(), variance.data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st

    def timed(call):
        ks, calls = [], []
        for r in range(a.warmup + a.rounds):
            st = call()
            if r >= a.warmup:
                ks.append(st.ms_kernels)
                calls.append(st.ms_total)
        return {"kernels_ms": med(ks), "call_ms": med(calls)}

    # the chain up to the last frame's input history
    with torch.cuda.stream(stream):
        hists = [new(H, W, 12)]
    accumulate(0, None, hists[0])
    shares = [0.0]
    for k in range(1, a.frames - 1):
        with torch.cuda.stream(stream):
            hists.append(new(H, W, 12))
        accumulate(k, hists[k - 1], hists[k])
        hit = (hists[k][..., 8:11] != 0).any(dim=2)
        shares.append(float((hists[k][..., 3][hit] > 1).float().mean()))
    last = a.frames - 1
    res["accumulate_first"] = timed(lambda: accumulate(0, None, hist_out))
    res["accumulate_frame1"] = timed(lambda: accumulate(1, hists[0], hist_out))
    res["accumulate_frame1_novar"] = timed(lambda: accumulate(1, hists[0], hist_out, variance_history=1))
    res["accumulate_steady"] = timed(lambda: accumulate(last, hists[last - 1], hist_out))
    young = float((hist_out[..., 3] < 4).float().mean())
    res["accumulate_steady"]["share_on_spatial_variance"] = young
    res["accumulate_steady_novar"] = timed(lambda: accumulate(last, hists[last - 1], hist_out, variance_history=1))
    res["history_found_per_frame"] = shares

    rgb1, feat1, _ = frames[1]
    for levels in (3, 5):
        p = fray_amd.denoise_params(levels=levels)

        def filt():
            st = abi.Stats()
            rc = L.frayhip_denoise_device(W, H, rgb1.data_ptr(), half.data_ptr(), feat1.data_ptr(), C.byref(p), out.data_ptr(), h, C.byref(st))
            assert rc == 0, L.frayhip_last_error()
            return st
        res["denoise_L%d_half" % levels] = timed(filt)
    accumulate(last, hists[last - 1], hist_out)
    p5 = fray_amd.denoise_params(levels=5)

    def filt_signal():
        st = abi.Stats()
        rc = L.frayhip_denoise_signal_device(W, H, signal.data_ptr(), variance.data_ptr(), frames[last][1].data_ptr(), C.byref(p5), out.data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st
    res["denoise_signal_L5"] = timed(filt_signal)

    level_ms = (res["denoise_L5_half"]["kernels_ms"] - res["denoise_L3_half"]["kernels_ms"]) / 2
    k_acc = res["accumulate_frame1_novar"]["kernels_ms"]
    k_var = res["accumulate_frame1"]["kernels_ms"] - k_acc
    k_var_steady = res["accumulate_steady"]["kernels_ms"] - res["accumulate_steady_novar"]["kernels_ms"]
    n = W * H

    def share(name, ms):
        return BYTES[name] * n / (ms * 1e-3) / (a.copy_rate * 1e12) if ms > 0 else None
    res["kernels"] = {
        "k_dn_level_ms": level_ms, "k_dn_level_bytes_per_pixel": BYTES["k_dn_level"], "k_dn_level_share_of_copy_rate": share("k_dn_level", level_ms),
        "k_tp_accumulate_ms": k_acc, "k_tp_accumulate_bytes_per_pixel": BYTES["k_tp_accumulate"],
        "k_tp_accumulate_share_of_copy_rate": share("k_tp_accumulate", k_acc),
        "k_tp_variance_full_ms": k_var, "k_tp_variance_bytes_per_pixel": BYTES["k_tp_variance"],
        "k_tp_variance_share_of_copy_rate": share("k_tp_variance", k_var), "k_tp_variance_steady_ms": k_var_steady,
        "stage_over_level_frame1": res["accumulate_frame1"]["kernels_ms"] / level_ms,
        "stage_over_level_steady": res["accumulate_steady"]["kernels_ms"] / level_ms}

    for k, v in res.items():
        print(k, json.dumps(v), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
