"""Weighted accumulation and history maps on one GPU (include/frayhip.h "weighted accumulation and history maps").  Two measurements; the results
live in profiles/history_map/README.md.

Times (the default): cornell_box at 1920x1080, 4 spp, a chain of --frames views whose yaw turns by --yaw-step degrees, seeds 42, 43, ...; every
call on one torch stream with all buffers resident on the device; the library's own timings (frayhip_stats.ms_kernels: HIP events around the
call's device work; ms_total: the call's wall time), medians over --rounds rounds after --warmup, the calls alternating round after round
and the two kernels of each map pair swapping places every round.

  accumulate_plain            frayhip_temporal_accumulate_device, the last frame of the chain onto the history before it: unchanged code, the yardstick
  accumulate_weighted         frayhip_temporal_accumulate_weighted_device on the same inputs, weight 1 and units = N (the outputs are the plain
                              entry's bit for bit; the tool checks it)
  map_settled, map_settled_aggregated         frayhip_history_map_device on that history with units = N of a settled sequence (most pixels
                              that find history in one bin), as the library runs it (one LDS atomic a pixel) and with the per-wave
                              aggregation of equal k (FRAYHIP_HISTORY_MAP_AGGREGATE=1)
  map_random, map_random_aggregated           the same with units uniform in [0, 2 max_history]
The three kernels of a map call (k_hm_held, k_hm_select, k_hm_map) are told apart by `rocprofv3 --kernel-trace --stats -- python
tools/history_map_rate.py --trace`, a run of its own: --trace makes a few calls of each kind and times nothing.

The point of the feature (--quality): an 8-frame yaw sequence of cornell_box at --size, rendered twice with the same sample budget per frame --
(a) uniform spp = S, (b) spp = S / 2 with boost and budget = S * W * H -- each compared with a --ref-spp render of the last frame's view: RMS
error of the last frame's denoised picture and of its accumulated signal (albedo multiplied back), over the pixels whose history (a) is
shorter than 4 frames and over the rest; the samples (b) really spent per frame beside (a)'s.  A recorded result, whatever it shows.

    python tools/history_map_rate.py [--rounds 10] [--warmup 2] [--frames 6] [--yaw-step 1] [--trace] [--out FILE]
    python tools/history_map_rate.py --quality [--size 480 360] [--spp 8] [--yaw-step 2] [--ref-spp 1024] [--target 8] [--max-units 8] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
SWITCH = "FRAYHIP_HISTORY_MAP_AGGREGATE"


def times(a):
    import torch
    import fray_amd
    from fray_amd import abi
    from conftest import open_scene

    L = fray_amd.lib
    L.frayhip_init(0)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
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
    s.close()
    torch.cuda.synchronize()
    hist = None
    for k in range(a.frames - 1):
        hist = fray_amd.temporal_accumulate(frames[k][0], frames[k][1], frames[k - 1][2] if k else None, hist, stream=stream)[0]
    rgb, feat, _ = frames[-1]
    view = frames[-2][2]
    p = fray_amd.temporal_params()
    gen = torch.Generator(device="cpu").manual_seed(7)
    with torch.cuda.stream(stream):
        settled = hist[..., 3].contiguous()
        random = (torch.rand((H, W), generator=gen) * (2.0 * p.max_history)).cuda()
        ones = torch.ones((H, W), dtype=torch.float32, device="cuda")
        out = [new(H, W, 12), new(H, W, 3), new(H, W)]
        outw = [new(H, W, 12), new(H, W), new(H, W, 3), new(H, W)]
        add = torch.empty((H, W), dtype=torch.int32, device="cuda")
        weight = new(H, W)
    torch.cuda.synchronize()
    seen = {}

    def plain():
        st = abi.Stats()
        rc = L.frayhip_temporal_accumulate_device(W, H, rgb.data_ptr(), feat.data_ptr(), C.byref(view), hist.data_ptr(), C.byref(p), out[0].data_ptr(),
                                                  out[1].data_ptr(), out[2].data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st

    def weighted():
        st = abi.Stats()
        rc = L.frayhip_temporal_accumulate_weighted_device(W, H, rgb.data_ptr(), feat.data_ptr(), None, None, ones.data_ptr(), C.byref(view), hist.data_ptr(),
                                                           settled.data_ptr(), C.byref(p), outw[0].data_ptr(), outw[1].data_ptr(), outw[2].data_ptr(),
                                                           outw[3].data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st

    def mapped(name, units, aggregate):
        def run():
            if aggregate:
                os.environ[SWITCH] = "1"
            else:
                os.environ.pop(SWITCH, None)
            m, st = abi.HistoryMap(), abi.Stats()
            L.frayhip_history_map_defaults(C.byref(m))
            m.base = 4
            rc = L.frayhip_history_map_device(W, H, feat.data_ptr(), None, None, C.byref(view), hist.data_ptr(), units.data_ptr(), C.byref(p), C.byref(m),
                                              add.data_ptr(), weight.data_ptr(), None, h, C.byref(st))
            os.environ.pop(SWITCH, None)
            assert rc == 0, L.frayhip_last_error()
            got = {"target_used": int(m.target_used), "samples": int(m.samples), "boosted": int(m.boosted)}
            twin = name.replace("_aggregated", "")
            assert seen.setdefault(twin, got) == got, (name, got, seen[twin])         # the same answer with and without the aggregation
            return st
        return run

    calls = [("accumulate_plain", plain), ("accumulate_weighted", weighted), ("map_settled", mapped("map_settled", settled, False)),
             ("map_settled_aggregated", mapped("map_settled_aggregated", settled, True)), ("map_random", mapped("map_random", random, False)),
             ("map_random_aggregated", mapped("map_random_aggregated", random, True))]
    # the two kernels of a pair swap places every round: whichever map call comes first after the accumulations measured about 4 % slower,
    # which is as much as the two ever differed
    swapped = calls[:2] + [calls[3], calls[2], calls[5], calls[4]]
    if a.trace:
        for r in range(4):
            for _, fn in (swapped if r % 2 else calls):
                fn()
        print("made 4 calls of each kind; nothing timed")
        return None
    ts = {k: [] for k, _ in calls}
    for r in range(a.warmup + a.rounds):
        for k, fn in (swapped if r % 2 else calls):
            st = fn()
            if r >= a.warmup:
                ts[k].append((st.ms_kernels, st.ms_total))
    same = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in ((out[0], outw[0]), (out[1], outw[2]), (out[2], outw[3]),
                                                                                     (outw[1], outw[0][..., 3].contiguous())))
    res = {k: {"kernels_ms": statistics.median(x[0] for x in v), "kernels_ms_min_max": [min(x[0] for x in v), max(x[0] for x in v)],
               "call_ms": statistics.median(x[1] for x in v)} for k, v in ts.items()}
    res["weighted_equals_plain_bit_for_bit"] = same
    res["maps"] = seen
    k = torch.floor(torch.clamp(settled, max=float(p.max_history))).to(torch.int64).flatten()
    res["settled_bins"] = {str(int(b)): int(c) for b, c in zip(*torch.unique(k, return_counts=True))}
    ms = lambda name: res[name]["kernels_ms"]
    res["ratios"] = {"weighted_over_plain": ms("accumulate_weighted") / ms("accumulate_plain"),
                     "settled_aggregated_over_plain_atomics": ms("map_settled_aggregated") / ms("map_settled"),
                     "random_aggregated_over_plain_atomics": ms("map_random_aggregated") / ms("map_random"),
                     "map_settled_over_accumulate_plain": ms("map_settled") / ms("accumulate_plain")}
    for name, _ in calls:
        print("%-28s kernels %7.3f ms (%.3f .. %.3f)  call %7.3f ms" % ((name, ms(name)) + tuple(res[name]["kernels_ms_min_max"]) + (res[name]["call_ms"],)),
              flush=True)
    assert same, "the weighted entry with weight 1 and units = N differs from the plain entry"
    return res


def quality(a):
    import numpy as np
    import fray_amd
    from fray_amd import abi
    from conftest import open_scene

    Wq, Hq = a.size
    S, frames = a.spp, 8
    if S % 2:
        sys.exit("--spp must be even: (b) renders spp / 2")
    s = open_scene(fray_amd, "cornell_box.fray", Wq, Hq, numPaths=a.ref_spp)
    s.beginRender()
    start = abi.Camera.from_buffer_copy(s.camera)
    cams = []
    for k in range(frames):
        c = abi.Camera.from_buffer_copy(start)
        c.yaw += a.yaw_step * k
        cams.append(c)
    C.memmove(C.byref(s.desc.camera), C.byref(cams[-1]), C.sizeof(cams[-1]))
    s.beginFrame()
    ref = s.render(seed=4242)[0].astype(np.float64)
    C.memmove(C.byref(s.desc.camera), C.byref(start), C.sizeof(start))

    def run(spp, boost):
        s.settings.numPaths = spp
        s.beginFrame()
        spent = []
        for out, raw, info in s.render_sequence(cams, seed=42, feature_samples=4, boost=boost):
            spent.append(int(info["boost"]["samples"]) if boost else Wq * Hq * spp)
        acc = (info["signal"] * info["features_frame"][..., 6:9].clamp(min=1e-3)).cpu().numpy()
        extra = {"target_used": info["boost"]["target_used"], "boosted": info["boost"]["boosted"]} if boost else {}
        return out.cpu().numpy(), acc, info["history"][..., 3].cpu().numpy(), spent, extra

    budget = S * Wq * Hq
    u_out, u_acc, u_N, u_spent, _ = run(S, None)
    b_out, b_acc, b_N, b_spent, b_last = run(S // 2, dict(target=a.target, max_units=a.max_units, budget=budget))
    s.close()
    young = u_N < 4
    rms = lambda x, m: float(np.sqrt(((x.astype(np.float64) - ref)[m] ** 2).mean())) if m.any() else None
    res = {"size": [Wq, Hq], "frames": frames, "yaw_step": a.yaw_step, "S": S, "ref_spp": a.ref_spp, "budget_per_frame": budget,
           "boost": {"target": a.target, "max_units": a.max_units, "last_frame": b_last},
           "pixels": {"history_shorter_than_4": int(young.sum()), "rest": int((~young).sum())},
           "samples_per_frame": {"uniform": u_spent, "boosted": b_spent}, "samples_total": {"uniform": sum(u_spent), "boosted": sum(b_spent)},
           "rms_denoised": {"uniform": {"short": rms(u_out, young), "rest": rms(u_out, ~young)},
                            "boosted": {"short": rms(b_out, young), "rest": rms(b_out, ~young)}},
           "rms_accumulated": {"uniform": {"short": rms(u_acc, young), "rest": rms(u_acc, ~young)},
                               "boosted": {"short": rms(b_acc, young), "rest": rms(b_acc, ~young)}}}
    for k in ("pixels", "samples_total", "rms_denoised", "rms_accumulated"):
        print(k, json.dumps(res[k]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10, help="an even number, so that each order of a pair is timed as often as the other")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--yaw-step", type=float, default=None)
    ap.add_argument("--trace", action="store_true", help="a few calls of each kind for a kernel trace; nothing is timed")
    ap.add_argument("--quality", action="store_true", help="the equal-samples comparison of a uniform and a boosted sequence")
    ap.add_argument("--size", type=int, nargs=2, default=[480, 360], metavar=("W", "H"))
    ap.add_argument("--spp", type=int, default=8, help="--quality: S")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--target", type=int, default=8)
    ap.add_argument("--max-units", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.yaw_step is None:
        a.yaw_step = 2.0 if a.quality else 1.0
    res = quality(a) if a.quality else times(a)
    if res is None:
        return
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
