"""Adaptive frames on one GPU (include/frayhip.h "adaptive frames"): cost and equal-time quality against fixed-spp frames, from the library's own
timings (frayhip_stats.ms_kernels: HIP events around the call's device work; ms_total: the call's wall time, which for an adaptive frame includes the
host's one read-back per rung).  cornell_box 1920x1080, 64 spp, wantAA off; every call on one torch stream, outputs resident on the device; the
calls alternate round after round, medians over --rounds rounds after --warmup.

  frame              the blocking 64-spp frame (frayhip_render_device)
  frame_1lane        the same frame with option pt_lanes 1: its batches on one stream, as an adaptive frame runs
  adaptive_full      the adaptive path with min_spp = spp: the same image, every pixel through the rung pipeline
  adaptive_T_F       threshold T with err_floor F (min_spp --min-spp): time, mean spp, RMS against a 1024-spp frame of the same scene.  A small
                     floor makes the error relative (dark pixels count as much as bright ones); a floor of 1 makes it close to absolute, as RMS is
  fixed_N            fixed-spp frames of N samples: time and RMS against the same reference, to read equal-time quality off

    python tools/adaptive_rate.py [--rounds 5] [--warmup 1] [--cases 0.1:0.01 0.02:1 ...] [--min-spp 16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, SPP = 1920, 1080, 64
FIXED = [8, 16, 24, 32, 48, 64]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", nargs="+", default=["0.1:0.01", "0.05:0.01", "0.025:0.01", "0.02:1", "0.01:1", "0.005:1"], metavar="T:F",
                    help="threshold:err_floor pairs")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import fray_amd
    from conftest import open_scene

    fray_amd.lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    s = open_scene(fray_amd, "cornell_box.fray", W, H, gi=1, numPaths=SPP, wantAA=0)
    s.beginRender()

    def set_spp(n):
        s.settings.numPaths = n
        s.beginFrame()

    set_spp(a.ref_spp)
    ref, _ = s.render(seed=42)
    ref = ref.astype(np.float64)
    set_spp(SPP)
    with torch.cuda.stream(stream):
        rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        spp = torch.empty((H, W), dtype=torch.int32, device="cuda")
        err = torch.empty((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def rms():
        torch.cuda.synchronize()
        return float(np.sqrt(((rgb.cpu().numpy().astype(np.float64) - ref) ** 2).mean()))

    def frame(n, lanes=4):
        def run():
            if n != SPP:
                set_spp(n)
            s.set_option("pt_lanes", lanes)
            st = s.render_device(rgb.data_ptr(), seed=42, stream=h)
            s.set_option("pt_lanes", 4)
            if n != SPP:
                set_spp(SPP)
            return st, {}
        return run

    def adaptive(thr, mn, floor=0.01):
        def run():
            info = s.render_adaptive_device(rgb.data_ptr(), spp.data_ptr(), err.data_ptr(), threshold=thr, min_spp=mn, err_floor=floor, stream=h)
            return info["stats"], {"mean_spp": info["samples"] / float(W * H), "rungs": info["rungs"]}
        return run

    calls = [("frame", frame(SPP)), ("frame_1lane", frame(SPP, 1)), ("adaptive_full", adaptive(0.0, SPP))]
    cases = [tuple(float(v) for v in c.split(":")) for c in a.cases]
    names = ["adaptive_%g_%g" % c for c in cases]
    calls += [(n, adaptive(t, a.min_spp, f)) for n, (t, f) in zip(names, cases)]
    calls += [("fixed_%d" % n, frame(n)) for n in FIXED if n != SPP]
    times = {k: [] for k, _ in calls}
    extra = {}
    for r in range(a.warmup + a.rounds):
        for k, fn in calls:
            st, ex = fn()
            if r >= a.warmup:
                times[k].append((st["ms_kernels"], st["ms_total"]))
            if r == a.warmup + a.rounds - 1:
                extra[k] = dict(ex, rms=rms())
    res = {}
    for k, v in times.items():
        res[k] = {"kernels_ms": statistics.median(x[0] for x in v), "call_ms": statistics.median(x[1] for x in v)}
        res[k].update(extra[k])
    res["frame"]["mean_spp"] = res["frame_1lane"]["mean_spp"] = SPP
    for n in FIXED:
        if n != SPP:
            res["fixed_%d" % n]["mean_spp"] = n
    res["full_ratio_kernels"] = res["adaptive_full"]["kernels_ms"] / res["frame"]["kernels_ms"]
    res["full_ratio_call"] = res["adaptive_full"]["call_ms"] / res["frame"]["call_ms"]
    # equal time: the RMS of fixed-spp frames, linearly interpolated in call time, at each adaptive frame's call time
    fx = sorted([(res["fixed_%d" % n]["call_ms"], res["fixed_%d" % n]["rms"]) for n in FIXED if n != SPP] + [(res["frame"]["call_ms"], res["frame"]["rms"])])
    for k in names:
        res[k]["fixed_rms_at_equal_time"] = float(np.interp(res[k]["call_ms"], [x[0] for x in fx], [x[1] for x in fx]))
    for k, v in res.items():
        if isinstance(v, dict):
            print("%-22s kernels %8.2f ms  call %8.2f ms  mean spp %6.2f  rms %.5f%s" % (
                k, v["kernels_ms"], v["call_ms"], v["mean_spp"], v["rms"],
                ("  fixed-spp rms at equal time %.5f" % v["fixed_rms_at_equal_time"]) if "fixed_rms_at_equal_time" in v else ""), flush=True)
    print("adaptive_full / frame: kernels %.3f, call %.3f" % (res["full_ratio_kernels"], res["full_ratio_call"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    s.close()


if __name__ == "__main__":
    main()
