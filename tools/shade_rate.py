"""Radiance query rate on one GPU (include/frayhip.h "radiance queries") against the frame that shades the same samples, from the library's own
device events (frayhip_stats.ms_kernels: HIP events around the call's device work; ms_trace / ms_shadow: around each bounce / shadow launch).  The
query and the frame alternate round after round on one torch stream, inputs and outputs resident on the device; medians over --rounds rounds
after --warmup.

  cornell   cornell_box 1920x1080: the 64-spp frame (its batch lanes) against frayhip_shade_rays_device of one fixed camera ray per pixel x 64
            samples, rng_skip 2 (one stream)
  dragon    hw9/dragon 1920x1080 Whitted, one sample: the frame (its own choice of Whitted path) against the query of the camera rays (k_whitted_rays),
            and the frame with option speculate_fans 0 (the query does not trace glossy fans ahead)

    python tools/shade_rate.py [--rounds 9] [--warmup 2] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import fray_amd
    from fray_amd import abi
    from conftest import open_scene

    fray_amd.lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    results = {}
    cases = [("cornell", "cornell_box.fray", dict(gi=1, numPaths=64, wantAA=0), 64, 2),
             ("dragon", "hw9/dragon.fray", dict(gi=0, wantAA=0), 1, 0)]
    for name, scene, over, spp, skip in cases:
        s = open_scene(fray_amd, scene, 1920, 1080, **over)
        s.beginRender()
        o, d = s.camera_rays()
        with torch.cuda.stream(stream):
            do, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
            rgb = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
            frame = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        req = abi.ShadeRequest(seed=42, spp=spp, sample_first=0, rng_skip=skip, flags=0, keys=None)
        h = C.c_void_p(stream.cuda_stream)

        def query():
            st = abi.Stats()
            rc = fray_amd.lib.frayhip_shade_rays_device(s._dev, 1920 * 1080, do.data_ptr(), dd.data_ptr(), C.byref(req), rgb.data_ptr(), h, C.byref(st))
            assert rc == 0, fray_amd.lib.frayhip_last_error()
            return st.as_dict()

        def render():
            return s.render_device(frame.data_ptr(), seed=42, stream=h)

        def render_nofans():                  # the frame without speculative glossy fans, which the query does not use either
            s.set_option("speculate_fans", 0)
            st = s.render_device(frame.data_ptr(), seed=42, stream=h)
            s.set_option("speculate_fans", 1)
            return st

        calls = [("query", query), ("frame", render)] + ([("frame_nofans", render_nofans)] if not over["gi"] else [])
        times = {k: [] for k, _ in calls}
        for r in range(a.warmup + a.rounds):
            for k, fn in calls:
                st = fn()
                if r >= a.warmup:
                    times[k].append((st["ms_kernels"], st["ms_trace"], st["ms_shadow"], st["ms_total"]))
        res = {}
        for k, v in times.items():
            res[k] = {f: statistics.median(x[i] for x in v) for i, f in enumerate(("kernels", "trace", "shadow", "call"))}
        res["ratio"] = res["query"]["kernels"] / res["frame"]["kernels"]
        res["whitted_path"] = s.get_option("whitted_path") if not over["gi"] else None
        results[name] = res
        print("%-8s frame %8.2f ms (trace %7.2f, shadow %7.2f)   query %8.2f ms (trace %7.2f, shadow %7.2f)   ratio %.2f" % (
            name, res["frame"]["kernels"], res["frame"]["trace"], res["frame"]["shadow"], res["query"]["kernels"], res["query"]["trace"],
            res["query"]["shadow"], res["ratio"]) + ("   frame without fans %8.2f ms" % res["frame_nofans"]["kernels"] if "frame_nofans" in res else ""), flush=True)
        s.close()
    line = json.dumps(results)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
