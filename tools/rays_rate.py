"""Ray query throughput on one GPU (include/frayhip.h "ray queries"), from the library's own device events (frayhip_stats.ms_trace / ms_shadow:
HIP events around the query kernel's launch; ms_kernels around the whole call's device work).  The calls of a group alternate round after round,
all on one torch stream, inputs and outputs resident on the device; medians over --rounds rounds after --warmup.

  primary   per scene (cornell_box, hw9/dragon at 1920x1080): the MODE_PRIMARY_ID frame (k_primary) against trace_rays of the same 1080p camera
            rays in row-major order, ids + dist only and with the hit record, and ids + dist of the rays in 8x8 pixel tiles (k_primary's order)
  incoherent  trace_rays of the fixtures' ray sets (tests/golden/ref_*.npz: camera rays and secondary rays from hit points), each set repeated to
            --incoherent-rays rays, in Grays/s
  visible   visible() of --segments segments: 1080p camera-ray hit points of cornell_box to random points of its rect light

    python tools/rays_rate.py [--rounds 15] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INCOHERENT = ["dragon_whitted", "forest_env_whitted", "boxed_whitted", "cornell_pt", "csg_nested", "smallpt_pt"]


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--incoherent-rays", type=int, default=1 << 21)
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    import fray_amd
    from fray_amd import abi
    fray_amd.lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    result = {"rounds": a.rounds, "warmup": a.warmup, "primary": {}, "incoherent": {}, "visible": {}}

    def rounds(calls):
        """calls: name -> fn returning the stats dict; alternated; medians of the device times"""
        times = {k: {"kernel": [], "device": [], "wall": []} for k in calls}
        for r in range(a.warmup + a.rounds):
            for k, fn in calls.items():
                st = fn()
                if r >= a.warmup:
                    times[k]["kernel"].append(st["ms_trace"] + st["ms_shadow"])
                    times[k]["device"].append(st["ms_kernels"])
                    times[k]["wall"].append(st["ms_total"])
        return {k: {m: med(v) for m, v in t.items()} for k, t in times.items()}

    for scene in ("cornell_box.fray", "hw9/dragon.fray"):
        s = fray_amd.Scene.parseScene(os.path.join(ROOT, "scenes", scene))
        s.settings.frameWidth, s.settings.frameHeight, s.settings.wantAA = 1920, 1080, 0
        s.beginRender()
        with torch.cuda.stream(stream):
            ids = torch.empty((1080, 1920), dtype=torch.int32, device="cuda")
            dist = torch.empty((1080, 1920), dtype=torch.float64, device="cuda")
            o, d = s.camera_rays()
            o, d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
            # the same rays in 8x8 pixel tiles, the order in which k_primary's waves take a frame's pixels (the caller's choice of order)
            tile = torch.arange(1080 * 1920, device="cuda").reshape(135, 8, 240, 8).permute(0, 2, 1, 3).reshape(-1)
            ot, dt = o.reshape(-1, 3)[tile].contiguous(), d.reshape(-1, 3)[tile].contiguous()
        h = stream.cuda_stream
        calls = {
            "MODE_PRIMARY_ID": lambda: s.render_device(None, mode=abi.MODE_PRIMARY_ID, d_id_ptr=ids.data_ptr(), d_dist_ptr=dist.data_ptr(), stream=h),
            "trace_rays": lambda: s.trace_rays(o, d, stream=stream)["stats"],
            "trace_rays+rec": lambda: s.trace_rays(o, d, record=True, stream=stream)["stats"],
            "trace_rays_tiled": lambda: s.trace_rays(ot, dt, stream=stream)["stats"],
        }
        r = rounds(calls)
        chk = s.trace_rays(o, d, stream=stream)
        assert torch.equal(chk["hit_id"], ids) and torch.equal(chk["hit_dist"], dist), "trace_rays differs from MODE_PRIMARY_ID"
        chk = s.trace_rays(ot, dt, stream=stream)
        assert torch.equal(chk["hit_id"], ids.reshape(-1)[tile]), "trace_rays (tile order) differs from MODE_PRIMARY_ID"
        for k in ("trace_rays", "trace_rays+rec", "trace_rays_tiled"):
            r[k]["vs_primary"] = r[k]["kernel"] / r["MODE_PRIMARY_ID"]["kernel"]
        result["primary"][scene] = r
        for k, v in r.items():
            print("%-18s %-16s kernel %8.3f ms  device %8.3f ms  call %8.3f ms%s" % (scene, k, v["kernel"], v["device"], v["wall"],
                  "  x%.3f of MODE_PRIMARY_ID" % v["vs_primary"] if "vs_primary" in v else ""), flush=True)
        s.close()

    from test_oracle_vs_ref import load_case
    for name in INCOHERENT:
        z, s = load_case(fray_amd, os.path.join(ROOT, "tests", "golden", "ref_%s.npz" % name))
        s.beginRender()
        S, D = z["ray_start"], z["ray_dir"]
        reps = max(1, a.incoherent_rays // len(S))
        with torch.cuda.stream(stream):
            o = torch.from_numpy(np.ascontiguousarray(np.tile(S, (reps, 1)))).cuda()
            d = torch.from_numpy(np.ascontiguousarray(np.tile(D, (reps, 1)))).cuda()
        r = rounds({"trace_rays": lambda: s.trace_rays(o, d, stream=stream)["stats"],
                    "trace_rays+rec": lambda: s.trace_rays(o, d, record=True, stream=stream)["stats"]})
        n = len(o)
        for k in r:
            r[k]["rays"] = n
            r[k]["grays_per_s"] = n / (r[k]["kernel"] * 1e-3) / 1e9
        result["incoherent"][name] = r
        print("%-18s %d rays (%d distinct): ids+dist %.3f ms = %.3f Grays/s, with record %.3f ms = %.3f Grays/s" % (
            name, n, len(S), r["trace_rays"]["kernel"], r["trace_rays"]["grays_per_s"], r["trace_rays+rec"]["kernel"], r["trace_rays+rec"]["grays_per_s"]), flush=True)
        s.close()

    s = fray_amd.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    s.settings.frameWidth, s.settings.frameHeight = 1920, 1080
    s.beginRender()
    o, d = s.camera_rays()
    rec = s.trace_rays(o, d, record=True)
    hit = rec["hit_rec"][rec["hit_id"] >= 0, 1:4]
    rng = np.random.default_rng(3)
    a_pts = hit[rng.integers(0, len(hit), a.segments)]
    L = s.desc.lights[0]
    b_pts = np.array(L.center[:]) + (rng.random((a.segments, 3)) - 0.5) * [0.5, 0, 0.5]
    with torch.cuda.stream(stream):
        ta, tb = torch.from_numpy(np.ascontiguousarray(a_pts)).cuda(), torch.from_numpy(np.ascontiguousarray(b_pts)).cuda()
    r = rounds({"visible": lambda: s.visible(ta, tb, stream=stream)[1]})["visible"]
    r["segments"] = a.segments
    r["gsegments_per_s"] = a.segments / (r["kernel"] * 1e-3) / 1e9
    vis, _ = s.visible(ta, tb, stream=stream)
    r["visible_share"] = float(vis.float().mean())
    result["visible"]["cornell_box.fray"] = r
    print("visible            %d segments: %.3f ms = %.3f Gsegments/s (%.1f %% visible)" % (a.segments, r["kernel"], r["gsegments_per_s"], 100 * r["visible_share"]), flush=True)
    s.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
