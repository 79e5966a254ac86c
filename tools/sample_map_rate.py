"""Sample maps on one GPU (include/frayhip.h "sample maps"): what per-pixel sample counts cost beside the uniform entry, from the library's own timings
(frayhip_stats.ms_kernels: HIP events around the call's device work; ms_total: the call's wall time).  cornell_box 1920x1080, wantAA off; every call
on one torch stream, every buffer resident on the device, no counting kernels; the calls alternate round after round, medians over --rounds rounds
after --warmup.  Every call adds its samples on top of a state of 4 samples per pixel, so none of them starts a row.

  samples_16      frayhip_render_samples_device, samples 4 .. 19 of every pixel
  map_uniform_16  (a) frayhip_render_samples_map_device with add = 16 everywhere: the same samples, through lists, scan and expansion
  map_random_16   (b) add = 16 for one pixel in four, chosen at random, 0 elsewhere: a quarter of the samples, scattered over every wave's tile
  map_tiles_16    (b) add = 16 for one 8x8 tile in four, chosen at random: a quarter of the samples, whole tiles
  sample_map      (c) frayhip_sample_map_device alone, on the state that samples_16 leaves

(b) is to be read against a quarter of samples_16: what sparsity costs in wave coherence and in fixed work per call.

--split measures component states under a map instead (frayhip_render_components_map_device), on a pair of states of 4 samples per pixel:

  components_16        frayhip_render_components_device, samples 4 .. 19 of every pixel
  pair_uniform_16      frayhip_render_components_map_device with add = 16 everywhere, against components_16
  map_uniform_16, map_random_16, map_tiles_16      the single-state maps above, and
  pair_random_16, pair_tiles_16                    the pair maps of the same add: the same rays, a second row in the resolve and the finish
  sample_map, sample_map_pair                      frayhip_sample_map_device and frayhip_sample_map_pair_device alone

--budget measures the budgeted map instead (frayhip_sample_map_budget_device), on the state of 4 samples per pixel, beside the plain map in the same
run; the calls alternate round after round.  D = the plain map's samples at the tolerance, F = its samples at tolerance FLT_MAX:

  sample_map        frayhip_sample_map_device (tolerance 0.05, max_count 256)
  budget_stage0     the budgeted entry with budget D: the prepare pass, eight search launches that return at once, the final pass
  budget_stage1     budget (D + F) / 2: the search runs over the tolerance's bit pattern
  budget_stage2     budget F8 / 2 with min_count 8, where F8 = 4 W H is what no tolerance removes (at min_count 4 a state of 4 samples has
                    F = 0 and no budget reaches stage 2): the search runs over the cap
  samples_1_over_16 one sixteenth of frayhip_render_samples_device's 16 samples: the sample per pixel the map is steering

    python tools/sample_map_rate.py [--split | --budget] [--rounds 7] [--warmup 2] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, BASE, ADD = 1920, 1080, 4, 16


def med(v):
    return {"kernels_ms": statistics.median(x[0] for x in v), "call_ms": statistics.median(x[1] for x in v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--split", action="store_true", help="measure the pair entries (component states under a map) beside the single-state ones")
    ap.add_argument("--budget", action="store_true", help="measure the budgeted map (frayhip_sample_map_budget_device) at stage 0, 1 and 2 beside the plain map")
    a = ap.parse_args()
    if a.budget and a.split:
        ap.error("--budget and --split are separate measurements")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import fray_amd
    from conftest import open_scene
    abi, lib = fray_amd.abi, fray_amd.lib

    lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    s = open_scene(fray_amd, "cornell_box.fray", W, H, gi=1, numPaths=ADD, wantAA=0)
    s.beginRender()
    gen = torch.Generator(device="cpu").manual_seed(7)
    with torch.cuda.stream(stream):
        base = fray_amd.Accumulation.empty((W, H), device="cuda")
        s.render_samples(BASE, base, stream=stream)
        acc = torch.empty_like(base.state)
        rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        noise = torch.empty((H, W), dtype=torch.float32, device="cuda")
        count = torch.empty((H, W), dtype=torch.int32, device="cuda")
        out_add = torch.empty((H, W), dtype=torch.int32, device="cuda")
        uniform = torch.full((H, W), ADD, dtype=torch.int32, device="cuda")
        scattered = ((torch.rand((H, W), generator=gen) < 0.25).to(torch.int32) * ADD).cuda()
        tiles = (torch.rand(((H + 7) // 8, (W + 7) // 8), generator=gen) < 0.25).to(torch.int32) * ADD
        tiled = tiles.repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W].contiguous().cuda()
    torch.cuda.synchronize()
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, flags=0)

    def reset():
        with torch.cuda.stream(stream):
            acc.copy_(base.state)
            count.fill_(BASE)
        stream.synchronize()

    def samples():
        reset()
        req, st = abi.Samples(sample_first=BASE, sample_count=ADD), abi.Stats()
        rc = lib.frayhip_render_samples_device(s._dev, C.byref(fr), C.byref(req), None, acc.data_ptr(), rgb.data_ptr(), noise.data_ptr(), h, C.byref(st))
        if rc:
            sys.exit("frayhip_render_samples_device: %s" % lib.frayhip_last_error().decode())
        return st.ms_kernels, st.ms_total

    def mapped(add):
        def run():
            reset()
            req, st = abi.SamplesMap(), abi.Stats()
            rc = lib.frayhip_render_samples_map_device(s._dev, C.byref(fr), C.byref(req), acc.data_ptr(), count.data_ptr(), add.data_ptr(), rgb.data_ptr(),
                                                       noise.data_ptr(), h, C.byref(st))
            if rc:
                sys.exit("frayhip_render_samples_map_device: %s" % lib.frayhip_last_error().decode())
            assert req.samples == int(add.sum())
            return st.ms_kernels, st.ms_total
        return run

    def sample_map():
        p, st = fray_amd.sample_map_params(tolerance=0.05, max_count=256), abi.Stats()
        rc = lib.frayhip_sample_map_device(W, H, acc.data_ptr(), count.data_ptr(), C.byref(p), out_add.data_ptr(), h, C.byref(st))
        if rc:
            sys.exit("frayhip_sample_map_device: %s" % lib.frayhip_last_error().decode())
        return st.ms_kernels, st.ms_total

    if a.budget:
        import numpy as np
        reset()

        def plain(**kw):
            p, st = fray_amd.sample_map_params(**dict(dict(tolerance=0.05, max_count=256), **kw)), abi.Stats()
            rc = lib.frayhip_sample_map_device(W, H, acc.data_ptr(), count.data_ptr(), C.byref(p), out_add.data_ptr(), h, C.byref(st))
            if rc:
                sys.exit("frayhip_sample_map_device: %s" % lib.frayhip_last_error().decode())
            return p, st

        D = int(plain()[0].samples)
        F = int(plain(tolerance=float(np.finfo(np.float32).max))[0].samples)
        F8 = int(plain(tolerance=float(np.finfo(np.float32).max), min_count=8)[0].samples)
        seen = {}

        def budgeted(name, budget, stage, **kw):
            def run():
                p, st = fray_amd.sample_map_params(**dict(dict(tolerance=0.05, max_count=256), **kw)), abi.Stats()
                b = abi.SampleBudget(budget=budget)
                rc = lib.frayhip_sample_map_budget_device(W, H, acc.data_ptr(), None, count.data_ptr(), C.byref(p), C.byref(b), out_add.data_ptr(), h, C.byref(st))
                if rc:
                    sys.exit("frayhip_sample_map_budget_device: %s" % lib.frayhip_last_error().decode())
                assert b.stage == stage and p.samples <= budget, (name, b.stage, p.samples, budget)
                seen[name] = {"budget": budget, "demand": int(b.demand), "samples": int(p.samples), "pixels": int(p.pixels), "stage": int(b.stage),
                              "tolerance_used": float(b.tolerance_used), "cap_used": int(b.cap_used)}
                return st.ms_kernels, st.ms_total
            return run

        def plain_map():
            _, st = plain()
            return st.ms_kernels, st.ms_total

        def samples_then_reset():
            v = samples()
            reset()
            return v

        calls = [("sample_map", plain_map), ("budget_stage0", budgeted("budget_stage0", D, 0)), ("budget_stage1", budgeted("budget_stage1", (D + F) // 2, 1)),
                 ("budget_stage2", budgeted("budget_stage2", F8 // 2, 2, min_count=8)), ("samples_16", samples_then_reset)]
        times = {k: [] for k, _ in calls}
        for r in range(a.warmup + a.rounds):
            for k, fn in calls:
                v = fn()
                if r >= a.warmup:
                    times[k].append(v)
        res = {k: med(v) for k, v in times.items()}
        res["spread_kernels_ms"] = {k: [min(x[0] for x in v), max(x[0] for x in v)] for k, v in times.items()}
        res["samples_1_over_16"] = {"kernels_ms": res["samples_16"]["kernels_ms"] / ADD}
        res["maps"] = dict(seen, D=D, F=F, F8=F8)
        one = res["samples_1_over_16"]["kernels_ms"]
        res["ratios"] = {k + "_over_one_sample_per_pixel": res[k]["kernels_ms"] / one for k in ("sample_map", "budget_stage0", "budget_stage1", "budget_stage2")}
        for k, _ in calls:
            print("%-15s kernels %8.3f ms  call %8.3f ms" % (k, res[k]["kernels_ms"], res[k]["call_ms"]), flush=True)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        s.close()
        return

    if a.split:
        with torch.cuda.stream(stream):
            pair = (fray_amd.Accumulation.empty((W, H), device="cuda"), fray_amd.Accumulation.empty((W, H), device="cuda"))
            s.render_components(BASE, pair, stream=stream)
            acc_d, acc_i = torch.empty_like(pair[0].state), torch.empty_like(pair[1].state)
            rgb_i = torch.empty_like(rgb)
            noise_i = torch.empty_like(noise)
        torch.cuda.synchronize()

        def reset_pair():
            with torch.cuda.stream(stream):
                acc_d.copy_(pair[0].state)
                acc_i.copy_(pair[1].state)
                count.fill_(BASE)
            stream.synchronize()

        def components():
            reset_pair()
            req, st = abi.Samples(sample_first=BASE, sample_count=ADD), abi.Stats()
            rc = lib.frayhip_render_components_device(s._dev, C.byref(fr), C.byref(req), None, acc_d.data_ptr(), acc_i.data_ptr(), rgb.data_ptr(),
                                                      rgb_i.data_ptr(), noise.data_ptr(), noise_i.data_ptr(), h, C.byref(st))
            if rc:
                sys.exit("frayhip_render_components_device: %s" % lib.frayhip_last_error().decode())
            return st.ms_kernels, st.ms_total

        def mapped_pair(add):
            def run():
                reset_pair()
                req, st = abi.SamplesMap(), abi.Stats()
                rc = lib.frayhip_render_components_map_device(s._dev, C.byref(fr), C.byref(req), acc_d.data_ptr(), acc_i.data_ptr(), count.data_ptr(),
                                                              add.data_ptr(), rgb.data_ptr(), rgb_i.data_ptr(), noise.data_ptr(), noise_i.data_ptr(), h,
                                                              C.byref(st))
                if rc:
                    sys.exit("frayhip_render_components_map_device: %s" % lib.frayhip_last_error().decode())
                assert req.samples == int(add.sum())
                return st.ms_kernels, st.ms_total
            return run

        def sample_map_pair():
            p, st = fray_amd.sample_map_params(tolerance=0.05, max_count=256), abi.Stats()
            rc = lib.frayhip_sample_map_pair_device(W, H, acc_d.data_ptr(), acc_i.data_ptr(), count.data_ptr(), C.byref(p), out_add.data_ptr(), h, C.byref(st))
            if rc:
                sys.exit("frayhip_sample_map_pair_device: %s" % lib.frayhip_last_error().decode())
            return st.ms_kernels, st.ms_total

        # every pair map follows the single-state map of the same add; the two sample maps read the states their predecessors left
        calls = [("map_uniform_16", mapped(uniform)), ("pair_uniform_16", mapped_pair(uniform)), ("map_random_16", mapped(scattered)),
                 ("pair_random_16", mapped_pair(scattered)), ("map_tiles_16", mapped(tiled)), ("pair_tiles_16", mapped_pair(tiled)),
                 ("samples_16", samples), ("sample_map", sample_map), ("components_16", components), ("sample_map_pair", sample_map_pair)]
        times = {k: [] for k, _ in calls}
        for r in range(a.warmup + a.rounds):
            for k, fn in calls:
                v = fn()
                if r >= a.warmup:
                    times[k].append(v)
        res = {k: med(v) for k, v in times.items()}
        res["map_samples"] = {"uniform": int(uniform.sum()), "random": int(scattered.sum()), "tiles": int(tiled.sum())}
        ms = lambda k: res[k]["kernels_ms"]
        res["ratios"] = {"a_pair_over_map_uniform": ms("pair_uniform_16") / ms("map_uniform_16"),
                         "a_pair_over_map_random": ms("pair_random_16") / ms("map_random_16"),
                         "a_pair_over_map_tiles": ms("pair_tiles_16") / ms("map_tiles_16"),
                         "b_uniform_pair_map_over_components": ms("pair_uniform_16") / ms("components_16")}
        for k, _ in calls:
            print("%-15s kernels %8.2f ms  call %8.2f ms" % (k, res[k]["kernels_ms"], res[k]["call_ms"]), flush=True)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        s.close()
        return

    # sample_map follows samples_16 in every round: it reads the state and the counts (BASE, as reset() left them) of that call
    calls = [("map_uniform_16", mapped(uniform)), ("map_random_16", mapped(scattered)), ("map_tiles_16", mapped(tiled)), ("samples_16", samples),
             ("sample_map", sample_map)]
    times = {k: [] for k, _ in calls}
    for r in range(a.warmup + a.rounds):
        for k, fn in calls:
            v = fn()
            if r >= a.warmup:
                times[k].append(v)
    res = {k: med(v) for k, v in times.items()}
    res["map_samples"] = {"uniform": int(uniform.sum()), "random": int(scattered.sum()), "tiles": int(tiled.sum())}
    u = res["samples_16"]["kernels_ms"]
    res["ratios"] = {"a_uniform_map_over_samples": res["map_uniform_16"]["kernels_ms"] / u,
                     "b_random_over_its_share": res["map_random_16"]["kernels_ms"] / (u * res["map_samples"]["random"] / res["map_samples"]["uniform"]),
                     "b_tiles_over_its_share": res["map_tiles_16"]["kernels_ms"] / (u * res["map_samples"]["tiles"] / res["map_samples"]["uniform"])}
    for k, _ in calls:
        print("%-15s kernels %8.2f ms  call %8.2f ms" % (k, res[k]["kernels_ms"], res[k]["call_ms"]), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    s.close()


if __name__ == "__main__":
    main()
