"""Change frames and gradient-adaptive accumulation on one GPU (include/frayhip.h "change frames"), the records of profiles/change/README.md.

1. Timing, 1920x1080, cornell_box at 4 spp whose short block (node 5) has moved: k_ch_frame (frayhip_change_frame_device on the states of
   samples [0, 2) before and after the move, with the motion frame), frayhip_temporal_accumulate_adaptive_device with that change frame, and
   the entry it extends (frayhip_temporal_accumulate_motion_device, or frayhip_temporal_accumulate_device with --no-motion rows) on the same
   inputs.  The three ALTERNATE in one loop of one process (a drifting clock or a busy neighbour hits all alike), --warmup rounds first, then
   the median of --rounds rounds each.  Times are the library's own (frayhip_stats.ms_kernels: HIP events around each call's kernels).  Rows:
   frame 0 (no history: every pixel takes k_tp_variance's 7x7 window, the kernel whose tile shape k_ch_frame has) and steady state (a history
   four frames deep under a still camera), each with and without the motion frame.  young_share is the share of pixels that take the window
   after the call: the adaptive entry sends the changed pixels back to it.
   --plain-only measures the two existing entries alone and needs nothing of this feature: run it in a checkout of the commit before, on the
   same box, for the comparison with the parent.
2. --sequence: a --frames-frame cornell_box sequence, --size (320x240) at --spp (4) samples, still camera, the short block translated before every frame, as
   Scene.render_sequence(edit=...) renders it with and without change_samples=2, unsplit and split.  Per frame: the wall time of the frame
   (the median over --repeats runs that alternate between the variants).  The error is the mean absolute difference, per channel, of the
   last frame's picture from a 1024-spp frame of the last pose, over the shadow's previous footprint: the pixels that show the same static
   surface point in every pose and whose direct light at the last pose (1024 spp) is brighter by more than --lit than the darkest it was at
   any earlier pose (256 spp each) -- tools/temporal_split_rate.py's mask, which that tool's record found to be dominated by noisy bright
   pixels.  mae_changed is the same error over a mask that has no noise in it: the static pixels whose DIRECT state of samples [0, 2) differs
   in any bit between the scene before and after some frame's move (the union over the frames of a split run's change_direct > 0 at radius 0)
   -- the pixels the block's shadow left or reached.
3. --split: frayhip_temporal_accumulate_split_adaptive_device against what it replaces, 1920x1080, cornell_box at 4 spp as components, the
   tall block moved by tests/scene_edits.py's cornell-block edit between frame 0 and frame 1, through the motion frame, onto a split history
   four frames deep, with the sequence's parameters (direct max_history 8).  Two rows: "sparse" passes the direct component's change frame
   for both components (zero on most pixels), "block" each component's own.  Per row, ALTERNATING in one loop of one process: (a) ms_kernels
   of the fused device call and of the two adaptive device calls on the history's parts (their sum); (b) the wall time, device synchronised
   before and after, of the step Scene.render_sequence(split=True, change_samples=n) runs per frame -- one
   temporal_accumulate_split(change_direct=, change_indirect=) -- and of the step it ran before: split_history_parts, two
   temporal_accumulate(change=), join_history_parts.  bit_equal: the two steps' five outputs hold the same bits.

    python tools/change_rate.py [--rounds 21] [--warmup 3] [--plain-only] [--out FILE]
    python tools/change_rate.py --split [--rounds 21] [--warmup 3] [--out FILE]
    python tools/change_rate.py --sequence [--frames 6] [--repeats 5] [--size W H] [--spp N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
NODE, STEP = 5, (8.0, 0.0, -4.0)
PROBE = 2
BLOCK_NODE, BLOCK_STEP = 6, (30.0, 0.0, 5.0)          # tests/scene_edits.py's cornell-block: the tall block, reset and translated


def timing(a, fray_amd, abi, open_scene):
    import ctypes as C
    import torch
    L = fray_amd.lib
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    s = open_scene(fray_amd, "cornell_box.fray", W, H, wantAA=0, numPaths=4)
    s.beginRender()
    view = fray_amd.view_from_camera(s.camera, W, H)
    fresh = lambda seed: fray_amd.Accumulation.empty((W, H), seed, device="cuda")
    with torch.cuda.stream(stream):
        # frame 0, then frame 1: its probe before the move, the move, its features and motion frame, its first PROBE samples, the rest
        prev = s.node_transforms()
        feat0, motion0 = new(H, W, 10), new(H, W, 8)
        fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
        assert L.frayhip_render_features_motion_device(s._dev, C.byref(fr), 4, prev, len(prev), feat0.data_ptr(), motion0.data_ptr(), h, None) == 0
        rgb0 = s.render_samples(4, fresh(42), seed=42, stream=stream)[0]
        probe = fresh(43)
        s.render_samples(PROBE, probe, seed=43, stream=stream)
        fray_amd.Transform(s.nodes[NODE]).translate(*STEP).store(s.nodes[NODE])
        s.update()
        feat1, motion1 = new(H, W, 10), new(H, W, 8)
        fr = abi.Frame(mode=abi.MODE_RENDER, seed=43)
        assert L.frayhip_render_features_motion_device(s._dev, C.byref(fr), 4, prev, len(prev), feat1.data_ptr(), motion1.data_ptr(), h, None) == 0
        state = fresh(43)
        s.render_samples(PROBE, state, seed=43, stream=stream)
        first = state.state.clone()
        rgb1 = s.render_samples(4 - PROBE, state, seed=43, stream=stream)[0]
    s.close()
    frames = [(rgb0, feat0, motion0), (rgb1, feat1, motion1)]
    p = fray_amd.temporal_params()
    with torch.cuda.stream(stream):
        out = dict(h=new(H, W, 12), s=new(H, W, 3), v=new(H, W), c=new(H, W))

    def plain(frame, motion, hin, hout=None):
        rgb, feat, mot = frames[frame]
        st = abi.Stats()
        vp, hp = (C.byref(view), hin.data_ptr()) if hin is not None else (None, None)
        ho = (hout if hout is not None else out["h"]).data_ptr()
        if motion:
            rc = L.frayhip_temporal_accumulate_motion_device(W, H, rgb.data_ptr(), feat.data_ptr(), mot.data_ptr(), vp, hp, C.byref(p), ho,
                                                             out["s"].data_ptr(), out["v"].data_ptr(), h, C.byref(st))
        else:
            rc = L.frayhip_temporal_accumulate_device(W, H, rgb.data_ptr(), feat.data_ptr(), vp, hp, C.byref(p), ho, out["s"].data_ptr(),
                                                      out["v"].data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st.ms_kernels

    def change(frame, motion):
        cp = fray_amd.change_params()
        st = abi.Stats()
        rc = L.frayhip_change_frame_device(W, H, probe.state.data_ptr(), first.data_ptr(), frames[frame][2].data_ptr() if motion else None, C.byref(cp),
                                           out["c"].data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st.ms_kernels

    def adaptive(frame, motion, hin):
        rgb, feat, mot = frames[frame]
        st = abi.Stats()
        vp, hp = (C.byref(view), hin.data_ptr()) if hin is not None else (None, None)
        rc = L.frayhip_temporal_accumulate_adaptive_device(W, H, rgb.data_ptr(), feat.data_ptr(), mot.data_ptr() if motion else None, out["c"].data_ptr(), vp,
                                                           hp, C.byref(p), out["h"].data_ptr(), out["s"].data_ptr(), out["v"].data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st.ms_kernels

    # the steady-state history: frame 0 accumulated onto itself under the still camera until N = 4 everywhere it can be
    hs = [new(H, W, 12), new(H, W, 12)]
    plain(0, False, None, hs[0])
    for k in range(3):
        plain(0, False, hs[k % 2], hs[(k + 1) % 2])
    steady = hs[1]
    res = {"library": os.path.relpath(fray_amd.render_info()["library"], ROOT), "size": [W, H], "rounds": a.rounds, "warmup": a.warmup,
           "steady_young_share": float((steady[..., 3] < 4).float().mean())}
    young = lambda: float((out["h"][..., 3] < 4).float().mean())
    med = statistics.median
    for name, motion, hin in (("frame0", False, None), ("frame0_motion", True, None), ("steady", False, steady), ("steady_motion", True, steady)):
        c, ad, pl = [], [], []
        row = {}
        for r in range(a.warmup + a.rounds):
            z = plain(1, motion, hin)
            if r == 0:
                row["plain_young_share"] = young()
            if not a.plain_only:
                x = change(1, motion)
                y = adaptive(1, motion, hin)
                if r == 0:
                    row["adaptive_young_share"] = young()
                    row["changed_share"] = float((out["c"] > 0).float().mean())
            if r >= a.warmup:
                pl.append(z)
                if not a.plain_only:
                    c.append(x)
                    ad.append(y)
        row.update(plain_ms=med(pl), plain_min_max=[min(pl), max(pl)])
        if not a.plain_only:
            row.update(change_frame_ms=med(c), change_frame_min_max=[min(c), max(c)], adaptive_ms=med(ad), adaptive_min_max=[min(ad), max(ad)],
                       adaptive_over_plain=med(ad) / med(pl))
        res[name] = row
        print(name, json.dumps(row), flush=True)
    return res


def split_timing(a, fray_amd, abi, open_scene):
    import ctypes as C
    import torch
    L = fray_amd.lib
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    s = open_scene(fray_amd, "cornell_box.fray", W, H, wantAA=0, numPaths=4)
    s.beginRender()
    view = fray_amd.view_from_camera(s.camera, W, H)
    pair_of = lambda seed: tuple(fray_amd.Accumulation.empty((W, H), seed, device="cuda") for _ in range(2))
    with torch.cuda.stream(stream):
        # frame 0, then frame 1 as render_sequence(split=True, change_samples=PROBE) renders it around the cornell-block edit
        prev = s.node_transforms()
        feat0, motion0 = new(H, W, 10), new(H, W, 8)
        fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
        assert L.frayhip_render_features_motion_device(s._dev, C.byref(fr), 4, prev, len(prev), feat0.data_ptr(), motion0.data_ptr(), h, None) == 0
        d0, i0, _ = s.render_components(4, pair_of(42), seed=42, stream=stream)
        probe = pair_of(43)
        s.render_components(PROBE, probe, seed=43, stream=stream)
        fray_amd.Transform().translate(*BLOCK_STEP).store(s.nodes[BLOCK_NODE])
        s.update()
        feat, motion = new(H, W, 10), new(H, W, 8)
        fr = abi.Frame(mode=abi.MODE_RENDER, seed=43)
        assert L.frayhip_render_features_motion_device(s._dev, C.byref(fr), 4, prev, len(prev), feat.data_ptr(), motion.data_ptr(), h, None) == 0
        state = pair_of(43)
        s.render_components(PROBE, state, seed=43, stream=stream)
        first = [x.state.clone() for x in state]
        d1, i1, _ = s.render_components(4 - PROBE, state, seed=43, stream=stream)
        chg_d = fray_amd.change_frame(probe[0], first[0], motion, stream=stream)
        chg_i = fray_amd.change_frame(probe[1], first[1], motion, stream=stream)
    s.close()
    tdirect, tindirect = dict(max_history=8), dict()                      # render_sequence's defaults
    pd, pi = fray_amd.temporal_params(**tdirect), fray_amd.temporal_params(**tindirect)
    with torch.cuda.stream(stream):
        out = dict(hs=new(H, W, 20), hd=new(H, W, 12), hi=new(H, W, 12), sd=new(H, W, 3), si=new(H, W, 3), vd=new(H, W), vi=new(H, W))
        # the steady-state history: frame 0 accumulated onto itself under the still camera, four frames deep
        hs = [new(H, W, 20), new(H, W, 20)]
        for k in range(4):
            rc = L.frayhip_temporal_accumulate_split_device(W, H, d0.data_ptr(), i0.data_ptr(), feat0.data_ptr(), motion0.data_ptr(),
                                                            C.byref(view) if k else None, hs[(k + 1) % 2].data_ptr() if k else None, C.byref(pd), C.byref(pi),
                                                            hs[k % 2].data_ptr(), out["sd"].data_ptr(), out["si"].data_ptr(), out["vd"].data_ptr(),
                                                            out["vi"].data_ptr(), h, None)
            assert rc == 0, L.frayhip_last_error()
        steady = hs[1]
        parts = fray_amd.split_history_parts(steady)

    def fused_kernels(cd, ci):
        st = abi.Stats()
        rc = L.frayhip_temporal_accumulate_split_adaptive_device(W, H, d1.data_ptr(), i1.data_ptr(), feat.data_ptr(), motion.data_ptr(), cd.data_ptr(),
                                                                 ci.data_ptr(), C.byref(view), steady.data_ptr(), C.byref(pd), C.byref(pi), out["hs"].data_ptr(),
                                                                 out["sd"].data_ptr(), out["si"].data_ptr(), out["vd"].data_ptr(), out["vi"].data_ptr(), h,
                                                                 C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st.ms_kernels

    def pair_kernels(cd, ci):
        ms = 0.0
        for rgb, c, hin, hout, sig, var, p in ((d1, cd, parts[0], out["hd"], out["sd"], out["vd"], pd), (i1, ci, parts[1], out["hi"], out["si"], out["vi"], pi)):
            st = abi.Stats()
            rc = L.frayhip_temporal_accumulate_adaptive_device(W, H, rgb.data_ptr(), feat.data_ptr(), motion.data_ptr(), c.data_ptr(), C.byref(view),
                                                               hin.data_ptr(), C.byref(p), hout.data_ptr(), sig.data_ptr(), var.data_ptr(), h, C.byref(st))
            assert rc == 0, L.frayhip_last_error()
            ms += st.ms_kernels
        return ms

    def fused_step(cd, ci):                                               # what render_sequence runs per frame with a probe
        return fray_amd.temporal_accumulate_split(d1, i1, feat, view, steady, motion=motion, direct=tdirect, indirect=tindirect, stats=True, stream=stream,
                                                  change_direct=cd, change_indirect=ci)[:5]

    def unfused_step(cd, ci):                                             # what it ran before: take-apart, two adaptive calls, join
        hd, hi = fray_amd.split_history_parts(steady)
        hd, sd, vd, _ = fray_amd.temporal_accumulate(d1, feat, view, hd, stats=True, stream=stream, motion=motion, change=cd, **tdirect)
        hi, si, vi, _ = fray_amd.temporal_accumulate(i1, feat, view, hi, stats=True, stream=stream, motion=motion, change=ci, **tindirect)
        return fray_amd.join_history_parts(hd, hi), sd, si, vd, vi

    def wall(f, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            r = f(*args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    res = {"library": os.path.relpath(fray_amd.render_info()["library"], ROOT), "size": [W, H], "rounds": a.rounds, "warmup": a.warmup,
           "node": BLOCK_NODE, "step": BLOCK_STEP, "change_samples": PROBE,
           "changed_share_direct": float((chg_d > 0).float().mean()), "changed_share_indirect": float((chg_i > 0).float().mean()),
           "steady_young_share_direct": float((steady[..., 3] < 4).float().mean()), "steady_young_share_indirect": float((steady[..., 15] < 4).float().mean())}
    med = statistics.median
    # "sparse": the direct component's change frame for both components (inputs may alias), zero on most pixels; "block": each component's own
    for name, cd, ci in (("sparse", chg_d, chg_d), ("block", chg_d, chg_i)):
        fk, pk, fw, uw = [], [], [], []
        row = {"changed_share": [float((cd > 0).float().mean()), float((ci > 0).float().mean())]}
        for r in range(a.warmup + a.rounds):
            x = fused_kernels(cd, ci)
            y = pair_kernels(cd, ci)
            tf, got = wall(fused_step, cd, ci)
            tu, want = wall(unfused_step, cd, ci)
            if r == 0:
                row["bit_equal"] = all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))
                row["young_share"] = [float((got[0][..., 3] < 4).float().mean()), float((got[0][..., 15] < 4).float().mean())]
            if r >= a.warmup:
                fk.append(x); pk.append(y); fw.append(tf); uw.append(tu)
        row.update(fused_kernels_ms=med(fk), fused_kernels_min_max=[min(fk), max(fk)], pair_kernels_ms=med(pk), pair_kernels_min_max=[min(pk), max(pk)],
                   kernels_ratio=med(fk) / med(pk), fused_step_ms=med(fw), fused_step_min_max=[min(fw), max(fw)], unfused_step_ms=med(uw),
                   unfused_step_min_max=[min(uw), max(uw)], step_ratio=med(fw) / med(uw))
        res[name] = row
        print(name, json.dumps(row), flush=True)
    return res


def sequence(a, fray_amd, abi, open_scene):
    import numpy as np
    import torch
    (w, h), spp, pose_spp, truth_spp = a.size, a.spp, 256, 1024
    over = dict(wantAA=0, numPaths=spp)

    def move(scene):
        fray_amd.Transform(scene.nodes[NODE]).translate(*STEP).store(scene.nodes[NODE])
        scene.update()

    # where the shadow has been (tools/temporal_split_rate.py): per earlier pose the direct component at 256 spp, its darkest value per pixel; a
    # pixel counts as static when its feature position (same seed, same jitter) is the last pose's in every pose
    s = open_scene(fray_amd, "cornell_box.fray", w, h, wantAA=0, numPaths=pose_spp)
    s.beginRender()
    lum = lambda c: c.astype(np.float64).mean(axis=2)
    darkest, positions = None, []
    for k in range(a.frames):
        if k:
            move(s)
        positions.append(s.render_features(4, seed=1)[..., 0:3])
        if k < a.frames - 1:
            d, _, _ = s.render_components(pose_spp, seed=99)
            darkest = lum(d) if darkest is None else np.minimum(darkest, lum(d))
    s.settings.numPaths = truth_spp
    s.beginFrame()
    d, i, _ = s.render_components(truth_spp, seed=99)
    s.close()
    static = np.all([np.abs(P - positions[-1]).max(axis=2) < 1e-3 for P in positions], axis=0)
    mask = (lum(d) - darkest > a.lit) & static
    truth = d + i
    # where some move changed the direct light, exactly: a split run whose change frames are the pixels' own differences
    s = open_scene(fray_amd, "cornell_box.fray", w, h, **over)
    s.beginRender()
    cam = abi.Camera.from_buffer_copy(s.camera)
    changed = np.zeros((h, w), bool)
    for out, raw, info in s.render_sequence([cam] * a.frames, seed=21, edit=lambda _k, scene: move(scene), split=True, change_samples=PROBE,
                                            change=dict(radius=0)):
        if info["change_direct"] is not None:
            changed |= (info["change_direct"] > 0).cpu().numpy()
    s.close()
    changed &= static
    res = {"library": os.path.relpath(fray_amd.render_info()["library"], ROOT), "size": [w, h], "frames": a.frames, "repeats": a.repeats, "spp": spp,
           "truth_spp": truth_spp, "pose_spp": pose_spp, "node": NODE, "step": STEP, "lit_threshold": a.lit, "mask_pixels": int(mask.sum()), "changed_pixels": int(changed.sum()),
           "change_samples": PROBE}
    runs = (("plain", dict()), ("change", dict(change_samples=PROBE)), ("split", dict(split=True)), ("split_change", dict(split=True, change_samples=PROBE)))
    times = {name: [[] for _ in range(a.frames)] for name, _ in runs}
    last = {}
    for rep in range(a.repeats + 1):                      # the first repeat warms up
        for name, kw in runs:
            s = open_scene(fray_amd, "cornell_box.fray", w, h, **over)
            s.beginRender()
            cam = abi.Camera.from_buffer_copy(s.camera)
            gen = s.render_sequence([cam] * a.frames, seed=21, edit=lambda _k, scene: move(scene), **kw)
            for k in range(a.frames):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out, raw, info = next(gen)
                torch.cuda.synchronize()
                if rep:
                    times[name][k].append((time.perf_counter() - t0) * 1e3)
            gen.close()
            s.close()
            last[name] = (out.cpu().numpy(), info)
    for name, _ in runs:
        out, info = last[name]
        err = np.abs(out.astype(np.float64) - truth)
        row = {"mae_footprint": float(err[mask].mean()), "mae_changed": float(err[changed].mean()), "mae_frame": float(err.mean()),
               "frame_ms": [round(statistics.median(t), 3) for t in times[name]]}
        for key in ("change", "change_direct", "change_indirect"):
            if info.get(key) is not None:
                row[key + "_share_last_frame"] = float((info[key] > 0).float().mean())
        res[name] = row
        print(name, json.dumps(row), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plain-only", action="store_true", help="timing: only the two existing entries (runs in a checkout without change frames)")
    ap.add_argument("--sequence", action="store_true")
    ap.add_argument("--split", action="store_true", help="timing of the fused adaptive split entry against the unfused step it replaces")
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=[320, 240], metavar=("W", "H"), help="--sequence: the frame's size")
    ap.add_argument("--spp", type=int, default=4, help="--sequence: the frames' samples per pixel")
    ap.add_argument("--lit", type=float, default=0.05, help="--sequence: how much brighter than at its darkest earlier pose the direct light must be (mean of r, g, b)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds must be >= 20: the record is a median")
    if a.frames < 2 or a.repeats < 1:
        ap.error("--frames must be >= 2 and --repeats >= 1")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import fray_amd
    from fray_amd import abi
    from conftest import open_scene
    fray_amd.lib.frayhip_init(0)
    res = (sequence if a.sequence else split_timing if a.split else timing)(a, fray_amd, abi, open_scene)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
