"""Split temporal accumulation on one GPU (include/frayhip.h "split temporal accumulation"), two records for profiles/temporal_split/README.md.

1. Timing, 1920x1080, cornell_box components (4 spp) and features: frayhip_temporal_accumulate_split_device against the two
   frayhip_temporal_accumulate[_motion]_device calls it replaces, on the same inputs.  The fused call and the pair ALTERNATE in one loop of one
   process (a drifting clock or a busy neighbour hits both alike), --warmup rounds first, then the median of --rounds rounds each.  Times are the
   library's own (frayhip_stats.ms_kernels: HIP events around each call's kernels; the pair's time is the sum of its two calls; call_ms is the
   wall time of the call or calls).  Four rows: with and without a motion frame, at frame 0 (no history: every pixel takes the 7x7 window, for
   both components) and in steady state (a history four frames deep under a still camera; young_share is the share of pixels that still take
   the window: with the motion frame, frame 1's, whose short block has moved).  Both components use the defaults, so that the pair's second
   call does the same work as its first.
2. --shadow: a moving shadow, 320x240: cornell_box's short block (node 5) translated per frame for --frames frames at 4 spp, as
   render_sequence(edit=...) renders it unsplit, split with the direct history's default length, and split with direct max_history 32.  The
   error is the mean absolute difference, per channel, of the last frame's picture from a 1024-spp frame of the last pose, over the shadow's
   previous footprint: the pixels that show the same static surface point in every pose and whose direct light at the last pose (1024 spp)
   is brighter by more than --lit than the darkest it was at any earlier pose (256 spp each).

    python tools/temporal_split_rate.py [--rounds 21] [--warmup 3] [--out FILE]
    python tools/temporal_split_rate.py --shadow [--frames 16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
NODE, STEP = 5, (8.0, 0.0, -4.0)


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
    frames = []
    with torch.cuda.stream(stream):
        for k in range(2):
            prev = s.node_transforms()
            if k:
                fray_amd.Transform(s.nodes[NODE]).translate(*STEP).store(s.nodes[NODE])
                s.update()
            feat, motion = new(H, W, 10), new(H, W, 8)
            fr = abi.Frame(mode=abi.MODE_RENDER, seed=42 + k)
            assert L.frayhip_render_features_motion_device(s._dev, C.byref(fr), 4, prev, len(prev), feat.data_ptr(), motion.data_ptr(), h, None) == 0
            state = tuple(fray_amd.Accumulation.empty((W, H), 42 + k, device="cuda") for _ in range(2))
            d, i, _ = s.render_components(4, state, seed=42 + k, stream=stream)
            frames.append((d, i, feat, motion))
    s.close()
    pd, pi = fray_amd.temporal_params(), fray_amd.temporal_params()
    with torch.cuda.stream(stream):
        out = dict(hs=new(H, W, 20), hd=new(H, W, 12), hi=new(H, W, 12), sd=new(H, W, 3), si=new(H, W, 3), vd=new(H, W), vi=new(H, W))

    def fused(frame, motion, hin, hout=None):
        d, i, feat, mot = frames[frame]
        st = abi.Stats()
        rc = L.frayhip_temporal_accumulate_split_device(W, H, d.data_ptr(), i.data_ptr(), feat.data_ptr(), mot.data_ptr() if motion else None,
                                                        C.byref(view) if hin is not None else None, hin.data_ptr() if hin is not None else None,
                                                        C.byref(pd), C.byref(pi), (hout if hout is not None else out["hs"]).data_ptr(),
                                                        out["sd"].data_ptr(), out["si"].data_ptr(), out["vd"].data_ptr(), out["vi"].data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st.ms_kernels

    def one(rgb, frame, motion, hin, hout, sig, var, p):
        _, _, feat, mot = frames[frame]
        st = abi.Stats()
        vp, hp = (C.byref(view), hin.data_ptr()) if hin is not None else (None, None)
        if motion:
            rc = L.frayhip_temporal_accumulate_motion_device(W, H, rgb.data_ptr(), feat.data_ptr(), mot.data_ptr(), vp, hp, C.byref(p), hout.data_ptr(),
                                                             sig.data_ptr(), var.data_ptr(), h, C.byref(st))
        else:
            rc = L.frayhip_temporal_accumulate_device(W, H, rgb.data_ptr(), feat.data_ptr(), vp, hp, C.byref(p), hout.data_ptr(), sig.data_ptr(),
                                                      var.data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st.ms_kernels

    def pair(frame, motion, hin, hout=None):
        hd, hi = hin if hin is not None else (None, None)
        od, oi = hout if hout is not None else (out["hd"], out["hi"])
        return (one(frames[frame][0], frame, motion, hd, od, out["sd"], out["vd"], pd) +
                one(frames[frame][1], frame, motion, hi, oi, out["si"], out["vi"], pi))

    # the steady-state history: frame 0 accumulated onto itself under the still camera until N = 4 everywhere it can be
    hs = [new(H, W, 20), new(H, W, 20)]
    hp = [(new(H, W, 12), new(H, W, 12)), (new(H, W, 12), new(H, W, 12))]
    fused(0, False, None, hs[0])
    pair(0, False, None, hp[0])
    for k in range(3):
        fused(0, False, hs[k % 2], hs[(k + 1) % 2])
        pair(0, False, hp[k % 2], hp[(k + 1) % 2])
    steady_s, steady_p = hs[1], hp[1]
    young = float((steady_s[..., 15] < 4).float().mean())
    parts = fray_amd.split_history_parts(steady_s)
    assert torch.equal(parts[0].view(torch.int32), steady_p[0].view(torch.int32)) and torch.equal(parts[1].view(torch.int32), steady_p[1].view(torch.int32))

    res = {"library": os.path.relpath(fray_amd.render_info()["library"], ROOT), "size": [W, H], "rounds": a.rounds, "warmup": a.warmup, "steady_young_share": young}
    for name, frame, motion, hin_s, hin_p in (("frame0", 0, False, None, None), ("frame0_motion", 0, True, None, None),
                                              ("steady", 0, False, steady_s, steady_p), ("steady_motion", 1, True, steady_s, steady_p)):
        f, p, fc, pc = [], [], [], []
        for r in range(a.warmup + a.rounds):
            t0 = time.perf_counter()
            x = fused(frame, motion, hin_s)
            t1 = time.perf_counter()
            y = pair(frame, motion, hin_p)
            t2 = time.perf_counter()
            if r >= a.warmup:
                f.append(x)
                p.append(y)
                fc.append((t1 - t0) * 1e3)
                pc.append((t2 - t1) * 1e3)
        med = statistics.median
        res[name] = {"fused_ms": med(f), "pair_ms": med(p), "ratio": med(f) / med(p), "fused_min_max": [min(f), max(f)], "pair_min_max": [min(p), max(p)],
                     "fused_call_ms": med(fc), "pair_call_ms": med(pc), "young_share": float((out["hs"][..., 15] < 4).float().mean())}
        print(name, json.dumps(res[name]), flush=True)
    return res


def shadow(a, fray_amd, abi, open_scene):
    import numpy as np
    w, h, spp, pose_spp, truth_spp = 320, 240, 4, 256, 1024
    over = dict(wantAA=0, numPaths=spp)

    def move(scene):
        fray_amd.Transform(scene.nodes[NODE]).translate(*STEP).store(scene.nodes[NODE])
        scene.update()

    # where the shadow has been: per earlier pose the direct component at 256 spp, its darkest value per pixel; a pixel counts as static when
    # its feature position (same seed, same jitter) is the last pose's in every pose
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
    res = {"library": os.path.relpath(fray_amd.render_info()["library"], ROOT), "size": [w, h], "frames": a.frames, "spp": spp, "truth_spp": truth_spp, "pose_spp": pose_spp, "node": NODE, "step": STEP,
           "lit_threshold": a.lit, "mask_pixels": int(mask.sum())}
    runs = (("unsplit", dict()), ("split_direct_8", dict(split=True)), ("split_direct_32", dict(split=True, temporal_direct=dict(max_history=32))))
    for name, kw in runs:
        s = open_scene(fray_amd, "cornell_box.fray", w, h, **over)
        s.beginRender()
        cam = abi.Camera.from_buffer_copy(s.camera)
        for out, raw, info in s.render_sequence([cam] * a.frames, seed=21, edit=lambda _k, scene: move(scene), **kw):
            pass
        s.close()
        err = np.abs(out.cpu().numpy().astype(np.float64) - truth)
        res[name] = {"mae_footprint": float(err[mask].mean()), "mae_frame": float(err.mean())}
        print(name, json.dumps(res[name]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shadow", action="store_true")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--lit", type=float, default=0.05, help="--shadow: how much brighter than at its darkest earlier pose the direct light must be (mean of r, g, b)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds must be >= 20: the record is a median")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import fray_amd
    from fray_amd import abi
    from conftest import open_scene
    fray_amd.lib.frayhip_init(0)
    res = (shadow if a.shadow else timing)(a, fray_amd, abi, open_scene)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
