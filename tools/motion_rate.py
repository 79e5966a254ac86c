"""Motion frames on one GPU (include/frayhip.h "motion frames"): what the motion output costs the feature pass, and what reprojecting through
it costs the temporal stage, at 1920x1080.  Times are the library's own (frayhip_stats.ms_kernels: HIP events around the call's device work;
ms_total: the call's wall time, which also holds the motion entry's host work -- comparing the transforms, filling and uploading the table),
medians over --rounds rounds after --warmup, every call on one torch stream with all buffers resident on the device.

  features_<scene>            frayhip_render_features_device: cornell_box (4 spp, n = 4) and hw9/dragon (a Whitted frame, n = 1)
  features_motion_<scene>_still    frayhip_render_features_motion_device with prev_T = the nodes' transforms: no lane reads the table
  features_<scene>_after_move      frayhip_render_features_device on the edited scene: what the next row is to be held against (the moved
                                   node covers other pixels and is no longer an untransformed one)
  features_motion_<scene>_moved    frayhip_render_features_motion_device after one node was translated (cornell_box: node 5, the short block; dragon: node 1, the dragon)
  accumulate                  frayhip_temporal_accumulate_device, frame 1 onto frame 0's history, variance_history 1: k_tp_accumulate alone
  accumulate_motion           frayhip_temporal_accumulate_motion_device on the same inputs and frame 1's motion frame (one node moved)

A library without the motion entries (an earlier checkout, --package) gives only the rows that need no motion entry (features_<scene>, features_<scene>_after_move, accumulate).

    python tools/motion_rate.py [--rounds 7] [--warmup 2] [--package DIR] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = (("cornell", "cornell_box.fray", dict(wantAA=0, numPaths=4), 4, 5, (8.0, 0.0, -4.0)),
          ("dragon", "hw9/dragon.fray", dict(wantAA=0), 1, 1, (0.5, 0.0, -0.25)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--package", default=ROOT, help="the directory to import fray_amd from (default: this checkout)")
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.package))
    import ctypes as C
    import torch
    import fray_amd
    from fray_amd import abi
    from conftest import open_scene

    L = fray_amd.lib
    L.frayhip_init(0)
    has_motion = hasattr(abi, "MOTION_CHANNELS")
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    res = {"library": fray_amd.render_info()["library"], "motion_entries": has_motion}

    def timed(call):
        ks, calls = [], []
        for r in range(a.warmup + a.rounds):
            st = call()
            if r >= a.warmup:
                ks.append(st.ms_kernels)
                calls.append(st.ms_total)
        return {"kernels_ms": statistics.median(ks), "min_ms": min(ks), "max_ms": max(ks), "call_ms": statistics.median(calls)}

    kept = {}
    for key, name, over, n, node, d in SCENES:
        s = open_scene(fray_amd, name, W, H, **over)
        s.beginRender()
        fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
        with torch.cuda.stream(stream):
            feat, motion, rgb = new(H, W, 10), new(H, W, 8), new(H, W, 3)

        def features():
            st = abi.Stats()
            assert L.frayhip_render_features_device(s._dev, C.byref(fr), n, feat.data_ptr(), h, C.byref(st)) == 0, L.frayhip_last_error()
            return st

        def features_motion(prev):
            st = abi.Stats()
            rc = L.frayhip_render_features_motion_device(s._dev, C.byref(fr), n, prev, len(prev), feat.data_ptr(), motion.data_ptr(), h, C.byref(st))
            assert rc == 0, L.frayhip_last_error()
            return st

        res["features_" + key] = timed(features)
        if has_motion:
            res["features_motion_%s_still" % key] = timed(lambda: features_motion(s.node_transforms()))
        if key == "cornell":
            # frame 0 of the temporal rows: the scene as loaded
            s.render_device(rgb.data_ptr(), seed=42, stream=h)
            features()
            kept["frame0"] = (rgb.clone(), feat.clone(), fray_amd.view_from_camera(s.camera, W, H))
        prev = [abi.Transform.from_buffer_copy(nd.T) for nd in s.nodes]
        fray_amd.Transform(s.nodes[node]).translate(*d).store(s.nodes[node])
        s.update()
        res["features_%s_after_move" % key] = timed(features)
        if has_motion:
            prev_T = (abi.Transform * len(prev))(*prev)
            res["features_motion_%s_moved" % key] = timed(lambda: features_motion(prev_T))
            res["features_motion_%s_moved" % key]["moved_pixels"] = int((motion[..., 3] > 0).sum())
        if key == "cornell":
            fr1 = abi.Frame(mode=abi.MODE_RENDER, seed=43)
            s.render_device(rgb.data_ptr(), seed=43, stream=h)
            if has_motion:
                assert L.frayhip_render_features_motion_device(s._dev, C.byref(fr1), n, prev_T, len(prev), feat.data_ptr(), motion.data_ptr(), h, None) == 0
            else:
                assert L.frayhip_render_features_device(s._dev, C.byref(fr1), n, feat.data_ptr(), h, None) == 0
            kept["frame1"] = (rgb.clone(), feat.clone(), motion.clone())
        s.close()
    torch.cuda.synchronize()

    rgb0, feat0, view0 = kept["frame0"]
    rgb1, feat1, motion1 = kept["frame1"]
    with torch.cuda.stream(stream):
        hist0, hist1, signal, variance = new(H, W, 12), new(H, W, 12), new(H, W, 3), new(H, W)
    p = fray_amd.temporal_params(variance_history=1)
    assert L.frayhip_temporal_accumulate_device(W, H, rgb0.data_ptr(), feat0.data_ptr(), None, None, C.byref(p), hist0.data_ptr(), signal.data_ptr(),
                                                variance.data_ptr(), h, None) == 0, L.frayhip_last_error()

    def accumulate():
        st = abi.Stats()
        rc = L.frayhip_temporal_accumulate_device(W, H, rgb1.data_ptr(), feat1.data_ptr(), C.byref(view0), hist0.data_ptr(), C.byref(p), hist1.data_ptr(),
                                                  signal.data_ptr(), variance.data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st

    def accumulate_motion():
        st = abi.Stats()
        rc = L.frayhip_temporal_accumulate_motion_device(W, H, rgb1.data_ptr(), feat1.data_ptr(), motion1.data_ptr(), C.byref(view0), hist0.data_ptr(),
                                                         C.byref(p), hist1.data_ptr(), signal.data_ptr(), variance.data_ptr(), h, C.byref(st))
        assert rc == 0, L.frayhip_last_error()
        return st

    res["accumulate"] = timed(accumulate)
    mv = motion1[..., 3] == 1 if has_motion else None
    if has_motion:
        res["accumulate"]["moved_pixels_with_history"] = float((hist1[..., 3][mv] > 1).float().mean())
        res["accumulate_motion"] = timed(accumulate_motion)
        res["accumulate_motion"]["moved_pixels_with_history"] = float((hist1[..., 3][mv] > 1).float().mean())

    for k, v in res.items():
        print(k, json.dumps(v), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
