"""Specular feature frames on one GPU (include/frayhip.h "specular feature frames"): what following mirrors and glass costs at 1080p, and what
the virtual-hit guides change in a denoised frame and in a short yawing sequence.  Times are the library's own (frayhip_stats.ms_kernels: HIP
events around the call's device work), medians over --rounds rounds after --warmup, the entries called in turn within every round (first-hit,
K = 1, 4, 8, first-hit, ...) on one torch stream with the outputs resident on the device.

  time_<scene>          frayhip_render_features_device and frayhip_render_features_specular_device (K = 1, 4, 8) at 1920x1080, n_samples 4, on the
                        scene's path-traced frame; the share of pixels that took a step and the mean steps per sample at K = 8
  first_hit_<scene>     with --baseline-root DIR (another built checkout of the project, e.g. the parent commit's): frayhip_render_features_device
                        of that checkout and of this one, each in a fresh child process, --alternations times in turn
  benefit_<scene>       at --size, --spp samples: render_denoised and the last frame of an 8-frame render_sequence yawing by --yaw-step degrees per
                        frame, with first-hit guides (specular=0) and with specular=4, each against a --ref-spp frame of the same view: relative
                        MSE (mean squared error / mean squared reference) over the pixels whose bounces plane is > 0 and over the rest

    python tools/specular_features_rate.py [--rounds 7] [--warmup 2] [--ref-spp 1024] [--baseline-root DIR] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SCENES = ("cornell_box.fray", "smallpt.fray")
KS = (1, 4, 8)


def med(xs):
    return statistics.median(xs)


def open_scene(fray, root, name, w, h, **over):
    s = fray.Scene.parseScene(os.path.join(root, "scenes", name))
    s.settings.frameWidth, s.settings.frameHeight = w, h
    for k, v in over.items():
        setattr(s.settings if hasattr(s.settings, k) else s.camera, k, v)
    return s


def first_hit_only(a):
    """frayhip_render_features_device of the package under a.import_root: one JSON line {scene: median ms}"""
    sys.path.insert(0, a.import_root)
    import ctypes as C
    import torch
    import fray_amd
    from fray_amd import abi
    assert os.path.dirname(os.path.dirname(os.path.abspath(fray_amd.__file__))) == os.path.abspath(a.import_root)
    fray_amd.lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        feat = torch.empty((H, W, 10), dtype=torch.float32, device="cuda")
    res = {}
    for name in SCENES:
        s = open_scene(fray_amd, ROOT, name, W, H, gi=1, numPaths=8)
        s.beginRender()
        ts = []
        for r in range(a.warmup + a.rounds):
            st = abi.Stats()
            fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
            assert fray_amd.lib.frayhip_render_features_device(s._dev, C.byref(fr), 4, feat.data_ptr(), stream.cuda_stream, C.byref(st)) == 0
            if r >= a.warmup:
                ts.append(st.ms_kernels)
        res[name.split(".")[0]] = med(ts)
        s.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(320, 240), metavar=("W", "H"))
    ap.add_argument("--yaw-step", type=float, default=1.0)
    ap.add_argument("--baseline-root", help="another built checkout whose frayhip_render_features_device is timed beside this one's")
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--first-hit-only", action="store_true", help="(the child process of --baseline-root)")
    ap.add_argument("--import-root", default=ROOT)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.first_hit_only:
        return first_hit_only(a)
    res = {}

    # ---- frayhip_render_features of another checkout against this one's: child processes, started before this process opens the GPU ----
    if a.baseline_root:
        runs = {"baseline": [], "this": []}
        for _ in range(a.alternations):
            for tag, root in (("baseline", os.path.abspath(a.baseline_root)), ("this", ROOT)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-hit-only", "--import-root", root, "--rounds", str(a.rounds),
                                      "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600, cwd=root)
                assert out.returncode == 0, out.stderr[-2000:]
                runs[tag].append(json.loads(out.stdout.strip().splitlines()[-1]))
        for name in SCENES:
            t = name.split(".")[0]
            base, this = [r[t] for r in runs["baseline"]], [r[t] for r in runs["this"]]
            res["first_hit_%s" % t] = {"baseline_ms": base, "this_ms": this, "ratio_of_medians": med(this) / med(base)}

    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import fray_amd
    from fray_amd import abi
    from fray_amd.__main__ import orbit

    fray_amd.lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    with torch.cuda.stream(stream):
        feat_t = torch.empty((H, W, 10), dtype=torch.float32, device="cuda")
        plane_t = torch.empty((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    # ---- time ----
    for name in SCENES:
        s = open_scene(fray_amd, ROOT, name, W, H, gi=1, numPaths=8)
        s.beginRender()
        ts = {k: [] for k in (0,) + KS}
        for r in range(a.warmup + a.rounds):
            for k in (0,) + KS:
                st = abi.Stats()
                fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
                if k == 0:
                    rc = fray_amd.lib.frayhip_render_features_device(s._dev, C.byref(fr), 4, feat_t.data_ptr(), h, C.byref(st))
                else:
                    rc = fray_amd.lib.frayhip_render_features_specular_device(s._dev, C.byref(fr), 4, k, feat_t.data_ptr(), plane_t.data_ptr(), h,
                                                                              C.byref(st))
                assert rc == 0, fray_amd.lib.frayhip_last_error()
                if r >= a.warmup:
                    ts[k].append(st.ms_kernels)
        torch.cuda.synchronize()
        plane = plane_t.cpu().numpy()                                   # K = 8's, the last call
        row = {"first_hit_ms": med(ts[0]), "share_of_pixels_with_a_step": float((plane > 0).mean()), "mean_steps_per_sample_K8": float(plane.mean())}
        for k in KS:
            row["specular_K%d_ms" % k] = med(ts[k])
            row["ratio_K%d" % k] = med(ts[k]) / med(ts[0])
        res["time_%s" % name.split(".")[0]] = row
        s.close()

    # ---- benefit ----
    w, hgt = a.size
    for name in SCENES:
        s = open_scene(fray_amd, ROOT, name, w, hgt, gi=1, numPaths=a.spp)
        s.beginRender()
        start = abi.Camera.from_buffer_copy(s.camera)
        cams = list(orbit(start, 8, a.yaw_step))

        def reference(cam):
            C.memmove(C.byref(s.desc.camera), C.byref(cam), C.sizeof(abi.Camera))
            s.settings.numPaths = a.ref_spp
            s.beginFrame()
            ref, _ = s.render(seed=4242)
            _, plane = s.render_features_specular(4, 4, seed=42, bounces=True)
            s.settings.numPaths = a.spp
            C.memmove(C.byref(s.desc.camera), C.byref(start), C.sizeof(abi.Camera))
            s.beginFrame()
            return ref.astype(np.float64), plane > 0

        def rel_mse(img, ref, mask):
            return float(((img.astype(np.float64) - ref) ** 2)[mask].mean() / (ref ** 2)[mask].mean()) if mask.any() else None

        row = {}
        ref0, m0 = reference(cams[0])
        ref7, m7 = reference(cams[-1])
        row["share_of_pixels_with_a_step"] = float(m0.mean())
        for k in (0, 4):
            den, raw, _ = s.render_denoised(seed=42, feature_samples=4, specular=k)
            last = None
            for out, _raw, _info in s.render_sequence(cams, seed=42, feature_samples=4, specular=k):
                last = out.cpu().numpy()
            tag = "specular4" if k else "first_hit"
            row["denoised_%s" % tag] = {"rel_mse_specular_pixels": rel_mse(den, ref0, m0), "rel_mse_other_pixels": rel_mse(den, ref0, ~m0)}
            row["sequence_frame7_%s" % tag] = {"rel_mse_specular_pixels": rel_mse(last, ref7, m7), "rel_mse_other_pixels": rel_mse(last, ref7, ~m7)}
            if k == 0:
                row["raw"] = {"rel_mse_specular_pixels": rel_mse(raw, ref0, m0), "rel_mse_other_pixels": rel_mse(raw, ref0, ~m0)}
        res["benefit_%s" % name.split(".")[0]] = row
        s.close()

    for k, v in res.items():
        print(k, json.dumps(v), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
