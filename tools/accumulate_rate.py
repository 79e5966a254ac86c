"""Resumable frames on one GPU (include/frayhip.h "resumable frames"): what a frame costs when its sum is a caller-held state, from the library's own
timings (frayhip_stats.ms_kernels: HIP events around the call's device work; ms_total: the call's wall time).  cornell_box 1920x1080, 64 spp, wantAA
off; every call on one torch stream, every buffer resident on the device; the calls alternate round after round, medians over --rounds rounds
after --warmup.

  frame          the one-shot 64-spp frame (frayhip_render_device)
  samples_64     one frayhip_render_samples_device call of 64 samples, rgb and noise asked for
  samples_8x8    eight calls of 8 samples into one state (the sums of their ms_kernels and ms_total)
  parent_frame   `frame` once more from a checkout of the parent commit with its library built (--parent-tree DIR: the parent's Python binds the
                 parent's symbols, which this tree's cannot), measured by a child process of this tool that is started before this process
                 touches the GPU

The resolves: per pixel and batch the frame's resolve reads its 12-byte sum (not in the first batch) and writes it (the last batch writes the
12-byte pixel instead); the accumulating resolve reads the 16-byte row (not when the batch begins at sample 0) and writes it after every batch,
and k_acc_mean reads the row and writes 12 + 4 bytes once per call.  The tool prints those bytes for the frame as it was batched, what they cost at
the device-to-device copy rate it measures, and the measured differences to compare them with.

--compose adds a composition that no test asserts: the noise buffer of an 8-spp state as frayhip_denoise_signal's variance (signal = rgb,
demodulate = 0), beside Scene.render_denoised of the same 8-spp frame, both as RMS against a --ref-spp frame.

    python tools/accumulate_rate.py [--rounds 7] [--warmup 2] [--parent-tree DIR] [--compose] [--ref-spp 1024] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, SPP = 1920, 1080, 64


def med(v):
    return {"kernels_ms": statistics.median(x[0] for x in v), "call_ms": statistics.median(x[1] for x in v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-tree", metavar="DIR", help="a checkout of the parent commit with its library built: its one-shot frame is measured in a child process")
    ap.add_argument("--only-frame", action="store_true", help="measure the one-shot frame alone and print its JSON line (what the child process runs)")
    ap.add_argument("--tree", default=ROOT, help="the tree whose fray_amd package is measured (default: this one)")
    ap.add_argument("--compose", action="store_true", help="also: denoise_signal(rgb, noise, feat, demodulate=0) of an 8-spp state against a --ref-spp frame")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {}
    if a.parent_tree:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-frame", "--tree", os.path.abspath(a.parent_tree), "--rounds", str(a.rounds),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit("the parent library's run failed:\n" + r.stderr[-2000:])
        res["parent_frame"] = json.loads(r.stdout.strip().splitlines()[-1])["frame"]
    sys.path.insert(0, a.tree)
    sys.path.insert(0, os.path.join(a.tree, "tests"))
    import torch
    import fray_amd
    from conftest import open_scene

    fray_amd.lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    s = open_scene(fray_amd, "cornell_box.fray", W, H, gi=1, numPaths=SPP, wantAA=0)
    s.beginRender()
    with torch.cuda.stream(stream):
        rgb = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def frame():
        st = s.render_device(rgb.data_ptr(), seed=42, stream=h)
        return st["ms_kernels"], st["ms_total"]

    def samples_call(first, count, acc, noise, progressive=None):
        """frayhip_render_samples_device without the counting flag (Scene.render_samples returns timings only with stats=True, which selects the
        counting kernel variants): (ms_kernels, ms_total)."""
        fr = fray_amd.abi.Frame(mode=fray_amd.abi.MODE_RENDER, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, flags=0)
        req = fray_amd.abi.Samples(sample_first=first, sample_count=count)
        st = fray_amd.abi.Stats()
        rc = fray_amd.lib.frayhip_render_samples_device(s._dev, C.byref(fr), C.byref(req), progressive, acc.data_ptr(), rgb.data_ptr(), noise.data_ptr(),
                                                        h, C.byref(st))
        if rc:
            sys.exit("frayhip_render_samples_device: %s" % fray_amd.lib.frayhip_last_error().decode())
        return st.ms_kernels, st.ms_total

    with torch.cuda.stream(stream):
        acc = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        noise = torch.empty((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def samples(parts):
        def run():
            k = t = 0.0
            for i in range(parts):
                a_, b_ = samples_call(i * (SPP // parts), SPP // parts, acc, noise)
                k += a_
                t += b_
            return k, t
        return run

    calls = [("frame", frame)] if a.only_frame else [("frame", frame), ("samples_64", samples(1)), ("samples_8x8", samples(8))]
    times = {k: [] for k, _ in calls}
    for r in range(a.warmup + a.rounds):
        for k, fn in calls:
            v = fn()
            if r >= a.warmup:
                times[k].append(v)
    res.update({k: med(v) for k, v in times.items()})
    if not a.only_frame:
        # the frame's own batching (it decides how often a row is read and written), and the copy rate of this device
        seen = []
        s.render_samples(SPP, fray_amd.Accumulation.empty((W, H), device="cuda"), progress=lambda info: seen.append(info["batches_total"]), stream=stream)
        batches = seen[-1]
        with torch.cuda.stream(stream):
            src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            dst.copy_(src)
            e0.record(stream)
            for _ in range(10):
                dst.copy_(src)
            e1.record(stream)
        e1.synchronize()
        copy_gbs = 10 * 2 * src.numel() / (e0.elapsed_time(e1) * 1e-3) / 1e9          # bytes read + bytes written
        px = W * H
        frame_bytes = (batches - 1) * 12 + (batches - 1) * 12 + 12                      # sum in, sum out, the pixel
        acc_bytes = (batches - 1) * 16 + batches * 16                                   # row in, row out
        mean_bytes = 16 + 12 + 4
        res["resolve"] = {"batches": batches, "copy_GBps": copy_gbs,
                          "frame_resolve_bytes_per_pixel": frame_bytes, "acc_resolve_bytes_per_pixel": acc_bytes, "acc_mean_bytes_per_pixel": mean_bytes,
                          "extra_bytes_per_pixel_one_call": acc_bytes + mean_bytes - frame_bytes,
                          "extra_ms_at_copy_rate_one_call": (acc_bytes + mean_bytes - frame_bytes) * px / (copy_gbs * 1e9) * 1e3,
                          "measured_extra_kernels_ms_one_call": res["samples_64"]["kernels_ms"] - res["frame"]["kernels_ms"],
                          "measured_extra_kernels_ms_eight_calls": res["samples_8x8"]["kernels_ms"] - res["frame"]["kernels_ms"],
                          "measured_extra_call_ms_eight_calls": res["samples_8x8"]["call_ms"] - res["frame"]["call_ms"]}
        for k in ("frame", "samples_64", "samples_8x8", "parent_frame"):
            if k in res:
                print("%-14s kernels %8.2f ms  call %8.2f ms" % (k, res[k]["kernels_ms"], res[k]["call_ms"]), flush=True)
        print("resolve:", json.dumps(res["resolve"]))
    if a.compose and not a.only_frame:
        import numpy as np

        def set_spp(n):
            s.settings.numPaths = n
            s.beginFrame()
        set_spp(a.ref_spp)
        ref, _ = s.render(seed=42)
        ref = ref.astype(np.float64)
        rms = lambda img: float(np.sqrt(((np.asarray(img, np.float64) - ref) ** 2).mean()))
        set_spp(8)
        den, raw, _ = s.render_denoised(seed=42)
        img, state, var = s.render_samples(8, noise=True)
        assert np.array_equal(img, raw)
        feat = s.render_features(4, seed=42)
        out = fray_amd.denoise_signal(img, var, feat, demodulate=0)
        set_spp(SPP)
        res["compose"] = {"spp": 8, "ref_spp": a.ref_spp, "rms_raw": rms(raw), "rms_render_denoised": rms(den), "rms_denoise_signal_noise": rms(out),
                          "noise_mean": float(var.mean()), "noise_max": float(var.max())}
        print("compose:", json.dumps(res["compose"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    s.close()


if __name__ == "__main__":
    main()
