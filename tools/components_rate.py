"""Component frames on one GPU (include/frayhip.h "component frames"): what keeping direct and indirect light apart costs, from the library's own
timings (frayhip_stats.ms_kernels: HIP events around the call's device work; ms_total: the call's wall time).  cornell_box 1920x1080, 64 spp, wantAA
off; every call on one torch stream, every buffer resident on the device; the two calls alternate round after round in one process, medians
over --rounds rounds after --warmup.

  samples      one frayhip_render_samples_device call of 64 samples, rgb and noise asked for
  components   one frayhip_render_components_device call of the same 64 samples, both rgb and both noise buffers asked for

The traced work is the same.  Per pixel and batch the split resolve reads two 16-byte rows (not when the batch begins at sample 0) and writes two
where the other reads and writes one, and k_acc_mean runs once more per call (16 bytes in, 12 + 4 out).  The tool prints those bytes for the
frame as it was batched, what they cost at the device-to-device copy rate it measures, and the measured difference to compare them with.

--quality adds a record that no test asserts: Scene.render_denoised_split and Scene.render_denoised of cornell_box 96x72 at 12 spp, both as RMS
against a --ref-spp frame of the same view.

    python tools/components_rate.py [--rounds 7] [--warmup 2] [--quality] [--ref-spp 4096] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, SPP = 1920, 1080, 64
QW, QH, QSPP = 96, 72, 12


def med(v):
    return {"kernels_ms": statistics.median(x[0] for x in v), "call_ms": statistics.median(x[1] for x in v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quality", action="store_true", help="also: render_denoised_split and render_denoised of a 96x72, 12-spp frame against a --ref-spp frame")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import fray_amd
    from conftest import open_scene
    abi, lib = fray_amd.abi, fray_amd.lib

    lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    s = open_scene(fray_amd, "cornell_box.fray", W, H, gi=1, numPaths=SPP, wantAA=0)
    s.beginRender()
    with torch.cuda.stream(stream):
        acc = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        rgb = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
        noise = [torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()

    # the entries themselves, without the counting flag (the Scene methods return timings only with stats=True, which selects the counting variants)
    def request():
        return (abi.Frame(mode=abi.MODE_RENDER, seed=42, bucket_first=0, bucket_stride=1, spp_chunk=0, flags=0), abi.Samples(sample_first=0, sample_count=SPP),
                abi.Stats())

    def samples():
        fr, req, st = request()
        rc = lib.frayhip_render_samples_device(s._dev, C.byref(fr), C.byref(req), None, acc[0].data_ptr(), rgb[0].data_ptr(), noise[0].data_ptr(), h, C.byref(st))
        if rc:
            sys.exit("frayhip_render_samples_device: %s" % lib.frayhip_last_error().decode())
        return st.ms_kernels, st.ms_total

    def components():
        fr, req, st = request()
        rc = lib.frayhip_render_components_device(s._dev, C.byref(fr), C.byref(req), None, acc[0].data_ptr(), acc[1].data_ptr(), rgb[0].data_ptr(),
                                                  rgb[1].data_ptr(), noise[0].data_ptr(), noise[1].data_ptr(), h, C.byref(st))
        if rc:
            sys.exit("frayhip_render_components_device: %s" % lib.frayhip_last_error().decode())
        return st.ms_kernels, st.ms_total

    calls = [("samples", samples), ("components", components)]
    times = {k: [] for k, _ in calls}
    for r in range(a.warmup + a.rounds):
        for k, fn in calls:
            v = fn()
            if r >= a.warmup:
                times[k].append(v)
    res = {k: med(v) for k, v in times.items()}
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
    extra = (batches - 1) * 16 + batches * 16 + (16 + 12 + 4)                      # the second state's rows in and out, and its k_acc_mean
    res["resolve"] = {"batches": batches, "copy_GBps": copy_gbs, "extra_bytes_per_pixel": extra,
                      "extra_ms_at_copy_rate": extra * W * H / (copy_gbs * 1e9) * 1e3,
                      "measured_extra_kernels_ms": res["components"]["kernels_ms"] - res["samples"]["kernels_ms"],
                      "measured_extra_call_ms": res["components"]["call_ms"] - res["samples"]["call_ms"]}
    for k, _ in calls:
        print("%-11s kernels %8.2f ms  call %8.2f ms" % (k, res[k]["kernels_ms"], res[k]["call_ms"]), flush=True)
    print("resolve:", json.dumps(res["resolve"]))
    s.close()
    if a.quality:
        import numpy as np
        q = open_scene(fray_amd, "cornell_box.fray", QW, QH, gi=1, numPaths=a.ref_spp, wantAA=0)
        q.beginRender()
        ref, _ = q.render(seed=42)
        ref = ref.astype(np.float64)
        rms = lambda img: float(np.sqrt(((np.asarray(img, np.float64) - ref) ** 2).mean()))
        q.settings.numPaths = QSPP
        q.beginFrame()
        den, raw, _ = q.render_denoised(seed=42)
        split, raw_sum, info = q.render_denoised_split(seed=42)
        res["quality"] = {"size": [QW, QH], "spp": QSPP, "ref_spp": a.ref_spp, "rms_raw": rms(raw), "rms_raw_sum_of_components": rms(raw_sum),
                          "rms_render_denoised": rms(den), "rms_render_denoised_split": rms(split), "rms_direct_filtered_plus_indirect_raw": rms(info["direct"] + info["indirect_rgb"]),
                          "noise_direct_mean": float(info["noise_direct"].mean()), "noise_indirect_mean": float(info["noise_indirect"].mean())}
        print("quality:", json.dumps(res["quality"]))
        q.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
