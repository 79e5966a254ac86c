"""The headline frame (cornell_box.fray 1920x1080 x 64 spp, path traced) through frayhip_render_device, and through
frayhip_render_device_progressive with a progress callback and no previews (preview_ms -1) and with a preview after every batch
(preview_ms 0): the same scene, the same stream, the three calls alternating round after round.  Prints one JSON line of medians.

    python tools/progressive_overhead.py [--rounds 15] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    import torch
    import fray_amd
    s = fray_amd.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    s.settings.frameWidth, s.settings.frameHeight, s.settings.numPaths = a.width, a.height, a.spp
    s.beginRender(0)
    frame = torch.zeros((a.height, a.width, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    calls = []
    variants = {
        "blocking": lambda: s.render_device(frame.data_ptr(), stream=stream.cuda_stream),
        "progress_only": lambda: s.render_device(frame.data_ptr(), stream=stream.cuda_stream, progress=lambda i: calls.append(i["samples_done"]), preview_ms=-1),
        "preview_every_batch": lambda: s.render_device(frame.data_ptr(), stream=stream.cuda_stream, progress=lambda i: calls.append(i["samples_done"]), preview_ms=0),
    }
    times = {k: [] for k in variants}
    frames = {}
    for r in range(a.warmup + a.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            if r == 0:
                frames[k] = frame.cpu().clone()
    same = all(torch.equal(frames["blocking"], f) for f in frames.values())
    out = {"frame": "cornell_box %dx%d x %d spp" % (a.width, a.height, a.spp), "rounds": a.rounds, "bit_identical": same}
    for k, v in times.items():
        out[k + "_ms_median"] = round(statistics.median(v), 3)
        out[k + "_ms_min"] = round(min(v), 3)
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
