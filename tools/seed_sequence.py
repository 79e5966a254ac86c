"""The seed table's two cases outside bench.py: the headline frame (cornell_box.fray 1920x1080 x 64 spp, path traced) rendered --frames times
through one scene handle, frame k with seed 42 + k (the way Scene.render_sequence seeds its frames: every frame misses the table and refills
it) or, with --fixed, with seed 42 every time (every frame after the first finds its seeds in the table).  Prints one JSON line: ms per frame
(median, min, max over the frames after --warmup) and, where the library has them, the k_seed launches and reused planes of the last frame.

    python tools/seed_sequence.py [--fixed] [--label NAME] [--frames 20] [--warmup 3]        (FRAYHIP_LIB selects another build of the library)"""
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
    ap.add_argument("--fixed", action="store_true", help="seed 42 for every frame instead of 42 + k")
    ap.add_argument("--label", default="this tree", help="what the line calls the library that rendered (e.g. parent)")
    ap.add_argument("--frames", type=int, default=20)
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
    times = []
    for k in range(a.warmup + a.frames):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.render_device(frame.data_ptr(), seed=42 if a.fixed else 42 + k, stream=stream.cuda_stream)
        torch.cuda.synchronize()
        if k >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    out = {"frame": "cornell_box %dx%d x %d spp" % (a.width, a.height, a.spp), "seeds": "42" if a.fixed else "42 + k", "frames": a.frames,
           "library": a.label,
           "ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}
    try:
        out.update(seed_launches_last_frame=s.get_option("seed_launches"), seed_planes_reused_last_frame=s.get_option("seed_planes_reused"),
                   seed_table_bytes=s.get_option("seed_table_bytes"))
    except fray_amd.FrayError:
        pass                                  # a library from before the table
    s.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
