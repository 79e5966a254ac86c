"""Scene edits on one GPU (include/frayhip.h "scene edits"): what it costs to show an edited scene, two ways, on the same tree and the same box.

  update     frayhip_scene_update of the edited description on the handle that is already there (Scene.update)
  recreate   frayhip_scene_destroy + frayhip_scene_create of the same edited description (Scene.beginRender): the only way to edit before
             frayhip_scene_update existed, and code this change does not touch -- the baseline

and after each, the first frame (the scene file's integrator, its size and samples; wall time of the call and the library's ms_kernels): a
re-created handle has lost its workspace, its lane streams' scratch arenas and its seed table, an updated one has not.  The edit is a translation
of node --node by a step that alternates in sign, so every round edits, and both ways see the same descriptions.  Wall times are
time.perf_counter around the Python call; medians over --rounds rounds after --warmup.  Scenes: hw9/dragon.fray and forest.fray, as shipped.

    python tools/update_rate.py [--rounds 7] [--warmup 2] [--node 0] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("hw9/dragon.fray", "forest.fray")


def measure(fray, scene, node, rounds, warmup):
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", scene))
    s.beginRender()
    s.render(seed=42)
    rows = {"update": [], "recreate": []}
    for k in range(warmup + rounds):
        for how in ("update", "recreate"):
            step = 0.25 if how == "update" else -0.25              # forth and back: no drift, and both ways upload an edited description
            fray.Transform(s.nodes[node]).translate(step, 0, 0).store(s.nodes[node])
            t0 = time.perf_counter()
            if how == "update":
                s.update()
            else:
                s.beginRender()
            t1 = time.perf_counter()
            _, st = s.render(seed=42)
            t2 = time.perf_counter()
            if k >= warmup:
                rows[how].append((1e3 * (t1 - t0), 1e3 * (t2 - t1), st["ms_kernels"]))
    out = {"scene": scene, "size": list(s.frame_size), "spp": s.samples_per_pixel(), "gi": int(s.settings.gi),
           "arena_bytes": s.get_option("arena_bytes"), "scene_update_bytes": s.get_option("scene_update_bytes") if rows["update"] else 0}
    for how, v in rows.items():
        out[how] = {"edit_ms": statistics.median(x[0] for x in v), "first_frame_ms": statistics.median(x[1] for x in v),
                    "first_frame_kernels_ms": statistics.median(x[2] for x in v)}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--node", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import fray_amd
    fray_amd.lib.frayhip_init(0)
    res = {"rounds": a.rounds, "scenes": [measure(fray_amd, sc, a.node, a.rounds, a.warmup) for sc in SCENES]}
    for r in res["scenes"]:
        print("%-16s %dx%d %d spp  arena %.1f MiB, update uploads %d bytes" % (r["scene"], r["size"][0], r["size"][1], r["spp"], r["arena_bytes"] / 2.0 ** 20, r["scene_update_bytes"]))
        for how in ("update", "recreate"):
            print("   %-9s edit %9.3f ms   first frame %9.3f ms (kernels %.3f ms)" % (how, r[how]["edit_ms"], r[how]["first_frame_ms"], r[how]["first_frame_kernels_ms"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
