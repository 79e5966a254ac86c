"""File-only front end over the C ABI (the reference's main() opens an SDL window instead,
src/main.cpp:494-530):  python -m fray_amd scene.fray -o out.bmp [--width W --height H --spp N] [--progress] [--time-limit SECONDS]
                         python -m fray_amd scene.fray --probe X Y [--shade] [--width W --height H]   (one JSON line: what the camera ray through pixel X, Y hits;
                                                                                          --shade: and its colour)
                         python -m fray_amd scene.fray -o out.bmp --adaptive THRESHOLD [--min-spp N] [--adaptive-floor F]   (an adaptive frame, and one
                                                                                          JSON line: its rungs, mean spp and the share of pixels per rung)
                         python -m fray_amd scene.fray -o out.bmp --denoise [--feature-samples N] [--features-out FILE.npy]   (the frame denoised
                                                                                          with its first-hit features; --features-out alone saves them)
                         python -m fray_amd scene.fray -o out.bmp --denoise --specular-features K   (the guides follow mirrors and glass through at most K
                                                                                          steps to what they show; with --features-out and --frames too)
                         python -m fray_amd scene.fray -o out.bmp --denoise --frames N [--yaw-step DEG]   (N frames with temporal accumulation, the scene
                                                                                          file's camera turned by DEG per frame: out_0000.bmp ...)
                         python -m fray_amd scene.fray -o out.bmp --frames N --move NODE DX DY DZ [--move ...] [--denoise]   (N frames of one uploaded
                                                                                          scene, node NODE moved by (DX, DY, DZ) more in each: frame k sees it
                                                                                          at k times that; plain frames unless --denoise)
                         python -m fray_amd scene.fray -o out.bmp --denoise --frames N --move NODE DX DY DZ --motion-vectors   (the same sequence,
                                                                                          its history fetched where the moved nodes' surfaces were)
                         python -m fray_amd scene.fray -o out.bmp --accumulate FILE.npz [--spp N] [--noise-out FILE.npy] [--time-limit SECONDS]
                                                                                         (N more samples per pixel on top of the state in FILE.npz, which
                                                                                          is started when it does not exist; the picture of all of them)
                         python -m fray_amd scene.fray -o out.bmp --components-out FILE.npz [--denoise --split]   (path-traced mono frames: direct and
                                                                                         indirect light kept apart and saved with their noise estimates;
                                                                                          --denoise --split: each filtered on its own, then added)
                         python -m fray_amd scene.fray -o out.bmp --denoise --split --frames N [--yaw-step DEG] [--move ... [--motion-vectors]]
                                                                                         (the sequence with one history per light component: direct
                                                                                          light keeps a short one, where a moved shadow lives)
                         python -m fray_amd scene.fray -o out.bmp --denoise --frames N --move NODE DX DY DZ --motion-vectors --change-samples K
                                                                                         (the sequence with a probe of K samples per frame that finds
                                                                                          what the move changed in the light -- the node's shadow -- and
                                                                                          shortens the history there; with or without --split)
                         python -m fray_amd scene.fray -o out.bmp --refine TOL --max-spp N [--sample-budget N] [--accumulate FILE.npz] [--noise-out FILE.npy] [--denoise]
                                                                                         (samples spent where the frame is noisy: each pixel sampled
                                                                                          until its relative standard error is TOL or it holds N samples;
                                                                                          --denoise: the result filtered with its own noise estimate)
                         python -m fray_amd scene.fray -o out.bmp --refine TOL --max-spp N --denoise --split [--components-out FILE.npz]
                                                                                         (the same samples kept apart as direct and indirect light
                                                                                          under one map, each component filtered on its own, then added)"""
import argparse
import json
import os
import sys
import time

import numpy as np

from . import Accumulation, Scene, Transform, abi, lib


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m fray_amd")
    ap.add_argument("scene")
    ap.add_argument("-o", "--output", default="fray_0000.bmp")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--spp", type=int, help="pathsPerPixel (gi scenes) / numSamples (dof scenes)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--progress", action="store_true", help="print one line per finished batch of samples")
    ap.add_argument("--time-limit", type=float, metavar="SECONDS",
                    help="cancel the frame once this much time has passed and write what is finished (an exact frame of fewer samples per pixel)")
    ap.add_argument("--probe", type=float, nargs=2, metavar=("X", "Y"),
                    help="trace the camera ray through pixel (X, Y) and print its hit record as one JSON line (the reference's debugRayTrace); no image is written")
    ap.add_argument("--shade", action="store_true",
                    help="with --probe: also fire the scene's integrator along that ray (one sample, key floor(Y) * width + floor(X), --seed) and add its \"rgb\"")
    ap.add_argument("--adaptive", type=float, metavar="THRESHOLD",
                    help="adaptive sampling (path-traced scenes): each pixel stops at the first rung of floor(N/2), N, 2N, ... spp whose noise estimate is "
                         "<= THRESHOLD; prints one JSON line with the rungs, the mean spp and the fraction of pixels at each rung")
    ap.add_argument("--min-spp", type=int, default=16, metavar="N", help="with --adaptive: the smallest sample count a pixel stops at (default 16)")
    ap.add_argument("--adaptive-floor", type=float, default=0.01, metavar="F",
                    help="with --adaptive: the floor added to the pixel's brightness in the error's denominator (default 0.01)")
    ap.add_argument("--denoise", action="store_true",
                    help="write the frame denoised (Scene.render_denoised: first-hit features, the half-spp frame as the noise estimate, "
                         "the a-trous filter with its default parameters); not with --adaptive or --time-limit")
    ap.add_argument("--feature-samples", type=int, default=4, metavar="N",
                    help="camera samples per pixel of the feature frame (--denoise, --features-out; clamped to the frame's spp; default 4)")
    ap.add_argument("--features-out", metavar="FILE.npy",
                    help="also save the feature frame, float32 [H, W, 10]: position, normal, albedo, depth")
    ap.add_argument("--specular-features", type=int, default=0, metavar="K",
                    help="with --denoise, --features-out or --frames: follow Refl / Refr nodes through at most K steps (1 .. 8) and store the virtual "
                         "hit they show as the guide (Scene.render_features_specular); default 0: first-hit features.  Not with --motion-vectors "
                         "(motion frames carry first hits only) or --refine")
    ap.add_argument("--frames", type=int, metavar="N",
                    help="with --denoise: render N frames with temporal accumulation (Scene.render_sequence; frame k has seed SEED + k) and write "
                         "OUTPUT's name with _0000, _0001, ... before the extension")
    ap.add_argument("--yaw-step", type=float, default=None, metavar="DEG",
                    help="with --frames: frame k sees the scene file's camera with its yaw turned by k * DEG degrees (default 1; 0 with --move)")
    ap.add_argument("--move", type=float, nargs=4, action="append", metavar=("NODE", "DX", "DY", "DZ"),
                    help="with --frames: translate node NODE (its index among the scene's nodes) by (DX, DY, DZ) more in every frame -- frame 0 is the "
                         "scene file's, frame k sees the node k steps on; the uploaded scene is edited in place (Scene.update).  May be repeated.  "
                         "Without --denoise the frames are plain frames of the edited scene, all with seed SEED")
    ap.add_argument("--motion-vectors", action="store_true",
                    help="with --denoise --frames N --move ...: render the motion frame with the features (Scene.render_sequence(edit=...)) and "
                         "accumulate through it, so that a moved node's pixels keep their history")
    ap.add_argument("--change-samples", type=int, default=0, metavar="K",
                    help="with --denoise --frames N --move ... --motion-vectors: before each move render K samples per pixel of the coming frame "
                         "(its first K, of the same seed) and compare them with the frame's own after the move: where they differ the light changed -- "
                         "a moved node's shadow or reflection -- and the history is shortened (Scene.render_sequence(change_samples=K); K / spp more "
                         "rays per frame; default 0: off)")
    ap.add_argument("--accumulate", metavar="FILE.npz",
                    help="resumable frame (Scene.render_samples): continue the state saved in FILE.npz by --spp more samples per pixel (default: the "
                         "scene's own count), or start it when the file does not exist; writes FILE.npz and the picture of all samples so far.  A "
                         "state of another size or seed is refused.  With --time-limit the state that was cut short is saved and can be continued")
    ap.add_argument("--noise-out", metavar="FILE.npy",
                    help="with --accumulate: also save the noise buffer, float32 [H, W] (the variance estimate of the mean's luminance)")
    ap.add_argument("--refine", type=float, metavar="TOL",
                    help="refined frame (Scene.refine; path-traced mono frames): passes of a sample map and the samples it asks for, until every pixel's "
                         "relative standard error is <= TOL or the pixel holds --max-spp samples; prints one JSON line with the passes, the samples and "
                         "the mean spp.  With --accumulate the state in FILE.npz is continued and saved; with --denoise the frame goes through the "
                         "a-trous filter with its own noise estimate as the variance (denoise_signal, demodulate=0); with --denoise --split the "
                         "samples are kept apart as direct and indirect light (Scene.render_denoised_split(refine=TOL)) and each is filtered on its own")
    ap.add_argument("--max-spp", type=int, metavar="N", help="with --refine: the most samples a pixel may hold (required)")
    ap.add_argument("--refine-passes", type=int, default=8, metavar="P", help="with --refine: the most passes (default 8)")
    ap.add_argument("--sample-budget", type=int, metavar="N",
                    help="with --refine: the most samples the passes may add over the whole frame (Scene.refine(budget=N)): the tolerance is raised until "
                         "the frame can afford it; the JSON line gains budget, tolerance_reached and stage")
    ap.add_argument("--boost", type=int, metavar="T",
                    help="with --denoise --frames N: spend samples where the reprojected history is short (Scene.render_sequence(boost=...)): a pixel "
                         "whose history holds fewer than T units of --spp samples gets the missing whole units this frame, at most --boost-max of them; "
                         "--sample-budget N caps the samples of one frame (the target is lowered until the frame fits).  Path-traced mono frames; not "
                         "with --split or --refine.  The per-frame line gains target_used, samples and boosted")
    ap.add_argument("--boost-max", type=int, metavar="U", help="with --boost: the most units one frame gives a pixel (default 8)")
    ap.add_argument("--components-out", metavar="FILE.npz",
                    help="component frame (Scene.render_components; path-traced mono frames): render the frame's samples with direct and indirect light "
                         "kept apart and save direct, indirect, noise_direct, noise_indirect, samples and seed; the picture is their sum")
    ap.add_argument("--split", action="store_true",
                    help="with --denoise: filter direct and indirect light apart and add the results (Scene.render_denoised_split); path-traced mono "
                         "frames only, not with --adaptive.  With --frames N: the sequence keeps one history per component "
                         "(Scene.render_sequence(split=True); direct light's max_history is 8, a choice, indirect light's 32)")
    return ap


def sequence_path(output, k):
    """The file of frame k of a sequence: out.bmp -> out_0000.bmp."""
    stem, ext = os.path.splitext(output)
    return "%s_%04d%s" % (stem, k, ext)


def orbit(camera, frames, yaw_step):
    """The cameras of --frames: copies of `camera` with yaw + k * yaw_step."""
    for k in range(frames):
        c = abi.Camera.from_buffer_copy(camera)
        c.yaw = camera.yaw + k * yaw_step
        yield c


def move_nodes(s, moves):
    """One step of --move: every named node's transform translated by its (DX, DY, DZ), and the uploaded scene updated."""
    for node, dx, dy, dz in moves:
        Transform(s.nodes[int(node)]).translate(dx, dy, dz).store(s.nodes[int(node)])
    s.update()


def check_args(ap, a):
    """Refuses combinations the CLI does not render (before the scene is loaded)."""
    if a.denoise and a.adaptive is not None:
        ap.error("--denoise cannot be combined with --adaptive: denoising adaptive frames is not supported")
    if a.denoise and a.time_limit is not None:
        ap.error("--denoise cannot be combined with --time-limit: the denoiser needs the whole frame")
    if a.refine is not None:
        if a.max_spp is None or a.max_spp < 1 or a.max_spp > (1 << 24):
            ap.error("--refine needs --max-spp N, 1 <= N <= 2^24")
        if not (a.refine > 0 and a.refine < float("inf")):
            ap.error("--refine: TOL must be finite and > 0")
        if a.refine_passes < 1:
            ap.error("--refine-passes must be >= 1")
        if a.adaptive is not None or a.probe or a.frames is not None or a.time_limit is not None or a.progress:
            ap.error("--refine cannot be combined with --adaptive, --probe, --frames, --time-limit or --progress")
        if a.components_out and not a.split:
            ap.error("--refine with --components-out needs --denoise --split")
        if a.split and a.noise_out:
            ap.error("--refine --split cannot be combined with --noise-out: --components-out saves both components' noise")
        if a.sample_budget is not None and a.sample_budget < 0:
            ap.error("--sample-budget must be >= 0")
    elif a.max_spp is not None:
        ap.error("--max-spp needs --refine")
    elif a.sample_budget is not None and a.boost is None:
        ap.error("--sample-budget needs --refine")
    if a.boost is not None:
        if a.refine is not None or a.split:
            ap.error("--boost cannot be combined with --refine or --split")
        if not (a.denoise and a.frames is not None):
            ap.error("--boost needs --denoise --frames N")
        if a.boost < 1:
            ap.error("--boost: T must be >= 1")
        if a.boost_max is not None and a.boost_max < 1:
            ap.error("--boost-max must be >= 1")
        if a.sample_budget is not None and a.sample_budget < 0:
            ap.error("--sample-budget must be >= 0")
    elif a.boost_max is not None:
        ap.error("--boost-max needs --boost")
    if a.frames is not None and not a.denoise and not a.move:
        ap.error("--frames needs --denoise: a sequence is rendered with temporal accumulation and the filter")
    if a.move and a.frames is None:
        ap.error("--move needs --frames")
    if a.motion_vectors and not (a.denoise and a.frames is not None and a.move):
        ap.error("--motion-vectors needs --denoise --frames N --move ...")
    if not 0 <= a.specular_features <= 8:
        ap.error("--specular-features must be 0 .. 8")
    if a.specular_features and not (a.denoise or a.features_out):
        ap.error("--specular-features needs --denoise, --features-out or --denoise --frames N")
    if a.specular_features and a.frames is not None and not a.denoise:
        ap.error("--specular-features with --frames needs --denoise: plain frames render no feature frame")
    if a.specular_features and a.motion_vectors:
        ap.error("--specular-features cannot be combined with --motion-vectors: motion frames carry first hits only")
    if a.specular_features and a.refine is not None:
        ap.error("--specular-features cannot be combined with --refine")
    if a.change_samples < 0:
        ap.error("--change-samples must be >= 0")
    if a.change_samples and not a.motion_vectors:
        ap.error("--change-samples needs --denoise --frames N --move ... --motion-vectors")
    if a.move and (a.adaptive is not None or a.accumulate or a.probe or a.time_limit is not None):
        ap.error("--move cannot be combined with --adaptive, --accumulate, --probe or --time-limit")
    for m in a.move or []:
        if m[0] != int(m[0]) or m[0] < 0:
            ap.error("--move: NODE must be a node index, got %r" % m[0])
    if a.frames is not None and a.frames < 1:
        ap.error("--frames must be >= 1")
    if a.frames is not None and a.features_out:
        ap.error("--frames cannot be combined with --features-out")
    if a.accumulate and ((a.denoise and a.refine is None) or a.adaptive is not None or a.probe):
        ap.error("--accumulate cannot be combined with --denoise (but with --refine), --adaptive or --probe")
    if a.noise_out and not (a.accumulate or a.refine is not None):
        ap.error("--noise-out needs --accumulate or --refine")
    if a.spp is not None and a.accumulate and a.spp < 1:
        ap.error("--spp must be >= 1")
    if a.split and a.adaptive is not None:
        ap.error("--split cannot be combined with --adaptive")
    if a.split and not a.denoise:
        ap.error("--split needs --denoise")
    if a.components_out and a.frames is not None:
        ap.error("--components-out cannot be combined with --frames")
    if (a.split or a.components_out) and (a.accumulate or a.probe or a.adaptive is not None or a.time_limit is not None):
        ap.error("--split and --components-out cannot be combined with --accumulate, --probe, --adaptive or --time-limit")
    if a.components_out and a.denoise and not a.split:
        ap.error("--components-out with --denoise needs --split")


def check_components(ap, a, s):
    """--split and --components-out, once the scene is parsed (before it is uploaded): a component frame is a mono path-traced frame."""
    if not (a.split or a.components_out):
        return
    flag = "--split" if a.split else "--components-out"
    if not s.settings.gi:
        ap.error("%s needs a path-traced scene (gi on): a Whitted frame has no direct / indirect split" % flag)
    if s.camera.stereoSeparation > 0:
        ap.error("%s is not offered for stereo frames" % flag)


def budget_fields(info):
    """What --sample-budget adds to --refine's JSON line (nothing without it)."""
    return {k: info[k] for k in ("budget", "tolerance_reached", "stage") if k in info}


def check_refine(ap, a, s):
    """--refine, once the scene is parsed (before it is uploaded): a sample map is rendered on a mono path-traced frame."""
    if a.refine is None:
        return
    if not s.settings.gi:
        ap.error("--refine needs a path-traced scene (gi on)")
    if s.camera.stereoSeparation > 0:
        ap.error("--refine is not offered for stereo frames")


def save_components(path, direct, indirect, noise_direct, noise_indirect, samples, seed):
    with open(path, "wb") as f:
        np.savez(f, direct=direct, indirect=indirect, noise_direct=noise_direct, noise_indirect=noise_indirect, samples=np.int64(samples),
                 seed=np.uint32(int(seed) & 0xffffffff))
    print("wrote", path)


def load_accumulation(ap, a, s):
    """The state of --accumulate before the scene is uploaded: FILE.npz's when it exists (refused unless it is a state of this size and seed),
    else a new one."""
    if not os.path.exists(a.accumulate):
        return Accumulation.empty(s.frame_size, a.seed)
    try:
        state = Accumulation.load(a.accumulate)
        state.check("--accumulate " + a.accumulate, s.frame_size, a.seed, 0, 1)
    except (ValueError, OSError, KeyError) as e:
        ap.error(str(e))
    return state


def adaptive_summary(spp, info):
    """The CLI's JSON line for an adaptive frame: rungs run, mean spp, and per sample count the fraction of pixels that stopped there."""
    counts, n = np.unique(spp, return_counts=True)
    return {"rungs": info["rungs"], "samples": int(info["samples"]), "mean_spp": float(spp.mean()),
            "fraction_at": {str(int(c)): float(k) / spp.size for c, k in zip(counts, n)}}


def probe(s, x, y, shade=False, seed=42):
    """debugRayTrace (main.cpp:426-435): the camera ray through (x, y) and its closest hit, as a dict; with `shade` also trace() of that ray -- one
    sample of the scene's integrator, generator key floor(y) * width + floor(x) -- as "rgb"."""
    o, d = s.camera_rays(np.array([[x, y]], np.float64))
    r = s.trace_rays(o, d, record=True)
    rec = [float(v) for v in r["hit_rec"][0]]
    out = {"x": x, "y": y, "origin": [float(v) for v in o[0]], "dir": [float(v) for v in d[0]], "hit_id": int(r["hit_id"][0]),
           "dist": rec[0], "ip": rec[1:4], "norm": rec[4:7], "u": rec[7], "v": rec[8]}
    if shade:
        key = int(np.floor(y)) * s.frame_size[0] + int(np.floor(x))
        rgb = s.shade_rays(o, d, seed=seed, keys=np.array([key], np.uint32))
        out["rgb"] = [float(v) for v in rgb[0]]
    return out


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_args(ap, a)
    s = Scene.parseScene(a.scene)
    if a.width:
        s.settings.frameWidth = a.width
    if a.height:
        s.settings.frameHeight = a.height
    if a.spp:
        if s.settings.gi:
            s.settings.numPaths = a.spp
        elif s.camera.dof:
            s.camera.numDOFSamples = a.spp
    for m in a.move or []:
        if int(m[0]) >= s.desc.n_nodes:
            ap.error("--move: the scene has %d nodes, no node %d" % (s.desc.n_nodes, int(m[0])))
    if a.yaw_step is None:
        a.yaw_step = 0.0 if a.move else 1.0
    check_components(ap, a, s)
    check_refine(ap, a, s)
    state = load_accumulation(ap, a, s) if a.accumulate else None
    s.beginRender(a.device)
    if a.probe:
        print(json.dumps(probe(s, a.probe[0], a.probe[1], a.shade, a.seed)))
        return 0
    t0 = time.time()
    if a.frames is not None and not a.denoise:
        # plain frames of the edited scene: the sequence of --move without the filter
        for k, cam in enumerate(orbit(abi.Camera.from_buffer_copy(s.camera), a.frames, a.yaw_step)):
            if k:
                move_nodes(s, a.move)
            s.camera.yaw = cam.yaw
            s.beginFrame()
            img, st = s.render(seed=a.seed)
            path = sequence_path(a.output, k)
            if lib.frayhip_save_bmp(path.encode(), img.ctypes.data, img.shape[1], img.shape[0]):
                print(lib.frayhip_last_error().decode(), file=sys.stderr)
                return 1
            print("frame %d: yaw %+.2f, frame %.1f ms (kernels), scene update %d bytes; wrote %s"
                  % (k, k * a.yaw_step, st["ms_kernels"], s.get_option("scene_update_bytes"), path), flush=True)
        print("Rendered %d frames in %.2fs" % (a.frames, time.time() - t0))
        return 0
    if a.frames is not None:
        start = abi.Camera.from_buffer_copy(s.camera)
        edit = (lambda _k, scene: move_nodes(scene, a.move)) if a.motion_vectors else None
        boost = None
        if a.boost is not None:
            boost = dict(target=a.boost, max_units=8 if a.boost_max is None else a.boost_max, budget=a.sample_budget)
        for k, (img, _raw, info) in enumerate(s.render_sequence(orbit(start, a.frames, a.yaw_step), seed=a.seed, feature_samples=a.feature_samples,
                                                                edit=edit, split=a.split, change_samples=a.change_samples, boost=boost,
                                                                specular=a.specular_features)):
            path = sequence_path(a.output, k)
            img = img.cpu().numpy()
            if lib.frayhip_save_bmp(path.encode(), img.ctypes.data, img.shape[1], img.shape[0]):
                print(lib.frayhip_last_error().decode(), file=sys.stderr)
                return 1
            filter_ms = info["denoise_direct"]["ms_kernels"] + info["denoise_indirect"]["ms_kernels"] if a.split else info["denoise"]["ms_kernels"]
            print("frame %d: yaw %+.2f, frame %.1f ms, features %.1f ms, accumulation %.2f ms, filter %.2f ms (kernels); wrote %s"
                  % (k, k * a.yaw_step, info["render"]["ms_kernels"], info["features"]["ms_kernels"], info["temporal"]["ms_kernels"],
                     filter_ms, path), flush=True)
            if boost is not None:
                b = info["boost"]
                print("frame %d: boost target_used %d, samples %d, boosted %d" % (k, b["target_used"], b["samples"], b["boosted"]), flush=True)
            if a.move and not a.motion_vectors and k + 1 < a.frames:
                move_nodes(s, a.move)           # the generator renders the next frame when it is asked for it: after this edit
        print("Rendered %d frames in %.2fs" % (a.frames, time.time() - t0))
        return 0
    if a.refine is not None and a.split:
        img, raw, info = s.render_denoised_split(seed=a.seed, feature_samples=a.feature_samples, refine=a.refine, max_count=a.max_spp,
                                                 passes=a.refine_passes, budget=a.sample_budget)
        st = info["render"]
        held = info["refine"]["counts"]
        print(json.dumps(dict({"passes": st["passes"], "samples": st["samples"], "mean_spp": float(held.mean()), "min_spp": int(held.min()),
                               "max_spp": int(held.max())}, **budget_fields(st))))
        spp_text = "refined to tolerance %g, mean %.2f spp, direct and indirect light denoised apart: features %.1f ms, filters %.1f + %.1f ms" % (
            a.refine, held.mean(), info["features"]["ms_kernels"], info["denoise_direct"]["ms_kernels"], info["denoise_indirect"]["ms_kernels"])
        if a.features_out:
            np.save(a.features_out, info["features_frame"])
        if a.components_out:
            save_components(a.components_out, info["direct_rgb"], info["indirect_rgb"], info["noise_direct"], info["noise_indirect"],
                            int(held.max()), a.seed)
    elif a.refine is not None:
        from . import denoise_signal
        img, state, noise, info = s.refine(state, a.refine, a.max_spp, passes=a.refine_passes, seed=a.seed, budget=a.sample_budget)
        held = state.count_plane()
        st = info
        print(json.dumps(dict({"passes": info["passes"], "samples": info["samples"], "mean_spp": float(held.mean()), "min_spp": int(held.min()),
                               "max_spp": int(held.max())}, **budget_fields(info))))
        spp_text = "refined to tolerance %g, mean %.2f spp" % (a.refine, held.mean())
        if a.accumulate:
            print("wrote", state.save(a.accumulate))
        if a.noise_out:
            np.save(a.noise_out, noise)
            print("wrote", a.noise_out)
        if a.denoise:
            feat = s.render_features(min(a.feature_samples, max(int(held.max()), 1)), seed=a.seed)
            if a.features_out:
                np.save(a.features_out, feat)
            img = denoise_signal(img, noise, feat, demodulate=0)
            spp_text += ", denoised with its own noise estimate"
    elif a.denoise and a.split:
        img, raw, info = s.render_denoised_split(seed=a.seed, feature_samples=a.feature_samples, specular=a.specular_features)
        st = info["render"]
        spp_text = "%d spp, direct and indirect light denoised apart: features %.1f ms, filters %.1f + %.1f ms" % (
            s.samples_per_pixel(), info["features"]["ms_kernels"], info["denoise_direct"]["ms_kernels"], info["denoise_indirect"]["ms_kernels"])
        if a.features_out:
            np.save(a.features_out, info["features_frame"])
        if a.components_out:
            save_components(a.components_out, info["direct_rgb"], info["indirect_rgb"], info["noise_direct"], info["noise_indirect"],
                            s.samples_per_pixel(), a.seed)
    elif a.components_out:
        direct, indirect, _state, nd, ni, st = s.render_components(s.samples_per_pixel(), seed=a.seed, noise=True, stats=True)
        img = direct + indirect
        spp_text = "%d spp, direct and indirect light kept apart" % s.samples_per_pixel()
        save_components(a.components_out, direct, indirect, nd, ni, s.samples_per_pixel(), a.seed)
    elif a.denoise:
        img, raw, info = s.render_denoised(seed=a.seed, feature_samples=a.feature_samples, specular=a.specular_features)
        st = info["render"]
        spp_text = "%d spp, denoised%s: features %.1f ms, filter %.1f ms" % (
            s.samples_per_pixel(), "" if info["rgb_half"] is not None else " without the half-spp estimate",
            info["features"]["ms_kernels"], info["denoise"]["ms_kernels"])
        if a.features_out:
            np.save(a.features_out, info["features_frame"])
    elif a.adaptive is not None:
        img, spp_map, _err, info = s.render_adaptive(a.adaptive, min_spp=a.min_spp, err_floor=a.adaptive_floor, seed=a.seed)
        st = info["stats"]
        print(json.dumps(adaptive_summary(spp_map, info)))
        spp_text = "adaptive, mean %.2f spp" % spp_map.mean()
    elif a.accumulate:
        def progress(info):
            if a.progress:
                print("%s%d / %d spp, batch %d / %d, %.1f ms" % ("done: " if info["final"] else "", info["samples_done"], info["samples_total"],
                                                                info["batches_done"], info["batches_total"], info["ms_elapsed"]), flush=True)
            return a.time_limit is not None and not info["final"] and info["ms_elapsed"] >= a.time_limit * 1000.0
        before = state.samples_done
        count = a.spp if a.spp else s.samples_per_pixel()
        watch = a.progress or a.time_limit is not None
        out = s.render_samples(count, state, seed=a.seed, stats=True, noise=bool(a.noise_out), progress=progress if watch else None)
        img, st = out[0], out[-1]
        spp_text = "samples %d .. %d of the state, %d spp in all" % (before, state.samples_done - 1, state.samples_done)
        if st.get("cancelled"):
            print("Time limit of %gs reached: the state holds %d samples per pixel (%d of this run's %d); run again to continue"
                  % (a.time_limit, state.samples_done, state.samples_done - before, count))
        print("wrote", state.save(a.accumulate))
        if a.noise_out:
            np.save(a.noise_out, out[2])
            print("wrote", a.noise_out)
    elif a.progress or a.time_limit is not None:
        def progress(info):
            if a.progress:
                print("%s%d / %d spp, batch %d / %d, %.1f ms" % ("done: " if info["final"] else "", info["samples_done"], info["samples_total"],
                                                                info["batches_done"], info["batches_total"], info["ms_elapsed"]), flush=True)
            if a.time_limit is not None and not info["final"] and info["ms_elapsed"] >= a.time_limit * 1000.0:
                cancel_at.append(info["ms_elapsed"])
                return True
            return False
        cancel_at = []
        img, st = s.render(seed=a.seed, progress=progress)
        spp = st["samples_done"]
        spp_text = "%d spp" % spp
        if st["cancelled"]:
            print("Time limit of %gs reached: the frame holds %d of %d samples per pixel (finished %.1f ms after the cancel)"
                  % (a.time_limit, spp, s.samples_per_pixel(), st["ms_total"] - cancel_at[0]))
    else:
        img, st = s.render(seed=a.seed)
        spp_text = "%d spp" % s.samples_per_pixel()
    print("Render took %.2fs (%d x %d, %s, kernels %.1f ms)" % (time.time() - t0, img.shape[1], img.shape[0], spp_text, st["ms_kernels"]))
    if a.features_out and not a.denoise:
        n_feat = min(a.feature_samples, s.samples_per_pixel())
        np.save(a.features_out, s.render_features_specular(a.specular_features, n_feat, seed=a.seed) if a.specular_features
                else s.render_features(n_feat, seed=a.seed))
        print("wrote", a.features_out)
    rc = lib.frayhip_save_bmp(a.output.encode(), img.ctypes.data, img.shape[1], img.shape[0])
    if rc:
        print(lib.frayhip_last_error().decode(), file=sys.stderr)
        return 1
    print("wrote", a.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
