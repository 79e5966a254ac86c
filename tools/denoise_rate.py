"""Feature frames and the denoiser on one GPU (include/frayhip.h "feature frames", "denoising"): their cost at 1080p and what the denoiser buys
against fixed-spp frames.  Times are the library's own (frayhip_stats.ms_kernels: HIP events around the call's device work; ms_total: the call's
wall time), medians over --rounds rounds after --warmup, every call on one torch stream with the outputs resident on the device.

  features_<scene>_n<N>   frayhip_render_features_device at 1920x1080 (cornell_box n = 1 and 4, hw9/dragon n = 1), beside
  primary_<scene>         the MODE_PRIMARY_ID frame of the same scene (k_primary: one camera ray and closest hit per pixel)
  denoise_L<levels>_<half|nohalf>   frayhip_denoise_device at 1920x1080 on a cornell_box 16-spp frame and its features
  quality_<scene>_<spp>   cornell_box / smallpt at 1920x1080, 4 / 16 / 64 spp, feature_samples 4, default parameters: RMS of the raw and of
                          the denoised frame against a --ref-spp frame of the same seed, relative RMS (RMS / root mean square of the reference),
                          the time of frame + features + filter (device kernels, each part alone), and the RMS a fixed-spp frame reaches in the
                          same time (linear interpolation over fixed-spp frames timed the same way)

    python tools/denoise_rate.py [--rounds 5] [--warmup 1] [--ref-spp 1024] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
FIXED = [2, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128]


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--out")
    a = ap.parse_args()
    import ctypes as C
    import torch
    import fray_amd
    from fray_amd import abi
    from conftest import open_scene

    fray_amd.lib.frayhip_init(0)
    stream = torch.cuda.Stream()
    h = stream.cuda_stream
    res = {}
    with torch.cuda.stream(stream):
        feat_t = torch.empty((H, W, 10), dtype=torch.float32, device="cuda")
        rgb_t = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        half_t = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        out_t = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def features_call(s, n):
        st = abi.Stats()
        fr = abi.Frame(mode=abi.MODE_RENDER, seed=42)
        rc = fray_amd.lib.frayhip_render_features_device(s._dev, C.byref(fr), n, feat_t.data_ptr(), h, C.byref(st))
        assert rc == 0, fray_amd.lib.frayhip_last_error()
        return st.as_dict()

    # ---- the feature kernel against k_primary ----
    for name, spp, ns in (("cornell_box.fray", 64, (1, 4)), ("hw9/dragon.fray", None, (1,))):
        s = open_scene(fray_amd, name, W, H, wantAA=0, **({"numPaths": spp} if spp else {}))
        s.beginRender()
        tag = os.path.basename(name).split(".")[0]
        prim, feats = [], {n: [] for n in ns}
        with torch.cuda.stream(stream):
            ids = torch.empty((H, W), dtype=torch.int32, device="cuda")
        for r in range(a.warmup + a.rounds):
            st = s.render_device(None, mode=abi.MODE_PRIMARY_ID, d_id_ptr=ids.data_ptr(), stream=h)
            if r >= a.warmup:
                prim.append(st["ms_kernels"])
            for n in ns:
                st = features_call(s, n)
                if r >= a.warmup:
                    feats[n].append(st["ms_kernels"])
        res["primary_%s" % tag] = {"kernels_ms": med(prim)}
        for n in ns:
            res["features_%s_n%d" % (tag, n)] = {"kernels_ms": med(feats[n]), "ratio_to_primary": med(feats[n]) / med(prim)}
        s.close()

    # ---- the filter ----
    s = open_scene(fray_amd, "cornell_box.fray", W, H, wantAA=0, numPaths=16)
    s.beginRender()
    s.render_device(rgb_t.data_ptr(), seed=42, stream=h)
    features_call(s, 4)
    s.settings.numPaths = 8
    s.beginFrame()
    s.render_device(half_t.data_ptr(), seed=42, stream=h)
    s.close()
    for levels in (3, 5):
        for with_half in (False, True):
            p = fray_amd.denoise_params(levels=levels)
            ks, calls = [], []
            for r in range(a.warmup + a.rounds):
                st = abi.Stats()
                rc = fray_amd.lib.frayhip_denoise_device(W, H, rgb_t.data_ptr(), half_t.data_ptr() if with_half else None, feat_t.data_ptr(),
                                                         C.byref(p), out_t.data_ptr(), h, C.byref(st))
                assert rc == 0, fray_amd.lib.frayhip_last_error()
                if r >= a.warmup:
                    ks.append(st.ms_kernels)
                    calls.append(st.ms_total)
            res["denoise_L%d_%s" % (levels, "half" if with_half else "nohalf")] = {"kernels_ms": med(ks), "call_ms": med(calls)}

    # ---- quality at equal time ----
    for name in ("cornell_box.fray", "smallpt.fray"):
        tag = name.split(".")[0]
        s = open_scene(fray_amd, name, W, H, wantAA=0, numPaths=a.ref_spp)
        s.beginRender()
        ref, _ = s.render(seed=42)
        ref = ref.astype(np.float64)
        ref_ms = float(np.sqrt((ref ** 2).mean()))

        def rms(img):
            return float(np.sqrt(((img.astype(np.float64) - ref) ** 2).mean()))

        def frame_ms(n):
            s.settings.numPaths = n
            s.beginFrame()
            ts = []
            for r in range(a.warmup + a.rounds):
                st = s.render_device(rgb_t.data_ptr(), seed=42, stream=h)
                if r >= a.warmup:
                    ts.append(st["ms_kernels"])
            torch.cuda.synchronize()
            return med(ts), rms(rgb_t.cpu().numpy())

        fixed = {n: frame_ms(n) for n in FIXED}
        fx = sorted(fixed.values())
        fstats = []
        for r in range(a.warmup + a.rounds):
            st = features_call(s, 4)
            if r >= a.warmup:
                fstats.append(st["ms_kernels"])
        f_ms = med(fstats)
        for spp in (4, 16, 64):
            s.settings.numPaths = spp
            s.beginFrame()
            den, raw, info = s.render_denoised(seed=42, feature_samples=4)
            d_args = [torch.from_numpy(raw).cuda(), torch.from_numpy(info["features_frame"]).cuda(),
                      torch.from_numpy(info["rgb_half"]).cuda() if info["rgb_half"] is not None else None]
            ds = []
            for r in range(a.warmup + a.rounds):
                _, st = fray_amd.denoise(*d_args, stats=True, stream=stream)
                if r >= a.warmup:
                    ds.append(st["ms_kernels"])
            fr_ms = fixed[spp][0] if spp in fixed else frame_ms(spp)[0]
            total = fr_ms + f_ms + med(ds)
            r_raw, r_den = rms(raw), rms(den)
            res["quality_%s_%d" % (tag, spp)] = {
                "rms_raw": r_raw, "rms_denoised": r_den, "rel_rms_raw": r_raw / ref_ms, "rel_rms_denoised": r_den / ref_ms,
                "ratio": r_den / r_raw, "frame_ms": fr_ms, "features_ms": f_ms, "denoise_ms": med(ds), "total_ms": total,
                "render_denoised_wall_ms": info["render"]["ms_total"] + info["features"]["ms_total"] + info["denoise"]["ms_total"],
                "fixed_rms_at_equal_time": float(np.interp(total, [x[0] for x in fx], [x[1] for x in fx])),
                "fixed_spp_at_equal_time": float(np.interp(total, [fixed[n][0] for n in FIXED], FIXED))}
        res["fixed_%s" % tag] = {str(n): {"kernels_ms": fixed[n][0], "rms": fixed[n][1]} for n in FIXED}
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
