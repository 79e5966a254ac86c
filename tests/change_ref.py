"""A float32 numpy restatement of the change frame (include/frayhip.h "change frames", fray_amd/csrc/change.hip) and of the gradient-adaptive
accumulation (frayhip_temporal_accumulate_adaptive, fray_amd/csrc/temporal.hip): every operation in the order the header writes it, vectorised
over pixels.  Only + - * / sqrt floor min max abs and compares, all correctly rounded in numpy as on the device, so the two agree in every bit.

texels        per texel (d, m): the luminance sums' difference and maximum, zero where a sum is not finite, where m <= 0 and where moved != 0
change_frame  frayhip_change_frame: the window's sum(d) / sum(m), j outer, i inner, times the gain, clamped to 1
accumulate    frayhip_temporal_accumulate_adaptive: tests/temporal_ref.py's accumulate (motion None) or tests/motion_ref.py's with step 3 as the
              header's three cases
Used by tests/test_change_abi.py (synthetic inputs) and tests/test_gpu_change.py (the device kernels against it, bit for bit)."""
import numpy as np

from denoise_ref import _shift
from temporal_ref import DEFAULTS, F, HISTORY_CHANNELS, dot, is_zero, lum, project, spatial_variance, unit_normals, view_fields

ACCUM_CHANNELS = 4
CHANGE_DEFAULTS = dict(radius=3, gain=1.0)


def texels(before, after, motion=None):
    """(d, m) per texel, float32 [H, W] each."""
    before, after = np.asarray(before, F), np.asarray(after, F)
    assert before.shape == after.shape and before.shape[2] == ACCUM_CHANNELS
    with np.errstate(all="ignore"):
        la, lb = lum(before), lum(after)
        m = np.maximum(la, lb)
        d = np.abs(lb - la)
        keep = np.isfinite(la) & np.isfinite(lb) & (m > 0)
    if motion is not None:
        keep = keep & (np.asarray(motion, F)[..., 3] == 0)
    return np.where(keep, d, F(0)).astype(F), np.where(keep, m, F(0)).astype(F)


def change_frame(before, after, motion=None, radius=3, gain=1.0):
    """frayhip_change_frame: change [H, W] float32."""
    assert 0 <= radius <= 3
    d, m = texels(before, after, motion)
    sd = np.zeros(d.shape, F)
    sm = np.zeros(d.shape, F)
    with np.errstate(all="ignore"):
        for j in range(-radius, radius + 1):
            for i in range(-radius, radius + 1):
                dq, valid = _shift(d, j, i)
                mq, _ = _shift(m, j, i)
                sd = sd + np.where(valid, dq, F(0))          # a tap outside the image is skipped: adding +0 to a sum of values >= +0 changes no bit
                sm = sm + np.where(valid, mq, F(0))
        some = sm > 0
        ratio = sd / np.where(some, sm, F(1))
        # fminf: the number when the other side is a NaN (inf / inf, when both sums overflow)
        return np.where(some, np.fmin(F(1), F(gain) * ratio), F(0)).astype(F)


def accumulate(rgb, feat, change, motion=None, prev_view=None, hist_in=None, **params):
    """frayhip_temporal_accumulate_adaptive: (hist_out [H, W, 12], signal [H, W, 3], variance [H, W]), float32."""
    p = dict(DEFAULTS)
    p.update(params)
    assert (prev_view is None) == (hist_in is None)
    rgb, feat, change = np.asarray(rgb, F), np.asarray(feat, F), np.asarray(change, F)
    H, W = rgb.shape[:2]
    assert change.shape == (H, W)
    P = feat[..., 0:3]
    n = unit_normals(feat)
    if motion is not None:
        motion = np.asarray(motion, F)
        Q = motion[..., 0:3]                                 # P'
        mn = unit_normals(motion[..., 1:7])                  # n' (channels 4..6), scaled the way the normal is
    else:
        Q, mn = P, n
    z = feat[..., 9]
    c = rgb / np.maximum(feat[..., 6:9], F(1e-3)) if p["demodulate"] else rgb.copy()
    l = lum(c)
    l2 = l * l
    sb = np.zeros((H, W), F)
    h = np.zeros((H, W, 6), F)                               # acc.rgb, N, m1, m2
    with np.errstate(all="ignore"):
        if hist_in is not None:
            hist_in = np.asarray(hist_in, F)
            V = view_fields(prev_view)
            assert (V["width"], V["height"]) == (W, H) and hist_in.shape == (H, W, HISTORY_CHANNELS)
            fx, fy, zc = project(Q, prev_view)
            d = Q - V["pos"]
            u, v = fx - F(p["film_offset"]), fy - F(p["film_offset"])
            x0f, y0f = np.floor(u), np.floor(v)
            ok = ~is_zero(n) & ~is_zero(mn) & (zc > 0) & (x0f >= F(-1)) & (x0f <= F(W - 1)) & (y0f >= F(-1)) & (y0f <= F(H - 1))
            x0 = np.where(ok, x0f, F(0)).astype(np.int64)
            y0 = np.where(ok, y0f, F(0)).astype(np.int64)
            tx, ty = u - x0f, v - y0f
            tol = F(p["plane_tolerance"]) * np.sqrt(dot(d, d))
            for j in (0, 1):
                for i in (0, 1):
                    xq, yq = x0 + i, y0 + j
                    inside = ok & (xq >= 0) & (xq < W) & (yq >= 0) & (yq < H)
                    q = hist_in[np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)]
                    Pq, nq = q[..., 4:7], q[..., 8:11]
                    tap = inside & ~is_zero(nq) & (dot(mn, nq) >= F(p["normal_min_dot"])) & (np.abs(dot(Pq - Q, mn)) <= tol)
                    b = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                    sb = sb + np.where(tap, b, F(0))
                    hq = np.concatenate([q[..., 0:4], q[..., 7:8], q[..., 11:12]], axis=-1)
                    h = h + np.where(tap[..., None], b[..., None] * hq, F(0))
        found = sb > 0
        h = h / np.where(found, sb, F(1))[..., None]
        g = np.where(found, change, F(0))                    # read only where a history was fetched
        cut = found & ~(g < F(1))                            # 1, above 1, NaN: no history
        part = found & ~cut & (g > 0)
        keep = found & ~cut & ~part                          # +0, -0, negative: the plain arithmetic
        N0 = np.minimum(h[..., 3] + F(1), F(p["max_history"]))
        a0 = np.maximum(F(p["alpha_min"]), F(1) / N0)
        a_part = a0 + g * (F(1) - a0)
        alpha = np.where(part, a_part, a0).astype(F)
        N = np.where(keep, N0, np.where(part, np.minimum(N0, F(1) / a_part), F(1))).astype(F)
        blend = keep | part
        acc = np.where(blend[..., None], h[..., 0:3] + alpha[..., None] * (c - h[..., 0:3]), c).astype(F)
        m1 = np.where(blend, h[..., 4] + alpha * (l - h[..., 4]), l).astype(F)
        m2 = np.where(blend, h[..., 5] + alpha * (l2 - h[..., 5]), l2).astype(F)
        hist = np.empty((H, W, HISTORY_CHANNELS), F)
        hist[..., 0:3], hist[..., 3] = acc, N
        hist[..., 4:7], hist[..., 7] = P, m1                 # the CURRENT position and unit normal
        hist[..., 8:11], hist[..., 11] = n, m2
        var = np.maximum(F(0), m2 - m1 * m1)
        vh = F(p["variance_history"])
        young = N < vh
        if young.any():
            var = np.where(young, spatial_variance(hist, z, p["plane_tolerance"], p["normal_min_dot"]) * (vh / N), var)
    return hist, acc.copy(), var.astype(F)
