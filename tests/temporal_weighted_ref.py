"""A float32 numpy restatement of the weighted accumulation (include/frayhip.h "weighted accumulation and history maps",
frayhip_temporal_accumulate_weighted), written from the header's text: every operation in the order the header writes it, vectorised over
pixels.  Only + - * / sqrt floor min max abs and compares, all correctly rounded in numpy as on the device, so the two agree in every bit.

fetch        steps 1 and 2: the surface carried into the previous view, the four taps in tap order (j outer), the sums over the counted taps
             of b, b * {acc.rgb, N, m1, m2} and b * units_in -- shared with tests/history_map_ref.py, as the two kernels share one device function
accumulate   frayhip_temporal_accumulate_weighted: (hist_out [H, W, 12], units_out [H, W], signal [H, W, 3], variance [H, W])
Used by tests/test_history_map_abi.py (synthetic inputs) and tests/test_gpu_history_map.py (the device kernels against it, bit for bit)."""
import numpy as np

from temporal_ref import DEFAULTS, F, HISTORY_CHANNELS, dot, is_zero, lum, project, spatial_variance, unit_normals, view_fields


def fetch(feat, prev_view, hist_in, units_in, motion, p):
    """(sb, h [H, W, 6] = sums of b * {acc.rgb, N, m1, m2}, hu = sum of b * units), all undivided; zeros where no history is fetched."""
    feat = np.asarray(feat, F)
    H, W = feat.shape[:2]
    sb = np.zeros((H, W), F)
    h = np.zeros((H, W, 6), F)
    hu = np.zeros((H, W), F)
    if hist_in is None:
        return sb, h, hu
    P = feat[..., 0:3]
    n = unit_normals(feat)
    if motion is not None:
        motion = np.asarray(motion, F)
        Q = motion[..., 0:3]                                 # P'
        mn = unit_normals(motion[..., 1:7])                  # n' (channels 4..6), scaled the way the normal is
    else:
        Q, mn = P, n
    hist_in, units_in = np.asarray(hist_in, F), np.asarray(units_in, F)
    V = view_fields(prev_view)
    assert (V["width"], V["height"]) == (W, H) and hist_in.shape == (H, W, HISTORY_CHANNELS) and units_in.shape == (H, W)
    with np.errstate(all="ignore"):
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
                yc, xc = np.clip(yq, 0, H - 1), np.clip(xq, 0, W - 1)
                q = hist_in[yc, xc]
                Pq, nq = q[..., 4:7], q[..., 8:11]
                tap = inside & ~is_zero(nq) & (dot(mn, nq) >= F(p["normal_min_dot"])) & (np.abs(dot(Pq - Q, mn)) <= tol)
                b = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                sb = sb + np.where(tap, b, F(0))
                hq = np.concatenate([q[..., 0:4], q[..., 7:8], q[..., 11:12]], axis=-1)
                h = h + np.where(tap[..., None], b[..., None] * hq, F(0))
                hu = hu + np.where(tap, b * units_in[yc, xc], F(0))
    return sb.astype(F), h.astype(F), hu.astype(F)


def clean_weight(weight, max_history):
    """w = weight; if (!(w >= 1)) w = 1; w = fminf(w, max_history)."""
    w = np.asarray(weight, F)
    with np.errstate(all="ignore"):
        w = np.where(w >= F(1), w, F(1)).astype(F)
    return np.fmin(w, F(max_history)).astype(F)


def accumulate(rgb, feat, weight, motion=None, change=None, prev_view=None, hist_in=None, units_in=None, **params):
    """frayhip_temporal_accumulate_weighted: (hist_out [H, W, 12], units_out [H, W], signal [H, W, 3], variance [H, W]), float32."""
    p = dict(DEFAULTS)
    p.update(params)
    assert (prev_view is None) == (hist_in is None) == (units_in is None)
    rgb, feat = np.asarray(rgb, F), np.asarray(feat, F)
    H, W = rgb.shape[:2]
    P = feat[..., 0:3]
    n = unit_normals(feat)
    z = feat[..., 9]
    mh = F(p["max_history"])
    w = clean_weight(weight, p["max_history"])
    assert w.shape == (H, W)
    with np.errstate(all="ignore"):
        c = rgb / np.maximum(feat[..., 6:9], F(1e-3)) if p["demodulate"] else rgb.copy()
        l = lum(c)
        l2 = l * l
        sb, h, hu = fetch(feat, prev_view, hist_in, units_in, motion, p)
        found = sb > 0
        div = np.where(found, sb, F(1))
        h = h / div[..., None]
        hu = hu / div
        if change is not None:
            g = np.where(found, np.asarray(change, F), F(0))     # read only where a history was fetched
        else:
            g = np.zeros((H, W), F)
        cut = found & ~(g < F(1))                            # 1, above 1, NaN: no history
        part = found & ~cut & (g > 0)
        keep = found & ~cut & ~part                          # no change frame, +0, -0, negative: the plain arithmetic
        N0 = np.fmin(h[..., 3] + F(1), mh)
        U0 = np.fmin(hu + w, mh)
        a0 = np.fmax(F(p["alpha_min"]), w / U0)
        a_part = a0 + g * (F(1) - a0)
        alpha = np.where(part, a_part, a0).astype(F)
        N = np.where(keep, N0, np.where(part, np.fmin(N0, F(1) / a_part), F(1))).astype(F)
        U = np.where(keep, U0, np.where(part, np.fmin(U0, w / a_part), w)).astype(F)
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
    return hist, U, acc.copy(), var.astype(F)
