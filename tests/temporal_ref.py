"""A float32 numpy restatement of the temporal stage (include/frayhip.h "temporal accumulation", fray_amd/csrc/temporal.hip): the same
projection, the same taps in the same order and the same roundings, vectorised over pixels.  Only + - * / sqrt floor min max and compares, all
correctly rounded in numpy as on the device, so the two agree in every bit.  Normative together with the header text.  Used by
tests/test_temporal_abi.py (checked on synthetic inputs and against the oracle's camera rays) and tests/test_gpu_temporal.py (the device
kernels against it)."""
import numpy as np

from denoise_ref import _shift

F = np.float32
HISTORY_CHANNELS = 12
DEFAULTS = dict(demodulate=1, max_history=32, variance_history=4, alpha_min=0.05, film_offset=0.5, plane_tolerance=0.02, normal_min_dot=0.9)


def lum(c):
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / F(3)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def view_fields(view):
    """A frayhip_view (the ctypes mirror, or a dict of the same names) as float32 arrays and ints."""
    get = (lambda k: view[k]) if isinstance(view, dict) else (lambda k: getattr(view, k))
    vec = lambda k: np.array([get(k)[i] for i in range(3)], F)
    return dict(pos=vec("pos"), right=vec("right"), up=vec("up"), front=vec("front"), tan_x=F(get("tan_x")), tan_y=F(get("tan_y")),
                width=int(get("width")), height=int(get("height")))


def project(P, view):
    """World points [..., 3] float32 onto the film of `view`: (fx, fy, zc); fx and fy mean nothing where zc <= 0."""
    V = view_fields(view)
    P = np.asarray(P, F)
    d = P - V["pos"]
    zc = dot(d, V["front"])
    xc = dot(d, V["right"])
    yc = dot(d, V["up"])
    with np.errstate(all="ignore"):
        fx = ((xc / zc / V["tan_x"] + F(1)) * F(0.5)) * F(V["width"])
        fy = ((F(1) - yc / zc / V["tan_y"]) * F(0.5)) * F(V["height"])
    return fx, fy, zc


def unit_normals(feat):
    """k_dn_prepare's normals: scaled to unit length where not zero."""
    n = np.asarray(feat, F)[..., 3:6].copy()
    nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    nz = nn > 0
    n[nz] = n[nz] / np.sqrt(nn)[nz][:, None]
    return n


def is_zero(n):
    return (n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0)


def accumulate(rgb, feat, prev_view=None, hist_in=None, **params):
    """frayhip_temporal_accumulate: (hist_out [H, W, 12], signal [H, W, 3], variance [H, W]), float32."""
    p = dict(DEFAULTS)
    p.update(params)
    assert (prev_view is None) == (hist_in is None)
    rgb, feat = np.asarray(rgb, F), np.asarray(feat, F)
    H, W = rgb.shape[:2]
    P = feat[..., 0:3]
    n = unit_normals(feat)
    z = feat[..., 9]
    c = rgb / np.maximum(feat[..., 6:9], F(1e-3)) if p["demodulate"] else rgb.copy()
    l = lum(c)
    l2 = l * l
    sb = np.zeros((H, W), F)
    h = np.zeros((H, W, 6), F)                       # acc.rgb, N, m1, m2
    with np.errstate(all="ignore"):
        if hist_in is not None:
            hist_in = np.asarray(hist_in, F)
            V = view_fields(prev_view)
            assert (V["width"], V["height"]) == (W, H) and hist_in.shape == (H, W, HISTORY_CHANNELS)
            fx, fy, zc = project(P, prev_view)
            d = P - V["pos"]
            u, v = fx - F(p["film_offset"]), fy - F(p["film_offset"])
            x0f, y0f = np.floor(u), np.floor(v)
            ok = ~is_zero(n) & (zc > 0) & (x0f >= F(-1)) & (x0f <= F(W - 1)) & (y0f >= F(-1)) & (y0f <= F(H - 1))
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
                    tap = inside & ~is_zero(nq) & (dot(n, nq) >= F(p["normal_min_dot"])) & (np.abs(dot(Pq - P, n)) <= tol)
                    b = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                    sb = sb + np.where(tap, b, F(0))
                    hq = np.concatenate([q[..., 0:4], q[..., 7:8], q[..., 11:12]], axis=-1)
                    h = h + np.where(tap[..., None], b[..., None] * hq, F(0))
        found = sb > 0
        h = h / np.where(found, sb, F(1))[..., None]
        N = np.where(found, np.minimum(h[..., 3] + F(1), F(p["max_history"])), F(1)).astype(F)
        alpha = np.maximum(F(p["alpha_min"]), F(1) / N)
        acc = np.where(found[..., None], h[..., 0:3] + alpha[..., None] * (c - h[..., 0:3]), c).astype(F)
        m1 = np.where(found, h[..., 4] + alpha * (l - h[..., 4]), l).astype(F)
        m2 = np.where(found, h[..., 5] + alpha * (l2 - h[..., 5]), l2).astype(F)
        hist = np.empty((H, W, HISTORY_CHANNELS), F)
        hist[..., 0:3], hist[..., 3] = acc, N
        hist[..., 4:7], hist[..., 7] = P, m1
        hist[..., 8:11], hist[..., 11] = n, m2
        var = np.maximum(F(0), m2 - m1 * m1)
        vh = F(p["variance_history"])
        young = N < vh
        if young.any():
            var = np.where(young, spatial_variance(hist, z, p["plane_tolerance"], p["normal_min_dot"]) * (vh / N), var)
    return hist, acc.copy(), var.astype(F)


def spatial_variance(hist, z, plane_tolerance, normal_min_dot):
    """k_tp_variance before the variance_history / N scale: the luminance variance of the 7x7 window's taps on the pixel's surface."""
    H, W = hist.shape[:2]
    P, n, m1, m2 = hist[..., 4:7], hist[..., 8:11], hist[..., 7], hist[..., 11]
    pzero = is_zero(n)
    tol = F(plane_tolerance) * np.asarray(z, F)
    s1 = np.zeros((H, W), F)
    s2 = np.zeros((H, W), F)
    cnt = np.zeros((H, W), F)
    for j in range(-3, 4):
        for i in range(-3, 4):
            Pq, valid = _shift(P, j, i)
            nq, _ = _shift(n, j, i)
            m1q, _ = _shift(m1, j, i)
            m2q, _ = _shift(m2, j, i)
            qzero = is_zero(nq)
            surface = (dot(n, nq) >= F(normal_min_dot)) & (np.abs(dot(Pq - P, n)) <= tol)
            tap = valid & np.where(pzero | qzero, pzero & qzero, surface)
            s1 = s1 + np.where(tap, m1q, F(0))
            s2 = s2 + np.where(tap, m2q, F(0))
            cnt = cnt + np.where(tap, F(1), F(0))
    some = cnt > 0
    mean1 = np.where(some, s1 / np.where(some, cnt, F(1)), m1).astype(F)
    mean2 = np.where(some, s2 / np.where(some, cnt, F(1)), m2).astype(F)
    return np.maximum(F(0), mean2 - mean1 * mean1)
