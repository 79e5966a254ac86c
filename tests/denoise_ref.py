"""A float32 numpy restatement of the denoiser (include/frayhip.h "denoising", fray_amd/csrc/denoise.hip): the same packing, the same taps in
the same order and the same roundings, vectorised over pixels.  Used by tests/test_denoise_abi.py (checked on synthetic inputs) and
tests/test_gpu_denoise.py (the device filter against it)."""
import numpy as np

F = np.float32
B3 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
DEFAULTS = dict(levels=5, demodulate=1, sigma_luminance=4.0, sigma_normal=128.0, sigma_depth=1.0, sigma_albedo=0.1)


def lum(c):
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / F(3)


def _demod(c, a):
    return c / np.maximum(a, F(1e-3))


def _shift(a, dy, dx):
    """a[y + dy, x + dx] with edge indices clamped, and the mask of taps inside the image."""
    H, W = a.shape[:2]
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    valid = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    return a[np.clip(ys, 0, H - 1)][:, np.clip(xs, 0, W - 1)], valid


def prepare(rgb, feat, rgb_half=None, demodulate=1):
    """k_dn_prepare: unit normals, depth, albedo, depth gradient, the signal and the prefiltered variance."""
    rgb, feat = np.asarray(rgb, F), np.asarray(feat, F)
    H, W = rgb.shape[:2]
    n = feat[..., 3:6].copy()
    nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    s = np.sqrt(nn)
    nz = nn > 0
    n[nz] = n[nz] / s[nz][:, None]
    z = feat[..., 9].copy()
    a = feat[..., 6:9].copy()
    gx = np.zeros((H, W), F)
    gy = np.zeros((H, W), F)
    if W > 1:
        gx[:, 0] = z[:, 1] - z[:, 0]
        gx[:, W - 1] = z[:, W - 1] - z[:, W - 2]
        gx[:, 1:W - 1] = (z[:, 2:] - z[:, :W - 2]) * F(0.5)
    if H > 1:
        gy[0] = z[1] - z[0]
        gy[H - 1] = z[H - 1] - z[H - 2]
        gy[1:H - 1] = (z[2:] - z[:H - 2]) * F(0.5)
    c = _demod(rgb, a) if demodulate else rgb.copy()
    var = np.zeros((H, W), F)
    if rgb_half is not None:
        h = np.asarray(rgb_half, F)
        dl = (lum(_demod(rgb, a)) - lum(_demod(h, a))) if demodulate else (lum(rgb) - lum(h))
        d2 = dl * dl
        sw = np.zeros((H, W), F)
        sv = np.zeros((H, W), F)
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                b = F((2.0 if i == 0 else 1.0) * (2.0 if j == 0 else 1.0))
                q, valid = _shift(d2, j, i)
                sw = sw + np.where(valid, b, F(0))
                sv = sv + np.where(valid, b * q, F(0))
        var = sv / sw
    return dict(n=n, z=z, a=a, gx=gx, gy=gy, c=c, var=var)


def level(g, c, var, k, use_var, sigma_luminance, sigma_normal, sigma_depth, sigma_albedo):
    """k_dn_level at step 2^k: (filtered signal, its variance)."""
    step = 1 << k
    n, z, a, gx, gy = g["n"], g["z"], g["a"], g["gx"], g["gy"]
    pzero = (n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0)
    lp = lum(c)
    if use_var:
        den_l = F(sigma_luminance) * np.sqrt(np.maximum(F(0), var)) + F(1e-4)
    else:
        den_l = np.full(lp.shape, F(sigma_luminance) * F(2.0 ** -k), F)
    sw = np.zeros(lp.shape, F)
    sc = np.zeros(c.shape, F)
    sv = np.zeros(lp.shape, F)
    with np.errstate(all="ignore"):
        for j in range(-2, 3):
            for i in range(-2, 3):
                cq, valid = _shift(c, j * step, i * step)
                nq, _ = _shift(n, j * step, i * step)
                zq, _ = _shift(z, j * step, i * step)
                aq, _ = _shift(a, j * step, i * step)
                vq, _ = _shift(var, j * step, i * step)
                h = B3[i + 2] * B3[j + 2]
                qzero = (nq[..., 0] == 0) & (nq[..., 1] == 0) & (nq[..., 2] == 0)
                dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                wn = np.power(np.maximum(F(0), dot), F(sigma_normal))
                wn = np.where(pzero | qzero, np.where(pzero & qzero, F(1), F(0)), wn).astype(F)
                wz = np.exp(-np.abs(z - zq) / (F(sigma_depth) * np.abs(gx * F(i * step) + gy * F(j * step)) + F(1e-4)))
                da = (np.abs(a[..., 0] - aq[..., 0]) + np.abs(a[..., 1] - aq[..., 1])) + np.abs(a[..., 2] - aq[..., 2])
                wa = np.exp(-da / F(sigma_albedo))
                wl = np.exp(-np.abs(lp - lum(cq)) / den_l)
                w = (((h * wn) * wz) * wa) * wl
                w = np.where(valid, w, F(0)).astype(F)
                sw = sw + w
                sc = sc + w[..., None] * (cq - c)
                sv = sv + (w * w) * np.where(valid, vq, F(0))
        ok = sw > 0
        out_c = np.where(ok[..., None], c + sc / np.where(ok, sw, F(1))[..., None], c).astype(F)
        out_v = np.where(ok, sv / np.where(ok, sw * sw, F(1)), var).astype(F)
    return out_c, out_v


def denoise(rgb, feat, rgb_half=None, **params):
    """The whole filter: float32 [H, W, 3]."""
    p = dict(DEFAULTS)
    p.update(params)
    g = prepare(rgb, feat, rgb_half, p["demodulate"])
    c, var = g["c"], g["var"]
    for k in range(p["levels"]):
        c, var = level(g, c, var, k, rgb_half is not None, p["sigma_luminance"], p["sigma_normal"], p["sigma_depth"], p["sigma_albedo"])
    if p["demodulate"]:
        c = c * np.maximum(g["a"], F(1e-3))
    return c.astype(F)
