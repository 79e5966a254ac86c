"""A numpy restatement of the motion frame (include/frayhip.h "motion frames", fray_amd/csrc/features_variant.hip) and of the accumulation
through it (frayhip_temporal_accumulate_motion, fray_amd/csrc/temporal.hip).

motion_from_hits   one sample's motion row from a hit record, in float64 and in the order the header writes: each vector-matrix product is
                   (v.x m[0][j] + v.y m[1][j]) + v.z m[2][j], the subtraction and the addition component-wise, nothing contracted.
accumulate         tests/temporal_ref.py's accumulate with step 2 on P' and n': the same functions (project, unit_normals, dot, lum, is_zero,
                   spatial_variance), the same taps in the same order, float32 throughout.
Used by tests/test_motion_abi.py (synthetic inputs) and tests/test_gpu_motion.py (the device kernels against it, bit for bit)."""
import numpy as np

from temporal_ref import DEFAULTS, F, HISTORY_CHANNELS, dot, is_zero, lum, project, spatial_variance, unit_normals, view_fields

MOTION_CHANNELS = 8


def transform_arrays(T):
    """A sequence of frayhip_transform records (ctypes) as float64 arrays: offset [n, 3], m [n, 3, 3], invM [n, 3, 3] (row-major)."""
    n = len(T)
    off = np.array([[T[i].offset[k] for k in range(3)] for i in range(n)], np.float64).reshape(n, 3)
    m = np.array([[T[i].m[k] for k in range(9)] for i in range(n)], np.float64).reshape(n, 3, 3)
    inv = np.array([[T[i].invM[k] for k in range(9)] for i in range(n)], np.float64).reshape(n, 3, 3)
    return off, m, inv


def moved_nodes(nodes_now, prev_T):
    """Node i is moved when any of the 21 doubles of its transform differs by bit pattern."""
    a, b = transform_arrays(nodes_now), transform_arrays(prev_T)
    n = len(a[0])
    bits = lambda t: np.concatenate([x.reshape(n, -1) for x in t], axis=1).view(np.uint64)
    return np.any(bits(a) != bits(b), axis=1) if n else np.zeros(0, bool)


def vec_mat(v, m):
    """Vector * Matrix of matrix.h:53-60 on v [..., 3] and m [..., 3, 3]: (v.x m[0][j] + v.y m[1][j]) + v.z m[2][j]."""
    return (v[..., 0:1] * m[..., 0, :] + v[..., 1:2] * m[..., 1, :]) + v[..., 2:3] * m[..., 2, :]


def motion_from_hits(hit_id, hit_rec, nodes_now, prev_T):
    """The motion row of ONE sample per ray, float64 [..., 8]: hit_id and hit_rec as Scene.trace_rays(record=True) returns them (dist, ip,
    norm, u, v -- norm before any bump map), nodes_now and prev_T sequences of frayhip_transform (Scene.node_transforms())."""
    hit_id = np.asarray(hit_id)
    rec = np.asarray(hit_rec, np.float64)
    off_n, _m_n, inv_n = transform_arrays(nodes_now)
    off_p, m_p, _inv_p = transform_arrays(prev_T)
    moved = moved_nodes(nodes_now, prev_T)
    out = np.zeros(hit_id.shape + (MOTION_CHANNELS,), np.float64)
    hit = hit_id != -1                                       # a node or a rect light: the record's point and normal; a miss: zeros
    out[..., 0:3] = np.where(hit[..., None], rec[..., 1:4], 0.0)
    out[..., 4:7] = np.where(hit[..., None], rec[..., 4:7], 0.0)
    node = np.where(hit_id >= 0, hit_id, 0)
    mv = (hit_id >= 0) & moved[node] if len(moved) else np.zeros(hit_id.shape, bool)
    if mv.any():
        i = node[mv]
        ip, norm = rec[mv][:, 1:4], rec[mv][:, 4:7]
        out[mv, 0:3] = vec_mat(vec_mat(ip - off_n[i], inv_n[i]), m_p[i]) + off_p[i]
        out[mv, 4:7] = vec_mat(vec_mat(norm, inv_n[i]), m_p[i])
        out[mv, 3] = 1.0
    return out


def accumulate(rgb, feat, motion, prev_view=None, hist_in=None, **params):
    """frayhip_temporal_accumulate_motion: (hist_out [H, W, 12], signal [H, W, 3], variance [H, W]), float32."""
    p = dict(DEFAULTS)
    p.update(params)
    assert (prev_view is None) == (hist_in is None)
    rgb, feat, motion = np.asarray(rgb, F), np.asarray(feat, F), np.asarray(motion, F)
    H, W = rgb.shape[:2]
    assert motion.shape == (H, W, MOTION_CHANNELS)
    P = feat[..., 0:3]
    n = unit_normals(feat)
    Q = motion[..., 0:3]                                     # P'
    m = unit_normals(motion[..., 1:7])                       # n' (channels 4..6), scaled the way the normal is
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
            ok = ~is_zero(n) & ~is_zero(m) & (zc > 0) & (x0f >= F(-1)) & (x0f <= F(W - 1)) & (y0f >= F(-1)) & (y0f <= F(H - 1))
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
                    tap = inside & ~is_zero(nq) & (dot(m, nq) >= F(p["normal_min_dot"])) & (np.abs(dot(Pq - Q, m)) <= tol)
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
        hist[..., 4:7], hist[..., 7] = P, m1                 # the CURRENT position and unit normal
        hist[..., 8:11], hist[..., 11] = n, m2
        var = np.maximum(F(0), m2 - m1 * m1)
        vh = F(p["variance_history"])
        young = N < vh
        if young.any():
            var = np.where(young, spatial_variance(hist, z, p["plane_tolerance"], p["normal_min_dot"]) * (vh / N), var)
    return hist, acc.copy(), var.astype(F)
