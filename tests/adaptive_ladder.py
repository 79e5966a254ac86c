"""A numpy restatement of adaptive frames (include/frayhip.h "adaptive frames"): the ladder of sample counts, the per-pixel error and the stop rule.
Given the fixed-spp frames F_r of every rung r, it yields the image, sample-count map and error map an adaptive call must produce, bit for bit."""
import numpy as np


def ladder(min_spp, spp):
    """r_0 = floor(min_spp / 2), r_1 = min_spp, r_{j+1} = min(2 r_j, spp), ending at the first rung equal to spp."""
    assert 2 <= min_spp <= spp
    r = [min_spp // 2, min_spp]
    while r[-1] < spp:
        r.append(min(2 * r[-1], spp))
    return r


def rung_error(m, h, err_floor):
    """err = ((|m.r - h.r| + |m.g - h.g|) + |m.b - h.b|) / (err_floor + ((m.r + m.g) + m.b)), in double, each float32 operand widened first."""
    m = np.asarray(m, np.float32).astype(np.float64)
    h = np.asarray(h, np.float32).astype(np.float64)
    d = np.abs(m - h)
    num = (d[..., 0] + d[..., 1]) + d[..., 2]
    den = np.float64(err_floor) + ((m[..., 0] + m[..., 1]) + m[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den


def expected(frames, min_spp, spp, threshold, err_floor):
    """frames: {r: float32 [H, W, 3]} for every rung r of the ladder.  Returns (rgb float32 [H, W, 3], spp int32 [H, W], err float32 [H, W]):
    each pixel stops at the first rung j >= 1 with err <= threshold (a NaN error never does) or r_j == spp."""
    rs = ladder(min_spp, spp)
    first = np.asarray(frames[rs[0]], np.float32)
    H, W = first.shape[:2]
    rgb = np.zeros((H, W, 3), np.float32)
    spp_map = np.zeros((H, W), np.int32)
    err_map = np.zeros((H, W), np.float32)
    active = np.ones((H, W), bool)
    for j in range(1, len(rs)):
        m = np.asarray(frames[rs[j]], np.float32)
        err = rung_error(m, frames[rs[j - 1]], err_floor)
        stop = active & ((err <= threshold) | (rs[j] == spp))
        rgb[stop] = m[stop]
        spp_map[stop] = rs[j]
        err_map[stop] = err[stop].astype(np.float32)
        active &= ~stop
    assert not active.any()
    return rgb, spp_map, err_map


def rung1_threshold(frames, min_spp, spp, err_floor, q=0.5):
    """A threshold at quantile q of the finite rung-1 errors: with q near the middle some pixels stop at min_spp and the others climb."""
    rs = ladder(min_spp, spp)
    e = rung_error(frames[rs[1]], frames[rs[0]], err_floor)
    return float(np.quantile(e[np.isfinite(e)], q))
