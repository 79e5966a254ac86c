"""A numpy restatement of the history map (include/frayhip.h "weighted accumulation and history maps", frayhip_history_map), written from the
header's text.  The fetch is tests/temporal_weighted_ref.py's -- the header says `held` is exactly the weighted entry's hu -- and the search for
the target is the definition itself: S(t) summed over the pixels for every t, no histogram.

held          the units each pixel's reprojected history holds, float32 [H, W]
units         units(t) per pixel for a target t, int64 [H, W]
total         S(t), a Python integer
history_map   frayhip_history_map: (add int32 [H, W], weight float32 [H, W], held float32 [H, W], info)
Used by tests/test_history_map_abi.py (synthetic inputs) and tests/test_gpu_history_map.py (the device kernels against it, all equal)."""
import numpy as np

import temporal_weighted_ref
from temporal_ref import DEFAULTS, F

NO_BUDGET = (1 << 64) - 1
MAP_DEFAULTS = dict(target=8, max_units=8, budget=NO_BUDGET)


def held(feat, prev_view=None, hist_in=None, units_in=None, motion=None, change=None, **params):
    p = dict(DEFAULTS)
    p.update(params)
    feat = np.asarray(feat, F)
    H, W = feat.shape[:2]
    if hist_in is None:
        return np.zeros((H, W), F)
    with np.errstate(all="ignore"):
        sb, _h, hu = temporal_weighted_ref.fetch(feat, prev_view, hist_in, units_in, motion, p)
        found = sb > 0
        hu = hu / np.where(found, sb, F(1))
        out = np.where(found, hu, F(0)).astype(F)
        if change is not None:
            g = np.where(found, np.asarray(change, F), F(0))
            out = np.where(found & ~(g < F(1)), F(0), np.where(found & (g > 0), hu * (F(1) - g), out)).astype(F)
        out = np.where(out >= 0, out, F(0)).astype(F)        # if (!(held >= 0)) held = 0
    return out


def whole_units(held_plane, max_history):
    """k = (int)floorf(fminf(held, max_history))."""
    return np.floor(np.fmin(np.asarray(held_plane, F), F(max_history))).astype(np.int64)


def units(k, t, max_units):
    return np.minimum(np.maximum(t - k, 1), max_units)


def total(k, t, base, max_units):
    return int(base) * int(units(k, t, max_units).sum())


def history_map(feat, prev_view=None, hist_in=None, units_in=None, motion=None, change=None, base=None, target=8, max_units=8, budget=None,
                **params):
    p = dict(DEFAULTS)
    p.update(params)
    budget = NO_BUDGET if budget is None else int(budget)
    hp = held(feat, prev_view, hist_in, units_in, motion, change, **params)
    k = whole_units(hp, p["max_history"])
    assert 1 <= target <= p["max_history"] and base >= 1 and max_units >= 1 and budget >= base * k.size
    used = max(t for t in range(1, target + 1) if total(k, t, base, max_units) <= budget)
    u = units(k, used, max_units)
    info = dict(target_used=used, samples=total(k, used, base, max_units), boosted=int((u > 1).sum()))
    return (base * u).astype(np.int32), u.astype(F), hp, info
