"""frayhip_sample_map_budget (include/frayhip.h "sample maps") restated on top of sample_map_ref / sample_map_pair_ref: the three stages of a
frame-wide sample budget, found by plain two-way bisection -- at most 31 evaluations of the map for the tolerance's bit pattern, at most
log2(max_add) + 1 for the cap.  Deliberately a different search from the kernels' 16-way one (fray_amd/csrc/budget_search.hpp): the two must agree
because the sum of a map does not increase with the tolerance, not because they walk alike."""
import numpy as np

from sample_map_pair_ref import sample_map_pair_ref
from sample_map_ref import sample_map_ref

F = np.float32
TOL_MAX = np.finfo(np.float32).max


def bits_of(tolerance):
    return int(np.array(tolerance, F).view(np.uint32))


def float_of(bits):
    return np.array(bits, np.uint32).view(F)[()]


def _map(state, count, tolerance, params):
    """add of the state (a pair: of both) at `tolerance`, everything else from params."""
    params = dict(params, tolerance=tolerance)
    if isinstance(state, (tuple, list)):
        return sample_map_pair_ref(state[0], state[1], count, **params)[0]
    return sample_map_ref(state, count, **params)[0]


def sample_map_budget_ref(state, count, budget, **params):
    """state float32 [H, W, 4] or a pair of them, count int32 [H, W], budget int >= 0 -> (add int32 [H, W], info) with info's pixels, samples,
    demand, tolerance_used (float32), cap_used and stage."""
    budget = int(budget)
    tol0 = F(params.get("tolerance", 0.05))
    max_add = int(params.get("max_add", 1 << 24))
    total = lambda add: int(add.astype(np.int64).sum())
    first = _map(state, count, tol0, params)
    demand = total(first)
    evaluations = 0
    if demand <= budget:
        add, tol, cap, stage = first, tol0, -1, 0
    else:
        last = _map(state, count, TOL_MAX, params)
        if total(last) <= budget:
            lo, hi = bits_of(tol0), bits_of(TOL_MAX)            # S(lo) > budget >= S(hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                evaluations += 1
                if total(_map(state, count, float_of(mid), params)) <= budget:
                    hi = mid
                else:
                    lo = mid
            assert evaluations <= 31
            tol, cap, stage = float_of(hi), -1, 1
            add = _map(state, count, tol, params)
        else:
            capped = lambda c: np.minimum(last, c).astype(np.int32)
            lo, hi = 0, max_add                                 # T(lo) <= budget < T(hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                evaluations += 1
                if total(capped(mid)) <= budget:
                    lo = mid
                else:
                    hi = mid
            assert evaluations <= max((max_add - 1).bit_length(), 1)        # 24 for the default max_add
            tol, cap, stage = TOL_MAX, lo, 2
            add = capped(cap)
    info = {"pixels": int((add > 0).sum()), "samples": total(add), "budget": budget, "demand": demand, "tolerance_used": F(tol), "cap_used": cap,
            "stage": stage}
    assert info["samples"] <= budget
    return add, info
