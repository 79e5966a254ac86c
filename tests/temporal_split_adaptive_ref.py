"""The numpy restatement of adaptive split accumulation (include/frayhip.h "change frames", frayhip_temporal_accumulate_split_adaptive;
fray_amd/csrc/temporal_split.hip).

accumulate_split_adaptive IS the contract: two calls of the adaptive restatement (tests/change_ref.py), one per component on that component's
part of the split history and with that component's change frame, packed into the 20-channel layout.  The fused kernels must give the same bits.
Also the synthetic chain of tests/temporal_split_ref.py with one change map per component and frame, computed once per (motion, demodulate) and
shared by tests/test_temporal_split_adaptive_abi.py and tests/test_gpu_temporal_split_adaptive.py."""
import functools

import numpy as np

import change_ref
import temporal_split_ref as split_ref
from test_gpu_change import CHANGE_VALUES, _change_map

F = np.float32
# both components have a window to return to, and histories long enough to be shortened on either side of it
CHAIN_DIRECT = dict(max_history=6, variance_history=3, alpha_min=0.3)
CHAIN_INDIRECT = split_ref.CHAIN_INDIRECT
NAMES = ("hist_out", "signal_direct", "signal_indirect", "variance_direct", "variance_indirect")
BRANCHES = ("keep", "part", "cut")


def accumulate_split_adaptive(rgb_direct, rgb_indirect, feat, change_direct, change_indirect, prev_view=None, hist_in=None, motion=None, direct=None,
                              indirect=None, **shared):
    """frayhip_temporal_accumulate_split_adaptive: (hist_out [H, W, 20], signal_direct, signal_indirect, variance_direct, variance_indirect)."""
    pd, pi = dict(shared, **(direct or {})), dict(shared, **(indirect or {}))
    for k in split_ref.SHARED:
        assert pd.get(k, change_ref.DEFAULTS[k]) == pi.get(k, change_ref.DEFAULTS[k]), k
    hin_d, hin_i = split_ref.split_parts(hist_in) if hist_in is not None else (None, None)
    hd, sd, vd = change_ref.accumulate(rgb_direct, feat, change_direct, motion, prev_view, hin_d, **pd)
    hi, si, vi = change_ref.accumulate(rgb_indirect, feat, change_indirect, motion, prev_view, hin_i, **pi)
    return split_ref.join_parts(hd, hi), sd, si, vd, vi


def branch(g):
    """Which of the header's three cases a change value takes, as an index into BRANCHES."""
    g = np.asarray(g, F)
    with np.errstate(invalid="ignore"):
        cut = ~(g < F(1))
        part = ~cut & (g > 0)
    return np.where(cut, 2, np.where(part, 1, 0))


def chain_change_maps(k, shape):
    """The chain's change maps of frame k: (direct, indirect), tests/test_gpu_change.py's _change_map with seeds 100 + k and 200 + k."""
    return _change_map(k, shape), _change_map(100 + k, shape)


def _frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def chain(with_motion, demodulate):
    """The five frames of split_ref.chain_frames(with_motion) accumulated with chain_change_maps, each frame onto the restatement's own history:
    a list of dicts with the inputs (rgb_d, rgb_i, feat, view, motion, chg_d, chg_i, prev_view, hist_in), `ref` (the five outputs), `plain` (the
    split restatement on the same inputs: change frames of +0) and `fetched` [H, W] bool (the pixels that fetched a history: there the plain
    N is min(N_hist + 1, max_history) >= 2, and 1 everywhere else).  Read-only arrays: computed once, shared."""
    D, I = CHAIN_DIRECT, CHAIN_INDIRECT
    out = []
    hist = view = None
    for k, (rgb_d, rgb_i, feat, v, motion) in enumerate(split_ref.chain_frames(with_motion)):
        chg_d, chg_i = chain_change_maps(k, rgb_d.shape[:2])
        ref = accumulate_split_adaptive(rgb_d, rgb_i, feat, chg_d, chg_i, view, hist, motion=motion, direct=D, indirect=I, demodulate=demodulate)
        plain = split_ref.accumulate_split(rgb_d, rgb_i, feat, view, hist, motion=motion, direct=D, indirect=I, demodulate=demodulate)
        fetched = plain[0][..., 3] > 1
        assert np.array_equal(fetched, plain[0][..., 15] > 1)               # the components share the taps
        fr = dict(rgb_d=rgb_d, rgb_i=rgb_i, feat=feat, view=v, motion=motion, chg_d=chg_d, chg_i=chg_i, prev_view=view, hist_in=hist,
                  ref=tuple(_frozen(a) for a in ref), plain=tuple(_frozen(a) for a in plain), fetched=_frozen(fetched))
        for key in ("rgb_d", "rgb_i", "feat", "motion", "chg_d", "chg_i"):
            _frozen(fr[key])
        out.append(fr)
        hist, view = ref[0], v
    return out


def chain_coverage(frames):
    """What the chain exercises, from the restatement alone: per frame the set of (direct branch, indirect branch) pairs among the pixels that
    fetched a history, and per component the counts (young, old) of histories that were shortened (0 < g < 1, N > 1) and ended below / not below
    that component's variance_history."""
    pairs = []
    count = {"direct": [0, 0], "indirect": [0, 0]}
    for fr in frames:
        bd, bi = branch(fr["chg_d"]), branch(fr["chg_i"])
        f = fr["fetched"]
        pairs.append(set(zip(bd[f].tolist(), bi[f].tolist())))
        for name, b, N, vh in (("direct", bd, fr["ref"][0][..., 3], CHAIN_DIRECT["variance_history"]),
                               ("indirect", bi, fr["ref"][0][..., 15], CHAIN_INDIRECT["variance_history"])):
            lowered = (b == 1) & (N > 1)
            count[name][0] += int((lowered & (N < vh)).sum())
            count[name][1] += int((lowered & (N >= vh)).sum())
    return pairs, count


def cyclic_change_maps(shape, shift):
    """Change maps that hold CHANGE_VALUES in turn along the flattened image, from `shift` on: (direct, indirect); the indirect map runs four
    values ahead, so that the components take different cases in a pixel."""
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    return CHANGE_VALUES[(idx + shift) % len(CHANGE_VALUES)].copy(), CHANGE_VALUES[(idx + shift + 4) % len(CHANGE_VALUES)].copy()
