"""The numpy restatement of split temporal accumulation (include/frayhip.h "split temporal accumulation", fray_amd/csrc/temporal_split.hip).

accumulate_split IS the contract: the two existing restatement calls (tests/temporal_ref.py, or tests/motion_ref.py with a motion frame), one per
component on that component's part of the history, packed into the 20-channel layout.  The fused kernels must give the same bits.
Also the synthetic five-frame chain that tests/test_temporal_split_abi.py (the packing) and tests/test_gpu_temporal_split.py (the kernels) share."""
import numpy as np

import motion_ref
import temporal_ref

F = np.float32
HISTORY_SPLIT_CHANNELS = 20
SHARED = ("demodulate", "film_offset", "plane_tolerance", "normal_min_dot")


def split_parts(hist):
    """(direct [H, W, 12], indirect [H, W, 12]) of a split history: rows 0-2 as they stand; {row 3}, {P, m1_I}, {n, m2_I}."""
    hist = np.asarray(hist, F)
    assert hist.shape[2] == HISTORY_SPLIT_CHANNELS
    hi = np.concatenate([hist[..., 12:16], hist[..., 4:7], hist[..., 16:17], hist[..., 8:11], hist[..., 17:18]], axis=2)
    return np.ascontiguousarray(hist[..., 0:12]), hi


def join_parts(hd, hi):
    """The split history of two ordinary histories of one frame (their position and normal columns are the same bits)."""
    assert hd[..., 4:7].tobytes() == hi[..., 4:7].tobytes() and hd[..., 8:11].tobytes() == hi[..., 8:11].tobytes()
    out = np.zeros(hd.shape[:2] + (HISTORY_SPLIT_CHANNELS,), F)
    out[..., 0:12] = hd
    out[..., 12:16] = hi[..., 0:4]
    out[..., 16], out[..., 17] = hi[..., 7], hi[..., 11]
    return out


def accumulate_split(rgb_direct, rgb_indirect, feat, prev_view=None, hist_in=None, motion=None, direct=None, indirect=None, **shared):
    """frayhip_temporal_accumulate_split: (hist_out [H, W, 20], signal_direct, signal_indirect, variance_direct, variance_indirect)."""
    pd, pi = dict(shared, **(direct or {})), dict(shared, **(indirect or {}))
    for k in SHARED:
        assert pd.get(k, temporal_ref.DEFAULTS[k]) == pi.get(k, temporal_ref.DEFAULTS[k]), k
    hin_d, hin_i = split_parts(hist_in) if hist_in is not None else (None, None)
    if motion is None:
        hd, sd, vd = temporal_ref.accumulate(rgb_direct, feat, prev_view, hin_d, **pd)
        hi, si, vi = temporal_ref.accumulate(rgb_indirect, feat, prev_view, hin_i, **pi)
    else:
        hd, sd, vd = motion_ref.accumulate(rgb_direct, feat, motion, prev_view, hin_d, **pd)
        hi, si, vi = motion_ref.accumulate(rgb_indirect, feat, motion, prev_view, hin_i, **pi)
    return join_parts(hd, hi), sd, si, vd, vi


# ---- the synthetic chain ------------------------------------------------------------------------------------------------------------------------
CHAIN_W, CHAIN_H = 37, 23                # 851 pixels: no multiple of 256, and neither side a multiple of 16 (ragged variance tiles)
CHAIN_CAMERA_X = (0.0, 0.0, 1.5, 1.5, -2.25)          # in pixel widths
CHAIN_DIRECT = dict(max_history=2, variance_history=1, alpha_min=0.3)
CHAIN_INDIRECT = dict(max_history=32, variance_history=4, alpha_min=0.05)
DEPTH, TAN = 10.0, 0.5
PIXEL_WIDTH = 2.0 * DEPTH * TAN / CHAIN_W


def plane_frame(W, H, cam_x=0.0, depth=DEPTH, tan=TAN, normal=(0.0, 0.0, -1.0), albedo=(0.5, 0.5, 0.5), offset=0.5):
    """A fronto-parallel plane z = depth seen by a camera at (cam_x, 0, 0) looking along +z: (feat, view dict); pixel i sampled at film i + offset
    (tests/test_temporal_abi.py's _plane_frame)."""
    view = dict(pos=(cam_x, 0.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), front=(0.0, 0.0, 1.0), tan_x=tan, tan_y=tan * H / W, width=W, height=H)
    xs = (np.arange(W) + offset) / W * 2 - 1
    ys = 1 - (np.arange(H) + offset) / H * 2
    feat = np.zeros((H, W, 10), F)
    feat[..., 0] = cam_x + depth * tan * xs[None, :]
    feat[..., 1] = depth * (tan * H / W) * ys[:, None]
    feat[..., 2] = depth
    feat[..., 3:6] = normal
    feat[..., 6:9] = albedo
    feat[..., 9] = np.sqrt(((feat[..., 0:3] - np.array([cam_x, 0, 0], F)) ** 2).sum(-1))
    return feat, view


def chain_frames(with_motion=False):
    """The five frames of the chain: [(rgb_direct, rgb_indirect, feat, view dict, motion or None)].  Image rows 0-4 are a miss (zero position,
    normal and depth); in frame 3 the columns >= 20 have the normal (1, 0, 0).  with_motion: P' is P one pixel width further along x in columns
    8-15, n' = n, both as feat's elsewhere, and n' exactly zero in columns 30 and 31."""
    rng = np.random.default_rng(20)
    frames = []
    for k, cx in enumerate(CHAIN_CAMERA_X):
        feat, view = plane_frame(CHAIN_W, CHAIN_H, cam_x=cx * PIXEL_WIDTH, albedo=(0.5, 0.25, 0.75))
        if k == 3:
            feat[:, 20:, 3:6] = (1.0, 0.0, 0.0)
        feat[0:5, :, 0:6] = 0.0
        feat[0:5, :, 9] = 0.0
        rgb_d = rng.uniform(0.0, 1.0, (CHAIN_H, CHAIN_W, 3)).astype(F)
        rgb_i = rng.uniform(0.0, 2.0, (CHAIN_H, CHAIN_W, 3)).astype(F)
        motion = None
        if with_motion:
            motion = np.zeros((CHAIN_H, CHAIN_W, 8), F)
            motion[..., 0:3], motion[..., 4:7] = feat[..., 0:3], feat[..., 3:6]
            motion[5:, 8:16, 0] += F(PIXEL_WIDTH)
            motion[5:, 8:16, 3] = 1.0
            motion[:, 30:32, 4:7] = 0.0
        frames.append((rgb_d, rgb_i, feat, view, motion))
    return frames
