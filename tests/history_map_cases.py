"""Synthetic frames for tests/test_history_map_abi.py and tests/test_gpu_history_map.py: a small world seen by a pinhole camera looking along
+z -- a far wall z = 10, a near slab z = 6 over a range of world x (so a sideways move of the camera uncovers wall that was never seen), and
sky (a miss: zero position, normal and depth) above a world height -- sampled at the pixel centres (film_offset 0.5)."""
import numpy as np

F = np.float32
SIZES = [(37, 29), (1, 1), (1, 300)]           # W, H: a partial 256-thread block and partial 16x16 tiles; one pixel; one column


def view(W, H, cam_x=0.0, tan=0.5):
    return dict(pos=(cam_x, 0.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), front=(0.0, 0.0, 1.0), tan_x=tan, tan_y=tan * H / W, width=W, height=H)


def ctypes_view(abi, v):
    out = abi.View()
    for k in ("pos", "right", "up", "front"):
        for i in range(3):
            getattr(out, k)[i] = v[k][i]
    out.tan_x, out.tan_y, out.width, out.height = v["tan_x"], v["tan_y"], v["width"], v["height"]
    return out


def frame(W, H, cam_x=0.0, tan=0.5, seed=0):
    """(rgb [H, W, 3], feat [H, W, 10], view dict) of the world from a camera at (cam_x, 0, 0)."""
    v = view(W, H, cam_x, tan)
    xs = ((np.arange(W) + 0.5) / W * 2 - 1) * v["tan_x"]
    ys = (1 - (np.arange(H) + 0.5) / H * 2) * v["tan_y"]
    dx, dy = np.meshgrid(xs, ys)
    slab = np.abs(cam_x + 6.0 * dx - 1.0) <= 1.2                       # the slab covers world x in [-0.2, 2.2] at z = 6
    depth = np.where(slab, 6.0, 10.0)
    P = np.stack([cam_x + depth * dx, depth * dy, depth], axis=-1)
    sky = ~slab & (P[..., 1] > 0.35 * 10.0 * v["tan_y"])               # the top of the wall is sky
    feat = np.zeros((H, W, 10), F)
    feat[..., 0:3] = P
    feat[..., 3:6] = (0.0, 0.0, -2.0)                                  # not unit length: the kernels scale it
    feat[..., 6:9] = np.where(slab[..., None], (0.8, 0.3, 0.2), (0.5, 0.5, 0.6))
    feat[..., 9] = np.sqrt(((P - np.array([cam_x, 0.0, 0.0])) ** 2).sum(-1))
    feat[sky] = 0
    feat[sky, 6:9] = 1.0
    rgb = np.random.default_rng(seed).uniform(0.05, 1.0, (H, W, 3)).astype(F)
    return rgb, feat, v


def pair(W, H, seed=0):
    """Two frames of the world: the second from a camera moved sideways by about 2.3 pixels of the wall (for W = 1 by a twentieth of a pixel,
    so that the one column stays on the slab and still finds history)."""
    step = 2.3 * (2 * 10.0 * 0.5 / W) if W > 1 else 0.05 * (2 * 10.0 * 0.5)
    return frame(W, H, 0.0, seed=seed), frame(W, H, step, seed=seed + 1)


def motion_frame(feat, seed=0):
    """A motion frame [H, W, 8] for feat: P' and n' the feature's own, but in a patch the point moved a little inside its plane."""
    H, W = feat.shape[:2]
    m = np.zeros((H, W, 8), F)
    m[..., 0:3] = feat[..., 0:3]
    m[..., 4:7] = feat[..., 3:6]
    patch = np.zeros((H, W), bool)
    patch[H // 3:H // 3 + max(1, H // 4), W // 4:W // 4 + max(1, W // 3)] = True
    patch &= np.any(feat[..., 3:6] != 0, axis=-1)
    m[patch, 0] += F(0.4)
    m[patch, 3] = 1.0
    return m
