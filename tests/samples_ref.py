"""A float32 numpy restatement of the resumable frames' state (include/frayhip.h "resumable frames"): what k_acc_resolve* add per sample and what
k_acc_mean makes of it.  Every operation is one float32 operation in the header's order; nothing is fused or reassociated."""
import numpy as np

F32 = np.float32


def luminance(c):
    """((r + g) + b) / 3.0f"""
    c = np.asarray(c, F32)
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / F32(3.0)


def accumulate(colours, state=None):
    """colours float32 [n, H, W, 3], the samples in order; state float32 [H, W, 4] of the samples before them, or None to start as the frame's
    sum does, at zero.  Returns the new state (the input is left as it is)."""
    colours = np.asarray(colours, F32)
    assert colours.ndim == 4 and colours.shape[-1] == 3 and colours.dtype == F32
    out = np.zeros(colours.shape[1:3] + (4,), F32) if state is None else np.array(state, F32, copy=True)
    for c in colours:
        out[..., :3] = out[..., :3] + c
        l = luminance(c)
        out[..., 3] = out[..., 3] + l * l
    return out


def mean_and_noise(state, N):
    """(rgb [H, W, 3], noise [H, W]) of a state holding N >= 1 samples."""
    state = np.asarray(state, F32)
    n = F32(N)
    assert int(n) == N and N >= 1
    rgb = state[..., :3] / n
    lbar = luminance(rgb)
    if N == 1:
        return rgb, lbar * lbar
    v = np.fmax(F32(0.0), state[..., 3] / n - lbar * lbar)          # fmaxf: a NaN difference gives 0
    return rgb, v / F32(N - 1)
