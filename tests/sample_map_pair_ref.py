"""k_sample_map<PAIR> (fray_amd/csrc/samplemap.hip, include/frayhip.h "sample maps": frayhip_sample_map_pair) restated in numpy: every operation in
float32, in the order the header writes it, so that the kernel and this file agree bit for bit.  Per component the mean luminance and the noise
estimate of tests/sample_map_ref.py; the two are added, and from `ref` on the rule is that file's."""
import numpy as np

F = np.float32


def _component(state, N, fn):
    """lbar and noise of one state's rows at the pixels' own N."""
    mean = state[..., :3] / fn[..., None]
    lbar = ((mean[..., 0] + mean[..., 1]) + mean[..., 2]) / F(3.0)
    v = np.fmax(F(0), state[..., 3] / fn - lbar * lbar)                          # fmaxf: a NaN operand gives the other one
    noise = np.where(N >= 2, v / (N - 1).astype(F), lbar * lbar).astype(F)
    return lbar.astype(F), noise


def sample_map_pair_ref(direct, indirect, count, tolerance=0.05, lum_floor=0.01, min_count=4, max_count=None, max_add=1 << 24, grow=2):
    """direct, indirect float32 [H, W, 4], count int32 [H, W] -> (add int32 [H, W], pixels, samples)."""
    assert max_count is not None and 1 <= min_count <= max_count <= 1 << 24 and max_add >= 1 and 2 <= grow <= 16
    direct, indirect = np.asarray(direct, F), np.asarray(indirect, F)
    N = np.asarray(count, np.int32).astype(np.int64)
    with np.errstate(all="ignore"):
        fn = N.astype(F)
        lbar_d, noise_d = _component(direct, N, fn)
        lbar_i, noise_i = _component(indirect, N, fn)
        lbar = (lbar_d + lbar_i).astype(F)
        noise = (noise_d + noise_i).astype(F)
        ref = np.fmax(lbar, F(lum_floor))
        t = F(tolerance) * ref
        need = np.ceil(fn * (noise / (t * t))).astype(F)
        fits = need <= F(max_count)                                              # false for a NaN need: it asks for max_count
        as_int = np.where(fits, need, F(0)).astype(np.int64)
        target = np.where(fits, np.maximum(N, as_int), max_count)
        target = np.minimum(target, grow * N)
    target = np.where(N < min_count, min_count, target)
    add = np.minimum(np.minimum(target, max_count) - N, max_add)
    add = np.where(N >= max_count, 0, add).astype(np.int32)
    return add, int((add > 0).sum()), int(add[add > 0].sum())
