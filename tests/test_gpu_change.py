"""Change frames and gradient-adaptive accumulation on the GPU (include/frayhip.h "change frames"), every comparison bit for bit:
1. k_ch_frame against tests/change_ref.py on seeded states (host entry against the restatement, device entry against the host entry);
2. frayhip_temporal_accumulate_adaptive on the synthetic chain of tests/temporal_split_ref.py, with and without a motion frame, with change
   frames that hold every kind of value; a frame of +0 is the plain (or motion) entry and a frame of 1 the first-frame call;
3. rendered states: the pixels whose direct states an edit leaves bit-equal are the pixels where the oracle's frames of the original and of the
   edited scene are bit-equal, and the change frame is exactly zero there;
4. Scene.render_sequence(change_samples=2) against the same sequence without it."""
import os

import numpy as np
import pytest

import change_ref
import motion_ref
import scene_edits
import temporal_ref
import temporal_split_ref as split_ref
from conftest import open_scene
from denoise_ref import _shift

pytestmark = pytest.mark.gpu
F = np.float32


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _bits(a):
    return np.ascontiguousarray(_np(a)).view(np.uint32)


def _same(what, got, want):
    """Equal bit patterns, with the first differing value in the message."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    i = tuple(bad[0])
    raise AssertionError("%s: %d of %d values differ, first at %s: %r against %r" % (what, len(bad), g.size, i, g.view(F)[i], w.view(F)[i]))


def _pixels_equal(a, b):
    """[H, W] bool: the pixels all of whose channels have equal bit patterns."""
    a, b = _bits(a), _bits(b)
    e = a == b
    return e.reshape(e.shape[0], e.shape[1], -1).all(axis=2)


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _view(abi, v):
    out = abi.View()
    for k in ("pos", "right", "up", "front"):
        for i in range(3):
            getattr(out, k)[i] = v[k][i]
    out.tan_x, out.tan_y, out.width, out.height = v["tan_x"], v["tan_y"], v["width"], v["height"]
    return out


# ---- 1. k_ch_frame -----------------------------------------------------------------------------------------------------------------------------
def _states(W, H):
    """Seeded states with every kind of region (bands of rows and columns, so that a 5 x 3 image has them too): changed texels, identical
    rows, rows that are zero in both states, rows with inf and NaN sums, negative sums, and a motion frame whose `moved` covers a band."""
    rng = np.random.default_rng(1000 * W + H)
    before = rng.uniform(0.0, 4.0, (H, W, 4)).astype(F)
    after = rng.uniform(0.0, 4.0, (H, W, 4)).astype(F)
    before[:, W // 2:W // 2 + 2, 0:3] = -before[:, W // 2:W // 2 + 2, 0:3]          # la < 0 beside lb > 0: d > m; both < 0 in the identical rows
    after[1::3] = before[1::3]                          # identical rows: d = 0
    before[2::6] = 0.0                                  # all-zero rows: m = 0
    after[2::6] = 0.0
    cols = np.arange(W)
    special = np.array([np.inf, -np.inf, np.nan, -3.0, 3e38], F)
    for y in range(0, H, 5):                            # a row with non-finite and negative sums, on either side
        side = after if (y // 5) % 2 else before
        side[y, :, 1] = special[cols % len(special)]
    motion = rng.uniform(-1.0, 1.0, (H, W, 8)).astype(F)
    motion[..., 3] = 0.0
    motion[:, W // 3:W // 3 + max(1, W // 5), 3] = rng.choice(np.array([0.25, 0.5, 1.0], F), (H, max(1, W // 5)))
    if W > 4:
        motion[0, W - 1, 3] = -0.0                      # -0 is 0: not masked
    return before, after, motion


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (37, 19), (64, 48)])
def test_change_frame_matches_restatement(fray, gpu, W, H):
    before, after, motion = _states(W, H)
    tb, ta, tm = _cuda(before), _cuda(after), _cuda(motion)
    seen = dict(zero=0, part=0, one=0)
    for radius in range(4):
        for gain in (1.0, 2.5):
            for mot, tmot in ((None, None), (motion, tm)):
                what = "%dx%d radius %d gain %g %s" % (W, H, radius, gain, "with motion" if mot is not None else "no motion")
                ref = change_ref.change_frame(before, after, mot, radius=radius, gain=gain)
                got = fray.change_frame(before, after, mot, radius=radius, gain=gain)
                assert got.dtype == F and got.shape == (H, W)
                _same(what + ", host entry against the restatement", got, ref)
                dev = fray.change_frame(tb, ta, tmot, radius=radius, gain=gain)
                assert dev.is_cuda
                _same(what + ", device entry against host entry", dev, got)
                assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
                seen["zero"] += int((got == 0).sum())
                seen["part"] += int(((got > 0) & (got < 1)).sum())
                seen["one"] += int((got == 1).sum())
    if W * H > 1:
        assert all(seen.values()), seen                 # the inputs reach the zero, the ratio and the clamp
    # identical states: zero everywhere, whatever the window; Accumulation objects are taken as their states
    A = fray.Accumulation(before, 2), fray.Accumulation(before.copy(), 2)
    assert not fray.change_frame(A[0], A[1]).any()


# ---- 2. the adaptive entry on the synthetic chain ------------------------------------------------------------------------------------------------
CHANGE_VALUES = np.array([0.0, -0.0, -0.5, 0.01, 0.05, 0.3, 0.999, 1.0, 1.5, np.nan, np.inf], F)


def _change_map(k, shape):
    """Half the pixels +0, the others drawn from CHANGE_VALUES: +0, -0, a negative, values inside (0, 1), 1, above 1, NaN and inf."""
    rng = np.random.default_rng(100 + k)
    m = CHANGE_VALUES[rng.integers(0, len(CHANGE_VALUES), shape)]
    return np.where(rng.uniform(size=shape) < 0.5, F(0), m).astype(F)


@pytest.mark.parametrize("with_motion", [False, True])
@pytest.mark.parametrize("demodulate", [0, 1])
def test_adaptive_chain(fray, abi, gpu, with_motion, demodulate):
    I = dict(split_ref.CHAIN_INDIRECT, demodulate=demodulate)
    vh = I["variance_history"]
    hist = hist_t = hist_r = view = view_r = None
    young = old = 0
    kinds = set()
    for k, (_d, rgb, feat, v, motion) in enumerate(split_ref.chain_frames(with_motion)):
        shape = rgb.shape[:2]
        g = _change_map(k, shape)
        kinds |= set(np.unique(g.view(np.uint32)).tolist())
        ref = change_ref.accumulate(rgb, feat, g, motion, view_r, hist_r, **I)
        N = ref[0][..., 3]
        lowered = (g > 0) & (g < 1) & (N > 1)                               # a history was fetched and shortened
        young += int((lowered & (N < vh)).sum())
        old += int((lowered & (N >= vh)).sum())
        got = fray.temporal_accumulate(rgb, feat, view, hist, motion=motion, change=g, **I)
        for name, a, b in zip(("history", "signal", "variance"), got, ref):
            _same("chain frame %d %s, host entry against the restatement" % (k, name), a, b)
        dev = fray.temporal_accumulate(_cuda(rgb), _cuda(feat), view, hist_t, motion=_cuda(motion), change=_cuda(g), **I)
        for name, a, b in zip(("history", "signal", "variance"), dev, got):
            _same("chain frame %d %s, device entry against host entry" % (k, name), a, b)
        # P1: a change frame of +0 is the plain (or motion) entry, in every output bit
        plain = fray.temporal_accumulate(rgb, feat, view, hist, motion=motion, **I)
        zero = fray.temporal_accumulate(rgb, feat, view, hist, motion=motion, change=np.zeros(shape, F), **I)
        want = (motion_ref.accumulate(rgb, feat, motion, view_r, hist_r, **I) if with_motion else temporal_ref.accumulate(rgb, feat, view_r, hist_r, **I))
        for name, a, b, c in zip(("history", "signal", "variance"), zero, plain, want):
            _same("chain frame %d %s, P1: a change frame of +0 against the plain entry" % (k, name), a, b)
            _same("chain frame %d %s, the plain entry against its restatement" % (k, name), b, c)
        # P2: a change frame of 1 is the first-frame call
        one = fray.temporal_accumulate(rgb, feat, view, hist, motion=motion, change=np.ones(shape, F), **I)
        first = fray.temporal_accumulate(rgb, feat, None, None, motion=motion, **I)
        for name, a, b in zip(("history", "signal", "variance"), one, first):
            _same("chain frame %d %s, P2: a change frame of 1 against hist_in = NULL" % (k, name), a, b)
        hist, hist_t, hist_r, view, view_r = got[0], dev[0], ref[0], _view(abi, v), v
    assert kinds == set(CHANGE_VALUES.view(np.uint32).tolist())             # every kind of value was in some frame
    assert young > 0 and old > 0, (young, old)                              # shortened histories on both sides of variance_history


# ---- 3. rendered states ----------------------------------------------------------------------------------------------------------------------
W3, H3, SEED, NPROBE = 64, 48, 42, 2


def _oracle_unchanged(fray, abi, oracle, case, tmp_path):
    """[H, W] bool: where the oracle's maxTraceDepth = 0, NPROBE-spp frames of the case's original and of its edited scene (the edited text
    parsed afresh) are bit-equal."""
    over = dict(numPaths=NPROBE, maxTraceDepth=0)
    s = open_scene(fray, "cornell_box.fray", W3, H3, **over)
    a, _ = oracle.render(s.desc, abi.MODE_RENDER, seed=SEED)
    s.close()
    c = scene_edits.CASES[case]
    path = os.path.join(str(tmp_path), case + ".fray")
    with open(path, "w") as f:
        f.write(scene_edits.edited_text(c, scene_edits.scene_path(c, tmp_path), tmp_path))
    e = fray.Scene.parseScene(path)
    e.settings.frameWidth, e.settings.frameHeight = W3, H3
    for k, v in over.items():
        setattr(e.settings, k, v)
    b, _ = oracle.render(e.desc, abi.MODE_RENDER, seed=SEED)
    e.close()
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return _pixels_equal(a, b)


def _states_around_edit(fray, case):
    """The component states of samples [0, NPROBE) of the 8-spp cornell frame before and after the case's edit: ((direct, indirect) before,
    (direct, indirect) after), numpy."""
    s = open_scene(fray, "cornell_box.fray", W3, H3, numPaths=8)
    s.beginRender()
    _, _, before = s.render_components(NPROBE, seed=SEED)
    scene_edits.apply(fray, s, scene_edits.CASES[case]["edit"])
    s.update()
    _, _, after = s.render_components(NPROBE, seed=SEED)
    s.close()
    assert before[0].samples_done == after[0].samples_done == NPROBE
    return before, after


def test_rendered_block_edit_matches_the_oracle(fray, abi, gpu, oracle, tmp_path):
    unchanged = _oracle_unchanged(fray, abi, oracle, "cornell-block", tmp_path)
    n = int(unchanged.sum())
    print("oracle, cornell-block: %d of %d pixels bit-equal, %d changed" % (n, unchanged.size, unchanged.size - n))
    assert 2 * n >= unchanged.size and 20 * (unchanged.size - n) >= unchanged.size
    before, after = _states_around_edit(fray, "cornell-block")
    same = _pixels_equal(before[0].state, after[0].state)
    print("direct states: %d pixels bit-equal; %d pixels where the two sets differ" % (int(same.sum()), int((same != unchanged).sum())))
    assert np.array_equal(same, unchanged)
    chg = fray.change_frame(before[0], after[0], radius=0)
    _same("radius 0, host entry against the restatement", chg, change_ref.change_frame(before[0].state, after[0].state, radius=0))
    assert not chg[unchanged].any()                      # exactly zero where nothing changed
    assert (chg[~unchanged] > 0).any()
    wide = fray.change_frame(before[0], after[0])
    _same("defaults, host entry against the restatement", wide, change_ref.change_frame(before[0].state, after[0].state))
    print("change > 0: %d pixels at radius 0, %d at radius 3" % (int((chg > 0).sum()), int((wide > 0).sum())))
    # indirect light reaches further: fewer pixels keep their bits
    assert _pixels_equal(before[1].state, after[1].state).sum() < same.sum()


def test_rendered_light_edit_changes_most_pixels(fray, abi, gpu):
    before, after = _states_around_edit(fray, "cornell-light")
    chg = fray.change_frame(before[0], after[0])
    chg0 = fray.change_frame(before[0], after[0], radius=0)
    print("cornell-light: change > 0 on %d of %d pixels (radius 0: %d)" % (int((chg > 0).sum()), chg.size, int((chg0 > 0).sum())))
    assert 2 * int((chg > 0).sum()) > chg.size


# ---- 4. render_sequence ------------------------------------------------------------------------------------------------------------------------
FRAMES, MOVE_AT = 4, 2
PLAIN_KEYS = ("features_frame", "motion", "history", "signal", "variance")
SPLIT_KEYS = ("features_frame", "motion", "history", "signal_direct", "signal_indirect", "variance_direct", "variance_indirect", "direct", "indirect")


def _sequence(fray, abi, split, **kw):
    """The four frames of the static-camera cornell sequence whose tall block moves before frame 2: [(out, raw, info as numpy)]."""
    s = open_scene(fray, "cornell_box.fray", W3, H3, numPaths=8)
    s.beginRender()
    start = abi.Camera.from_buffer_copy(s.camera)
    calls = []

    def edit(k, scene):
        calls.append(k)
        if k == MOVE_AT:
            scene_edits.apply(fray, scene, scene_edits.CASES["cornell-block"]["edit"])
            scene.update()
    frames = []
    for out, raw, info in s.render_sequence([start] * FRAMES, seed=SEED, edit=edit, split=split, **kw):
        keep = {k: (_np(v) if hasattr(v, "cpu") else v) for k, v in info.items()}
        frames.append((_np(out), _np(raw), keep))
    assert calls == [1, 2, 3] and len(frames) == FRAMES
    s.close()
    return frames


def _eroded(mask):
    """The pixels whose 3 x 3 neighbourhood (inside the image) lies in `mask`."""
    out = mask.copy()
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            q, valid = _shift(mask, j, i)
            out &= q | ~valid
    return out


def _check_component(what, frames_c, frames_p, change_key, signal_key, history_of):
    """One signal of the sequence with change frames (frames_c) against the one without (frames_p): P1 at system level.

    What can hold, and is asserted.  The accumulated signal and the history of pixel p in frame k are a function of p's own change and of the
    previous history at p's four bilinear taps; with a static camera the taps lie in p's 3 x 3 neighbourhood (the feature frame's position is a
    mean of points that project into p, so it projects into p, and x0 = floor(fx - 0.5) is p.x - 1 or p.x).  So: in a frame whose change
    frame is zero everywhere and whose previous history is equal everywhere, every bit is equal (frame 1); a pixel whose change is 0 in frame 2
    has the plain run's signal and history there, because frame 1's history is equal everywhere; and in frame 3, whose change frame is zero
    everywhere, so has every pixel whose 3 x 3 neighbourhood had change 0 in frame 2.  A pixel whose own change is 0 in frames 1..3 but whose
    NEIGHBOUR's was not in frame 2 fetches that neighbour's shortened history in frame 3 and differs; the count is printed (MI355X: 45 of the
    241 such pixels of the unsplit run, 49 of 2511 for direct light, 45 of 241 for indirect light; none of those with a clean neighbourhood).
    The filtered picture is five a-trous levels, whose footprint covers this 64 x 48 frame: it is compared in the frames where every input
    is equal (0 and 1).  So "a pixel whose change is 0 in frames 1..3 has out, signal and history bit-equal" holds in this form and no wider
    one, for any implementation of these launches."""
    c1, c2, c3 = (frames_c[k][2][change_key] for k in (1, 2, 3))
    assert frames_c[0][2][change_key] is None                                    # frame 0 has no probe
    assert not c1.any() and not c3.any()                                         # the edit changed nothing before frames 1 and 3
    assert c2.any() and (c2 == 0).any()
    for k in (0, 1):
        _same("%s frame %d signal" % (what, k), frames_c[k][2][signal_key], frames_p[k][2][signal_key])
        _same("%s frame %d history" % (what, k), history_of(frames_c[k][2]), history_of(frames_p[k][2]))
    still2 = c2 == 0
    sig2 = _pixels_equal(frames_c[2][2][signal_key], frames_p[2][2][signal_key])
    his2 = _pixels_equal(history_of(frames_c[2][2]), history_of(frames_p[2][2]))
    assert sig2[still2].all() and his2[still2].all(), (what, int((~sig2[still2]).sum()), int((~his2[still2]).sum()))
    safe3 = _eroded(still2)
    sig3 = _pixels_equal(frames_c[3][2][signal_key], frames_p[3][2][signal_key])
    his3 = _pixels_equal(history_of(frames_c[3][2]), history_of(frames_p[3][2]))
    print("%s: change 0 in frames 1..3 at %d pixels (3 x 3 neighbourhoods too: %d); frame 3 differs from the plain run at %d / %d of them"
          % (what, int(still2.sum()), int(safe3.sum()), int((still2 & ~(sig3 & his3)).sum()), int((safe3 & ~(sig3 & his3)).sum())))
    assert safe3.any() and sig3[safe3].all() and his3[safe3].all(), what
    # where the change frame is not zero the history is shorter: never longer than the plain run's, and shorter wherever that one had any
    # (a change below 2^-20 may round away in alpha = a0 + g (1 - a0), a0 >= alpha_min = 0.05: it is held to <= only)
    Nc, Np = history_of(frames_c[2][2])[..., 3], history_of(frames_p[2][2])[..., 3]
    hit = c2 > 0
    clear = (c2 >= F(2.0 ** -20)) & (Np > 1)
    assert (Nc[hit] <= Np[hit]).all() and (Nc[clear] < Np[clear]).all() and clear.any(), what
    return hit


def test_render_sequence_with_change_samples(fray, abi, gpu):
    plain = _sequence(fray, abi, False)
    adapt = _sequence(fray, abi, False, change_samples=NPROBE)
    own = _sequence(fray, abi, False, change_samples=NPROBE, change=dict(radius=0))          # change > 0 exactly where the pixel's own states differ
    # change_samples=0 is the default, and exactly today's launches
    off = _sequence(fray, abi, False, change_samples=0)
    for k in range(FRAMES):
        assert "change" not in off[k][2] and "probe" not in off[k][2] and "change" not in plain[k][2]
        _same("frame %d picture, change_samples=0 against the default" % k, off[k][0], plain[k][0])
        _same("frame %d raw" % k, adapt[k][1], plain[k][1])                     # the resumable contract: raw is render(seed + k)
        _same("frame %d raw, radius 0" % k, own[k][1], plain[k][1])
        for key in ("features_frame", "motion"):
            _same("frame %d %s" % (k, key), adapt[k][2][key], plain[k][2][key])
        assert (adapt[k][2]["probe"] is None) == (k == 0)
        if k:
            assert adapt[k][2]["probe"]["ms_kernels"] > 0 and adapt[k][2]["render"]["ms_kernels"] > 0
    for k in (0, 1):                                                                # nothing has changed yet: every output bit
        _same("frame %d picture" % k, adapt[k][0], plain[k][0])
        _same("frame %d variance" % k, adapt[k][2]["variance"], plain[k][2]["variance"])
    _check_component("sequence", adapt, plain, "change", "signal", lambda info: info["history"])
    # some pixels differ in the probe at frame 2 (radius 0: the pixel's own states), and their N after frame 2 is below the plain run's
    differ = own[2][2]["change"] > 0
    Nc, Np = adapt[2][2]["history"][..., 3], plain[2][2]["history"][..., 3]
    had = differ & (Np > 1) & (adapt[2][2]["change"] >= F(2.0 ** -20))            # (a smaller change may round away in alpha, see above)
    print("frame 2: %d pixels differ in the probe, %d of them had a history; N there %.3f on average against %.3f"
          % (int(differ.sum()), int(had.sum()), float(Nc[had].mean()), float(Np[had].mean())))
    assert had.sum() > 20 and (Nc[had] < Np[had]).all() and (Nc[differ] <= Np[differ]).all()
    assert (adapt[2][2]["change"][differ] > 0).all()                               # the window holds the pixel itself
    # and the moved block's own pixels are the motion frame's business: masked out of the difference
    moved = plain[2][2]["motion"][..., 3] != 0
    assert moved.any() and not (differ & moved).any()


def test_render_sequence_split_with_change_samples(fray, abi, gpu):
    plain = _sequence(fray, abi, True)
    adapt = _sequence(fray, abi, True, change_samples=NPROBE)
    for k in range(FRAMES):
        _same("frame %d raw" % k, adapt[k][1], plain[k][1])
        for key in ("features_frame", "motion", "direct_rgb", "indirect_rgb"):
            _same("frame %d %s" % (k, key), adapt[k][2][key], plain[k][2][key])
        assert "change" not in adapt[k][2] and "change_direct" not in plain[k][2]
        assert tuple(adapt[k][2]["history"].shape) == (H3, W3, 20)
    for k in (0, 1):                                      # the unfused frame 1 is the fused one in every bit
        _same("frame %d picture" % k, adapt[k][0], plain[k][0])
        for key in SPLIT_KEYS:
            _same("frame %d %s" % (k, key), adapt[k][2][key], plain[k][2][key])
    hit_d = _check_component("direct", adapt, plain, "change_direct", "signal_direct", lambda info: fray.split_history_parts(info["history"])[0])
    hit_i = _check_component("indirect", adapt, plain, "change_indirect", "signal_indirect", lambda info: fray.split_history_parts(info["history"])[1])
    print("frame 2: change > 0 at %d pixels of the direct component and %d of the indirect one" % (int(hit_d.sum()), int(hit_i.sum())))
    assert hit_i.sum() > hit_d.sum()                      # indirect light reaches further


def test_render_sequence_change_refusals(fray, abi, gpu):
    s = open_scene(fray, "cornell_box.fray", W3, H3, numPaths=2)
    s.beginRender()
    cam = abi.Camera.from_buffer_copy(s.camera)
    rendered = []
    edit = lambda k, scene: rendered.append(k)
    for kw, exc, words in ((dict(change_samples=2), ValueError, "needs edit"),
                           (dict(change_samples=-1, edit=edit), ValueError, "change_samples"),
                           (dict(change=dict(radius=1), edit=edit), ValueError, "change_samples > 0"),
                           (dict(change_samples=2, change=dict(window=1), edit=edit), TypeError, "radius and gain"),
                           (dict(change_samples=2, change=dict(radius=4), edit=edit), ValueError, "radius"),
                           (dict(change_samples=2, change=dict(gain=0.0), edit=edit), ValueError, "gain")):
        with pytest.raises(exc, match=words):
            next(s.render_sequence([cam, cam], **kw))
    assert not rendered and bytes(s.camera) == bytes(cam)
    # n = min(change_samples, spp): a probe of the whole frame, and no samples left to add
    frames = list(s.render_sequence([cam, cam], edit=edit, change_samples=50))
    assert rendered == [1] and frames[0][2]["change"] is None and not frames[1][2]["change"].any()
    raw, _ = s.render(seed=43)
    _same("raw of a frame that is all probe", frames[1][1], raw)
    s.close()
