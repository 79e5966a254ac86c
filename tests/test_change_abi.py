"""Change frames and gradient-adaptive accumulation without a GPU (include/frayhip.h "change frames"): the six entries and their mirrors, struct
frayhip_change's layout and defaults, every FRAYHIP_E_ARG case of frayhip_change_frame and frayhip_temporal_accumulate_adaptive (host and
_device; none touches a device), the Python-side refusals, the CLI flag, and the restatement (tests/change_ref.py) on synthetic inputs: a
change frame of zeros is the plain restatement, one of ones is the first-frame call."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import change_ref
import motion_ref
import temporal_ref
import temporal_split_ref as split_ref
from conftest import ROOT
from test_abi import header_functions

ENTRIES = ["frayhip_change_defaults", "frayhip_change_frame", "frayhip_change_frame_device", "frayhip_temporal_accumulate_adaptive",
           "frayhip_temporal_accumulate_adaptive_device"]
F = np.float32


def test_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    for n in ("change_frame", "change_params"):
        assert callable(getattr(fray, n)) and n in fray.__all__, n
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additions only
    # the header's prototypes and abi.py's agree in the number of arguments (pointers and ints are told apart by test_abi's own check)
    src = " ".join(open(os.path.join(ROOT, "include", "frayhip.h")).read().split())
    for n in ENTRIES:
        proto = src[src.index("int " + n + "("):]
        args = proto[proto.index("(") + 1:proto.index(");")].split(",")
        assert len(args) == len(abi.SYMBOLS[n][1]), (n, args)
    for words in ("struct frayhip_change {", "int32_t radius;", "float gain;"):
        assert words in src, words


def test_struct_and_defaults(fray, abi):
    assert fray.lib.frayhip_sizeof(b"frayhip_change") == C.sizeof(abi.Change) == 8
    assert (abi.Change.radius.offset, abi.Change.gain.offset) == (0, 4)
    assert fray.lib.frayhip_sizeof(b"frayhip_temporal") == C.sizeof(abi.Temporal) == 28         # as it was
    p = abi.Change(radius=-5, gain=9.0)
    assert fray.lib.frayhip_change_defaults(C.byref(p)) == abi.OK
    assert (p.radius, p.gain) == (change_ref.CHANGE_DEFAULTS["radius"], change_ref.CHANGE_DEFAULTS["gain"]) == (3, 1.0)
    assert fray.lib.frayhip_change_defaults(None) == abi.E_ARG
    assert "frayhip_change_defaults:" in fray.lib.frayhip_last_error().decode()
    q = fray.change_params(radius=1, gain=2.5)
    assert (q.radius, q.gain) == (1, 2.5)
    assert abi.ACCUM_CHANNELS == change_ref.ACCUM_CHANNELS == 4


def _arena(channels, W, H):
    """One arena, 2 KiB apart and 16-byte aligned: an output moved into another buffer and longer than it ends in the gap behind."""
    arena = np.zeros(512 * len(channels) + 4, F)
    base = (-arena.ctypes.data % 16) // 4
    bufs = {k: arena[base + 512 * n: base + 512 * n + H * W * c] for n, (k, c) in enumerate(channels.items())}
    ptr = {k: v.ctypes.data for k, v in bufs.items()}
    assert all(q % 16 == 0 for q in ptr.values())
    return arena, ptr, {k: v.nbytes for k, v in bufs.items()}


@pytest.mark.parametrize("dev", [False, True])
def test_change_frame_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    _keep, ptr, size = _arena(dict(b=4, a=4, mo=8, c=1), W, H)
    who = "frayhip_change_frame_device" if dev else "frayhip_change_frame"

    def call(w=W, h=H, prm="default", **over):
        p = abi.Change()
        L.frayhip_change_defaults(C.byref(p))
        for k in ("radius", "gain"):
            if k in over:
                setattr(p, k, over.pop(k))
        args = dict(ptr, p=C.byref(p) if prm == "default" else None)
        args.update(over)
        a = [args[k] for k in ("b", "a", "mo", "p", "c")]
        if dev:
            return L.frayhip_change_frame_device(w, h, *a, None, None)
        return L.frayhip_change_frame(w, h, *a, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, (rc, words)
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    expect(call(w=0), "width and height")
    expect(call(h=-1), "width and height")
    expect(call(w=1 << 16, h=1 << 15), "2^30")
    expect(call(b=None), "null accum_before")
    expect(call(a=None), "null accum_after")
    expect(call(prm=None), "null parameters")
    expect(call(c=None), "null change")
    for r in (-1, 4, 1 << 20):
        expect(call(radius=r), "radius")
    for g in (0.0, -0.0, -1.0, math.nan, math.inf, -math.inf):
        expect(call(gain=g), "gain")
    for i in ("b", "a", "mo"):
        expect(call(c=ptr[i]), "change must not overlap an input")
        expect(call(c=ptr[i] + size[i] - 16), "change must not overlap an input")
    if dev:
        expect(call(b=ptr["b"] + 4), "state not 16-byte")
        expect(call(a=ptr["a"] + 8), "state not 16-byte")
        expect(call(mo=ptr["mo"] + 4), "motion frame not 16-byte")
        expect(call(c=ptr["c"] + 2), "4-byte aligned")
    # a NULL motion is no error: with it the next wrong argument is the one that is named
    expect(call(mo=None, c=ptr["a"]), "change must not overlap an input")
    expect(call(mo=None, radius=7), "radius")


@pytest.mark.parametrize("dev", [False, True])
def test_adaptive_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    channels = dict(r=3, f=10, mo=8, ch=1, hi=12, ho=12, sg=3, va=1)
    _keep, ptr, size = _arena(channels, W, H)
    who = "frayhip_temporal_accumulate_adaptive_device" if dev else "frayhip_temporal_accumulate_adaptive"
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    view = fray.view_from_camera(s.camera, W, H)
    s.close()
    ORDER = ("r", "f", "mo", "ch", "v", "hi", "p", "ho", "sg", "va")

    def call(w=W, h=H, vw=None, prm=None, **over):
        p = abi.Temporal()
        L.frayhip_temporal_defaults(C.byref(p))
        for k, val in (prm or {}).items():
            setattr(p, k, val)
        vv = abi.View.from_buffer_copy(view)
        for k, val in (vw or {}).items():
            if k == "pos0":
                vv.pos[0] = val
            else:
                setattr(vv, k, val)
        args = dict(ptr, v=C.byref(vv), p=C.byref(p))
        args.update(over)
        a = [args[k] for k in ORDER]
        if dev:
            return L.frayhip_temporal_accumulate_adaptive_device(w, h, *a, None, None)
        return L.frayhip_temporal_accumulate_adaptive(w, h, *a, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, (rc, words)
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    # the plain entry's list
    expect(call(w=0), "width and height")
    expect(call(h=-1), "width and height")
    expect(call(w=1 << 16, h=1 << 15), "2^30")
    for k, words in (("r", "null rgb"), ("f", "null feat"), ("p", "null parameters"), ("ho", "null hist_out"), ("sg", "null signal"),
                     ("va", "null variance")):
        expect(call(**{k: None}), words)
    expect(call(v=None), "both")
    expect(call(hi=None), "both")
    expect(call(vw=dict(width=W + 1)), "size")
    expect(call(vw=dict(height=H - 1)), "size")
    expect(call(vw=dict(pos0=math.nan)), "non-finite")
    expect(call(vw=dict(tan_x=math.inf)), "non-finite")
    expect(call(vw=dict(tan_y=0.0)), "tan_x and tan_y")
    cases = [("demodulate", 2)] + [(k, n) for n in (0, 4097) for k in ("max_history", "variance_history")]
    cases += [("alpha_min", x) for x in (-0.1, 1.5, math.nan)] + [("film_offset", x) for x in (math.nan, math.inf)]
    cases += [("plane_tolerance", x) for x in (-1.0, math.nan, math.inf)] + [("normal_min_dot", x) for x in (-1.5, 1.5, math.nan)]
    for k, x in cases:
        expect(call(prm={k: x}), k)
    outs = (("ho", "hist_out"), ("sg", "signal"), ("va", "variance"))
    for n, (o, name) in enumerate(outs):
        for i in ("r", "f", "mo", "ch", "hi"):                 # the change frame is an input like the others
            expect(call(**{o: ptr[i]}), name + " must not overlap an input")
            expect(call(**{o: ptr[i] + size[i] - 16}), name + " must not overlap an input")
        for o2, name2 in outs[:n]:
            expect(call(**{o: ptr[o2] + 16}), "%s must not overlap %s" % (name, name2))
    # and the change frame's own
    expect(call(ch=None), "null change")
    expect(call(ch=None, mo=None), "null change")
    if dev:
        for k in ("r", "f", "sg", "va", "ch"):
            expect(call(**{k: ptr[k] + 2}), "4-byte aligned")
        expect(call(hi=ptr["hi"] + 4), "history not 16-byte")
        expect(call(ho=ptr["ho"] + 8), "history not 16-byte")
        expect(call(mo=ptr["mo"] + 4), "motion frame not 16-byte")
    # a NULL motion is no error (the plain arithmetic): with it the next wrong argument is the one that is named
    expect(call(mo=None, sg=ptr["ch"]), "signal must not overlap an input")
    expect(call(mo=None, v=None, hi=None, va=ptr["f"]), "variance must not overlap an input")


def test_python_side_refuses_bad_inputs(fray, abi):
    st = np.zeros((4, 5, 4), F)
    rgb = np.zeros((4, 5, 3), F)
    feat = np.zeros((4, 5, 10), F)
    chg = np.zeros((4, 5), F)
    with pytest.raises(ValueError):
        fray.change_frame(st, st[:, :4])
    with pytest.raises(ValueError):
        fray.change_frame(st, rgb)                              # a frame is not a state
    with pytest.raises(TypeError):
        fray.change_frame(st.astype(np.float64), st)
    with pytest.raises(ValueError):
        fray.change_frame(st, st, motion=np.zeros((4, 5, 7), F))
    with pytest.raises(ValueError, match="samples"):
        fray.change_frame(fray.Accumulation(st, 2), fray.Accumulation(st.copy(), 3))
    with pytest.raises(fray.FrayError, match="radius"):
        fray.change_frame(st, st.copy(), radius=4)
    with pytest.raises(fray.FrayError, match="gain"):
        fray.change_frame(st, st.copy(), gain=0.0)
    with pytest.raises(ValueError):
        fray.temporal_accumulate(rgb, feat, change=np.zeros((4, 5, 1), F))
    with pytest.raises(ValueError):
        fray.temporal_accumulate(rgb, feat, change=chg[:, :4])
    with pytest.raises(TypeError):
        fray.temporal_accumulate(rgb, feat, change=chg.astype(np.float64))
    if "torch" in sys.modules:
        import torch
        with pytest.raises(TypeError, match="mix"):
            fray.change_frame(torch.zeros(4, 5, 4), st)
        with pytest.raises(TypeError, match="mix"):
            fray.temporal_accumulate(rgb, feat, change=torch.zeros(4, 5))
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    with pytest.raises(fray.FrayError, match="beginRender"):
        next(s.render_sequence([s.camera], edit=lambda k, scene: None, change_samples=2))
    s.close()


def test_cli_lists_change_samples(capsys):
    env = dict(os.environ, FRAYHIP_NO_TORCH="1")
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr
    assert "--change-samples K" in out.stdout and "Scene.render_sequence(change_samples=K)" in " ".join(out.stdout.split())
    from fray_amd.__main__ import build_parser, check_args
    ap = build_parser()
    seq = ["--denoise", "--frames", "3", "--move", "6", "1", "0", "0", "--motion-vectors"]
    for argv in (seq + ["--change-samples", "2"], seq + ["--split", "--change-samples", "2"], seq):
        a = ap.parse_args(["scene.fray"] + argv)
        check_args(ap, a)
        assert a.change_samples == (2 if "--change-samples" in argv else 0)
    for argv, words in ((["--denoise", "--frames", "3", "--change-samples", "2"], "--change-samples needs"),
                        (["--denoise", "--frames", "3", "--move", "6", "1", "0", "0", "--change-samples", "2"], "--change-samples needs"),
                        (seq + ["--change-samples", "-1"], "--change-samples must be >= 0")):
        with pytest.raises(SystemExit) as e:
            check_args(ap, ap.parse_args(["scene.fray"] + argv))
        assert e.value.code == 2 and words in capsys.readouterr().err, argv


# ---- the restatement on synthetic inputs ----------------------------------------------------------------------------------------------------
def test_change_restatement_properties():
    rng = np.random.default_rng(3)
    H, W = 19, 37
    before = rng.uniform(0.0, 4.0, (H, W, 4)).astype(F)
    after = before.copy()
    after[5:9, 10:14, 0:3] = rng.uniform(0.0, 4.0, (4, 4, 3)).astype(F)
    for radius in range(4):
        c = change_ref.change_frame(before, after, radius=radius)
        assert c.dtype == F and c.shape == (H, W) and (c >= 0).all() and (c <= 1).all()
        reach = np.zeros((H, W), bool)
        reach[max(0, 5 - radius):9 + radius, max(0, 10 - radius):14 + radius] = True
        assert (c[~reach] == 0).all() and (c[reach] > 0).all(), radius                  # exactly the window's reach
    assert (change_ref.change_frame(before, before.copy()) == 0).all()
    assert (change_ref.change_frame(before, after, gain=1e6)[5:9, 10:14] == 1).all()       # the clamp
    moved = np.zeros((H, W, 8), F)
    moved[5:9, 10:14, 3] = 0.25                                                          # a share of the samples is enough
    assert (change_ref.change_frame(before, after, motion=moved) == 0).all()
    bad = after.copy()
    bad[5:9, 10:14, 1] = (np.nan, np.inf, -np.inf, np.nan)
    assert (change_ref.change_frame(before, bad) == 0).all()                             # a texel that is not finite counts for nothing
    assert (change_ref.change_frame(np.zeros_like(before), np.zeros_like(before)) == 0).all()          # sm = 0


@pytest.mark.parametrize("with_motion", [False, True])
def test_adaptive_restatement_zero_and_one(with_motion):
    I = split_ref.CHAIN_INDIRECT
    hist = view = None
    for k, (_d, rgb, feat, v, motion) in enumerate(split_ref.chain_frames(with_motion)):
        if with_motion:
            plain = motion_ref.accumulate(rgb, feat, motion, view, hist, demodulate=0, **I)
        else:
            plain = temporal_ref.accumulate(rgb, feat, view, hist, demodulate=0, **I)
        zero = change_ref.accumulate(rgb, feat, np.zeros(rgb.shape[:2], F), motion, view, hist, demodulate=0, **I)
        neg = change_ref.accumulate(rgb, feat, np.full(rgb.shape[:2], -0.0, F), motion, view, hist, demodulate=0, **I)
        one = change_ref.accumulate(rgb, feat, np.ones(rgb.shape[:2], F), motion, view, hist, demodulate=0, **I)
        first = change_ref.accumulate(rgb, feat, np.zeros(rgb.shape[:2], F), motion, None, None, demodulate=0, **I)
        for a, b, c, d in zip(plain, zero, neg, one):
            assert a.tobytes() == b.tobytes() == c.tobytes(), k
        for a, b in zip(one, first):
            assert a.tobytes() == b.tobytes(), k
        hist, view = plain[0], v
