"""Split temporal accumulation without a GPU (include/frayhip.h "split temporal accumulation"): the two entries and their mirrors, every
FRAYHIP_E_ARG case of both (none touches a device), the history helpers, the Python-side refusals, the CLI, and the restatement's packing
(tests/temporal_split_ref.py) on the synthetic chain."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import motion_ref
import temporal_ref
import temporal_split_ref as split_ref
from conftest import ROOT
from test_abi import header_functions

ENTRIES = ["frayhip_temporal_accumulate_split", "frayhip_temporal_accumulate_split_device"]
F = np.float32


def test_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    for n in ("temporal_accumulate_split", "split_history_parts", "join_history_parts"):
        assert callable(getattr(fray, n)) and n in fray.__all__, n
    assert abi.HISTORY_SPLIT_CHANNELS == split_ref.HISTORY_SPLIT_CHANNELS == 20
    assert "#define FRAYHIP_HISTORY_SPLIT_CHANNELS 20" in open(os.path.join(ROOT, "include", "frayhip.h")).read()
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additions only
    assert fray.lib.frayhip_sizeof(b"frayhip_temporal") == C.sizeof(abi.Temporal) == 28         # no new struct, and this one as it was


@pytest.mark.parametrize("dev", [False, True])
def test_split_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    # one arena, 2 KiB apart: an output moved into another buffer and longer than it ends in the gap behind, not in a third buffer
    channels = dict(rd=3, ri=3, f=10, mo=8, hi=20, ho=20, sd=3, si=3, vd=1, vi=1)
    arena = np.zeros(512 * len(channels) + 4, F)
    base = (-arena.ctypes.data % 16) // 4
    bufs = {k: arena[base + 512 * n: base + 512 * n + H * W * c] for n, (k, c) in enumerate(channels.items())}
    ptr = {k: v.ctypes.data for k, v in bufs.items()}
    size = {k: v.nbytes for k, v in bufs.items()}
    assert all(q % 16 == 0 for q in ptr.values())
    who = ENTRIES[1] if dev else ENTRIES[0]
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    view = fray.view_from_camera(s.camera, W, H)
    s.close()
    ORDER = ("rd", "ri", "f", "mo", "v", "hi", "pd", "pi", "ho", "sd", "si", "vd", "vi")

    def call(w=W, h=H, vw=None, direct=None, indirect=None, **over):
        prm = {}
        for name, fields in (("pd", direct), ("pi", indirect)):
            prm[name] = abi.Temporal()
            L.frayhip_temporal_defaults(C.byref(prm[name]))
            for k, val in (fields or {}).items():
                setattr(prm[name], k, val)
        vv = abi.View.from_buffer_copy(view)
        for k, val in (vw or {}).items():
            if k == "pos0":
                vv.pos[0] = val
            else:
                setattr(vv, k, val)
        args = dict(ptr, v=C.byref(vv), pd=C.byref(prm["pd"]), pi=C.byref(prm["pi"]))
        args.update(over)
        a = [args[k] for k in ORDER]
        if dev:
            return L.frayhip_temporal_accumulate_split_device(w, h, *a, None, None)
        return L.frayhip_temporal_accumulate_split(w, h, *a, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, (rc, words)
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    expect(call(w=0), "width and height")
    expect(call(h=-1), "width and height")
    expect(call(w=1 << 16, h=1 << 15), "2^30")
    for k, words in (("rd", "null rgb_direct"), ("ri", "null rgb_indirect"), ("f", "null feat"), ("pd", "null p_direct"), ("pi", "null p_indirect"),
                     ("ho", "null hist_out"), ("sd", "null signal_direct"), ("si", "null signal_indirect"), ("vd", "null variance_direct"),
                     ("vi", "null variance_indirect")):
        expect(call(**{k: None}), words)
    expect(call(v=None), "both")
    expect(call(hi=None), "both")
    expect(call(vw=dict(width=W + 1)), "size")
    expect(call(vw=dict(height=H - 1)), "size")
    expect(call(vw=dict(pos0=math.nan)), "non-finite")
    expect(call(vw=dict(tan_x=math.inf)), "non-finite")
    expect(call(vw=dict(tan_y=0.0)), "tan_x and tan_y")
    # the fields that decide which taps count must agree, bit for bit
    for k, a, b in (("demodulate", 1, 0), ("film_offset", 0.5, 0.0), ("plane_tolerance", 0.02, 0.03), ("normal_min_dot", 0.9, 0.5),
                    ("film_offset", 0.0, -0.0)):
        expect(call(direct={k: a}, indirect={k: b}), "differ in " + k)
        expect(call(direct={k: b}, indirect={k: a}), "differ in " + k)
    # each range, in either struct (the other one's shared fields follow, so that only the range is wrong)
    cases = [("demodulate", 2)] + [(k, n) for n in (0, 4097) for k in ("max_history", "variance_history")]
    cases += [("alpha_min", x) for x in (-0.1, 1.5, math.nan)] + [("film_offset", x) for x in (math.nan, math.inf)]
    cases += [("plane_tolerance", x) for x in (-1.0, math.nan, math.inf)] + [("normal_min_dot", x) for x in (-1.5, 1.5, math.nan)]
    for k, x in cases:
        both = {k: x} if k in split_ref.SHARED else {}
        expect(call(direct={k: x}, indirect=both), "p_direct: " + k)
        expect(call(direct={}, indirect={k: x}), "p_indirect: " + k)
    # each output over each input, wholly and in part, and over each other output
    outs = (("ho", "hist_out"), ("sd", "signal_direct"), ("si", "signal_indirect"), ("vd", "variance_direct"), ("vi", "variance_indirect"))
    for n, (o, name) in enumerate(outs):
        for i in ("rd", "ri", "f", "mo", "hi"):
            expect(call(**{o: ptr[i]}), name + " must not overlap an input")
            expect(call(**{o: ptr[i] + size[i] - 16}), name + " must not overlap an input")
        for o2, name2 in outs[:n]:
            expect(call(**{o: ptr[o2] + 16}), "%s must not overlap %s" % (name, name2))
    if dev:
        for k in ("rd", "ri", "f", "sd", "si", "vd", "vi"):
            expect(call(**{k: ptr[k] + 2}), "4-byte aligned")
        expect(call(hi=ptr["hi"] + 4), "history not 16-byte")
        expect(call(ho=ptr["ho"] + 8), "history not 16-byte")
        expect(call(mo=ptr["mo"] + 4), "motion frame not 16-byte")
    # a NULL motion is no error: with it the next wrong argument is the one that is named
    expect(call(mo=None, sd=ptr["rd"]), "signal_direct must not overlap an input")
    expect(call(mo=None, v=None, hi=None, vi=ptr["f"]), "variance_indirect must not overlap an input")


def test_history_parts_round_trip(fray, abi):
    rng = np.random.default_rng(4)
    hist = rng.standard_normal((5, 7, 20)).astype(F)
    hist[..., 18:20] = 0.0
    hist[0, 0, 4:11] = [-0.0, np.inf, np.nan, 3.0, 0.0, -0.0, 1e-42]          # bits, not values
    hd, hi = fray.split_history_parts(hist)
    assert hd.shape == hi.shape == (5, 7, 12) and hd.flags.c_contiguous and hi.flags.c_contiguous
    rd, ri = split_ref.split_parts(hist)
    assert hd.tobytes() == rd.tobytes() and hi.tobytes() == ri.tobytes()
    assert hd.tobytes() == hist[..., 0:12].tobytes()
    assert hi[..., 0:4].tobytes() == hist[..., 12:16].tobytes() and hi[..., 4:7].tobytes() == hist[..., 4:7].tobytes()
    assert hi[..., 7].tobytes() == hist[..., 16].tobytes() and hi[..., 11].tobytes() == hist[..., 17].tobytes()
    back = fray.join_history_parts(hd, hi)
    assert back.dtype == F and back.tobytes() == hist.tobytes() == split_ref.join_parts(hd, hi).tobytes()
    for col, words in ((5, "position"), (10, "normal")):
        other = hi.copy()
        other[2, 3, col] = np.nextafter(other[2, 3, col], F(9))
        with pytest.raises(ValueError, match=words):
            fray.join_history_parts(hd, other)
    other = hi.copy()
    other[0, 0, 9] = 0.0                                   # +0.0 against -0.0: equal values, other bits
    with pytest.raises(ValueError, match="normal"):
        fray.join_history_parts(hd, other)
    with pytest.raises(ValueError):
        fray.split_history_parts(hd)
    with pytest.raises(ValueError):
        fray.join_history_parts(hd, hi[:, :6])
    with pytest.raises(ValueError):
        fray.join_history_parts(hist, hi)


def test_python_side_refuses_bad_inputs(fray, abi):
    rgb = np.zeros((4, 5, 3), F)
    feat = np.zeros((4, 5, 10), F)
    hist = np.zeros((4, 5, 20), F)
    s = fray.Scene.parseScene(os.path.join(ROOT, "scenes", "cornell_box.fray"))
    view = fray.view_from_camera(s.camera, 5, 4)
    split = fray.temporal_accumulate_split
    for k, a, b in (("demodulate", 1, 0), ("film_offset", 0.5, 0.25), ("plane_tolerance", 0.02, 0.04), ("normal_min_dot", 0.9, 0.8)):
        with pytest.raises(ValueError, match=k):
            split(rgb, rgb, feat, direct={k: a}, indirect={k: b})
        with pytest.raises(ValueError, match=k):
            split(rgb, rgb, feat, indirect={k: b}, **{k: a})
    with pytest.raises(TypeError):
        split(rgb, rgb, feat, direct=dict(history=3))
    with pytest.raises(TypeError):
        split(rgb, rgb, feat, alpha=0.5)
    with pytest.raises(TypeError):
        split(rgb.astype(np.float64), rgb, feat)
    with pytest.raises(ValueError):
        split(rgb, rgb[:, :4], feat)
    with pytest.raises(ValueError):
        split(rgb, rgb, feat, view, hist[..., :12])            # an ordinary history is not a split one
    with pytest.raises(ValueError):
        split(rgb, rgb, feat, motion=np.zeros((4, 5, 7), F))
    with pytest.raises(ValueError, match="both"):
        split(rgb, rgb, feat, view, None)
    with pytest.raises(ValueError, match="both"):
        split(rgb, rgb, feat, None, hist)
    with pytest.raises(TypeError):
        split(rgb, rgb, feat, s.camera, hist)
    with pytest.raises(fray.FrayError, match="p_indirect: max_history"):
        split(rgb, rgb, feat, indirect=dict(max_history=0))
    with pytest.raises(fray.FrayError, match="size"):
        split(rgb, rgb, feat, fray.view_from_camera(s.camera, 6, 4), hist)
    if "torch" in sys.modules:
        import torch
        with pytest.raises(TypeError, match="mix"):
            split(torch.zeros(4, 5, 3), rgb, feat)
        with pytest.raises(TypeError, match="CPU tensor"):
            split(torch.zeros(4, 5, 3), torch.zeros(4, 5, 3), torch.zeros(4, 5, 10))
    with pytest.raises(fray.FrayError, match="beginRender"):
        next(s.render_sequence([s.camera], split=True))
    s.close()


def test_cli_lists_the_split_sequence(capsys):
    env = dict(os.environ, FRAYHIP_NO_TORCH="1")
    out = subprocess.run([sys.executable, "-m", "fray_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr
    assert "With --frames N: the sequence keeps one history per component" in " ".join(out.stdout.split())       # --split's help, re-wrapped
    from fray_amd.__main__ import build_parser, check_args
    ap = build_parser()
    for argv in (["--denoise", "--split", "--frames", "3"], ["--denoise", "--split", "--frames", "3", "--yaw-step", "0.5"],
                 ["--denoise", "--split", "--frames", "3", "--move", "2", "1", "0", "0"],
                 ["--denoise", "--split", "--frames", "3", "--move", "2", "1", "0", "0", "--motion-vectors"]):
        a = ap.parse_args(["scene.fray"] + argv)
        check_args(ap, a)
        assert a.split and a.frames == 3
    # the other refusals stay
    for argv, words in ((["--split", "--frames", "3"], "--frames needs --denoise"),
                        (["--split", "--frames", "3", "--move", "2", "1", "0", "0"], "--split needs --denoise"),
                        (["--denoise", "--split", "--frames", "3", "--adaptive", "0.05"], "--adaptive"),
                        (["--denoise", "--split", "--frames", "3", "--components-out", "c.npz"], "--components-out cannot be combined with --frames"),
                        (["--denoise", "--split", "--accumulate", "a.npz"], "--accumulate")):
        with pytest.raises(SystemExit) as e:
            check_args(ap, ap.parse_args(["scene.fray"] + argv))
        assert e.value.code == 2 and words in capsys.readouterr().err, argv


@pytest.mark.parametrize("with_motion", [False, True])
def test_restatement_is_two_calls_packed(with_motion):
    hist = hd = hi = view = None
    for k, (rgb_d, rgb_i, feat, v, motion) in enumerate(split_ref.chain_frames(with_motion)):
        hist, sd, si, vd, vi = split_ref.accumulate_split(rgb_d, rgb_i, feat, view, hist, motion=motion, direct=split_ref.CHAIN_DIRECT,
                                                          indirect=split_ref.CHAIN_INDIRECT, demodulate=0)
        if with_motion:
            hd, wsd, wvd = motion_ref.accumulate(rgb_d, feat, motion, view, hd, demodulate=0, **split_ref.CHAIN_DIRECT)
            hi, wsi, wvi = motion_ref.accumulate(rgb_i, feat, motion, view, hi, demodulate=0, **split_ref.CHAIN_INDIRECT)
        else:
            hd, wsd, wvd = temporal_ref.accumulate(rgb_d, feat, view, hd, demodulate=0, **split_ref.CHAIN_DIRECT)
            hi, wsi, wvi = temporal_ref.accumulate(rgb_i, feat, view, hi, demodulate=0, **split_ref.CHAIN_INDIRECT)
        view = v
        assert hist.shape == (split_ref.CHAIN_H, split_ref.CHAIN_W, 20) and hist.dtype == F
        assert hist[..., 0:12].tobytes() == hd.tobytes(), k                                     # rows 0-2: the direct history as it stands
        assert hist[..., 12:16].tobytes() == hi[..., 0:4].tobytes(), k                          # row 3: {accI, N_I}
        assert hist[..., 16].tobytes() == hi[..., 7].tobytes() and hist[..., 17].tobytes() == hi[..., 11].tobytes(), k      # row 4: m1_I, m2_I
        assert hist[..., 18:20].tobytes() == np.zeros((split_ref.CHAIN_H, split_ref.CHAIN_W, 2), F).tobytes(), k            # and +0.0f twice
        assert hi[..., 4:7].tobytes() == hd[..., 4:7].tobytes() and hi[..., 8:11].tobytes() == hd[..., 8:11].tobytes(), k
        for got, want in ((sd, wsd), (si, wsi), (vd, wvd), (vi, wvi)):
            assert got.tobytes() == want.tobytes(), k
