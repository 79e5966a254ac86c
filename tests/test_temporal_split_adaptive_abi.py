"""Adaptive split accumulation without a GPU (include/frayhip.h "change frames", frayhip_temporal_accumulate_split_adaptive): the two entries
and their mirrors, every FRAYHIP_E_ARG case of both (the split entry's list and the change frames' own; none touches a device), the
Python-side refusals, and the restatement (tests/temporal_split_adaptive_ref.py) on the synthetic chain: what the chain exercises, change
frames of +0 are the split restatement, change frames of 1 the first-frame call, and one change frame passed twice equals two copies."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import temporal_split_adaptive_ref as ref
import temporal_split_ref as split_ref
from conftest import ROOT
from test_abi import header_functions

ENTRIES = ["frayhip_temporal_accumulate_split_adaptive", "frayhip_temporal_accumulate_split_adaptive_device"]
F = np.float32


def test_entries_exported_and_mirrored(fray, abi):
    names = header_functions()
    for n in ENTRIES:
        assert n in names and n in abi.SYMBOLS and hasattr(fray.lib, n), n
    assert fray.lib.frayhip_abi_version() == abi.ABI_VERSION == 3          # additions only
    assert fray.lib.frayhip_sizeof(b"frayhip_temporal") == C.sizeof(abi.Temporal) == 28         # no new struct, and this one as it was
    # the header's prototypes and abi.py's agree in the number of arguments: the split entry's and two change frames
    src = " ".join(open(os.path.join(ROOT, "include", "frayhip.h")).read().split())
    for n in ENTRIES:
        proto = src[src.index("int " + n + "("):]
        args = proto[proto.index("(") + 1:proto.index(");")].split(",")
        assert len(args) == len(abi.SYMBOLS[n][1]) == len(abi.SYMBOLS[n.replace("_adaptive", "")][1]) + 2, (n, args)
    assert "a fused adaptive form" not in src                              # what "Not covered" used to list
    import inspect
    sig = inspect.signature(fray.temporal_accumulate_split).parameters
    assert sig["change_direct"].default is None and sig["change_indirect"].default is None


@pytest.mark.parametrize("dev", [False, True])
def test_split_adaptive_argument_checks(fray, abi, dev):
    L = fray.lib
    W, H = 4, 3
    # one arena, 2 KiB apart: an output moved into another buffer and longer than it ends in the gap behind, not in a third buffer
    channels = dict(rd=3, ri=3, f=10, mo=8, cd=1, ci=1, hi=20, ho=20, sd=3, si=3, vd=1, vi=1)
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
    ORDER = ("rd", "ri", "f", "mo", "cd", "ci", "v", "hi", "pd", "pi", "ho", "sd", "si", "vd", "vi")

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
            return L.frayhip_temporal_accumulate_split_adaptive_device(w, h, *a, None, None)
        return L.frayhip_temporal_accumulate_split_adaptive(w, h, *a, None)

    def expect(rc, words):
        assert rc == abi.E_ARG, (rc, words)
        msg = L.frayhip_last_error().decode()
        assert words in msg and who + ":" in msg, msg

    # ---- the split entry's list, as tests/test_temporal_split_abi.py walks it
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
    for k, a, b in (("demodulate", 1, 0), ("film_offset", 0.5, 0.0), ("plane_tolerance", 0.02, 0.03), ("normal_min_dot", 0.9, 0.5),
                    ("film_offset", 0.0, -0.0)):
        expect(call(direct={k: a}, indirect={k: b}), "differ in " + k)
        expect(call(direct={k: b}, indirect={k: a}), "differ in " + k)
    cases = [("demodulate", 2)] + [(k, n) for n in (0, 4097) for k in ("max_history", "variance_history")]
    cases += [("alpha_min", x) for x in (-0.1, 1.5, math.nan)] + [("film_offset", x) for x in (math.nan, math.inf)]
    cases += [("plane_tolerance", x) for x in (-1.0, math.nan, math.inf)] + [("normal_min_dot", x) for x in (-1.5, 1.5, math.nan)]
    for k, x in cases:
        both = {k: x} if k in split_ref.SHARED else {}
        expect(call(direct={k: x}, indirect=both), "p_direct: " + k)
        expect(call(direct={}, indirect={k: x}), "p_indirect: " + k)
    # each output over each input -- the change frames are inputs like the others -- wholly and in part, and over each other output
    outs = (("ho", "hist_out"), ("sd", "signal_direct"), ("si", "signal_indirect"), ("vd", "variance_direct"), ("vi", "variance_indirect"))
    for n, (o, name) in enumerate(outs):
        for i in ("rd", "ri", "f", "mo", "cd", "ci", "hi"):
            expect(call(**{o: ptr[i]}), name + " must not overlap an input")
            expect(call(**{o: ptr[i] + size[i] - 16}), name + " must not overlap an input")
        for o2, name2 in outs[:n]:
            expect(call(**{o: ptr[o2] + 16}), "%s must not overlap %s" % (name, name2))
    if dev:
        for k in ("rd", "ri", "f", "sd", "si", "vd", "vi", "cd", "ci"):
            expect(call(**{k: ptr[k] + 2}), "4-byte aligned")
        expect(call(hi=ptr["hi"] + 4), "history not 16-byte")
        expect(call(ho=ptr["ho"] + 8), "history not 16-byte")
        expect(call(mo=ptr["mo"] + 4), "motion frame not 16-byte")
    # ---- the change frames' own: both are required, with or without a motion frame or a history
    expect(call(cd=None), "null change_direct")
    expect(call(ci=None), "null change_indirect")
    expect(call(cd=None, ci=None), "null change_direct")
    expect(call(ci=None, mo=None), "null change_indirect")
    expect(call(cd=None, v=None, hi=None), "null change_direct")
    # inputs may alias each other: with one change frame for both components the next wrong argument is the one that is named, and an output
    # over that one frame is still refused
    expect(call(ci=ptr["cd"], vd=None), "null variance_direct")
    expect(call(ci=ptr["cd"], vi=ptr["cd"]), "variance_indirect must not overlap an input")
    expect(call(cd=ptr["ci"], sd=ptr["ci"]), "signal_direct must not overlap an input")
    # a NULL motion is no error: with it the next wrong argument is the one that is named
    expect(call(mo=None, sd=ptr["ci"]), "signal_direct must not overlap an input")
    expect(call(mo=None, v=None, hi=None, vi=ptr["cd"]), "variance_indirect must not overlap an input")


def test_python_side_refuses_bad_inputs(fray, abi):
    rgb = np.zeros((4, 5, 3), F)
    feat = np.zeros((4, 5, 10), F)
    chg = np.zeros((4, 5), F)
    split = fray.temporal_accumulate_split
    with pytest.raises(ValueError, match="both"):
        split(rgb, rgb, feat, change_direct=chg)
    with pytest.raises(ValueError, match="both"):
        split(rgb, rgb, feat, change_indirect=chg)
    for bad in (np.zeros((4, 5, 1), F), chg[:, :4], np.zeros((5, 4), F), np.zeros(20, F)):              # temporal_accumulate(change=)'s shape checks
        with pytest.raises(ValueError):
            split(rgb, rgb, feat, change_direct=bad, change_indirect=chg)
        with pytest.raises(ValueError):
            split(rgb, rgb, feat, change_direct=chg, change_indirect=bad)
    with pytest.raises(TypeError, match="float32"):
        split(rgb, rgb, feat, change_direct=chg.astype(np.float64), change_indirect=chg)
    with pytest.raises(TypeError, match="float32"):
        split(rgb, rgb, feat, change_direct=chg, change_indirect=chg.astype(np.int32))
    if "torch" in sys.modules:
        import torch
        with pytest.raises(TypeError, match="mix"):
            split(rgb, rgb, feat, change_direct=torch.zeros(4, 5), change_indirect=torch.zeros(4, 5))
    # the refusals of the call without change frames stay, with them
    with pytest.raises(ValueError, match="demodulate"):
        split(rgb, rgb, feat, direct=dict(demodulate=1), indirect=dict(demodulate=0), change_direct=chg, change_indirect=chg)


# ---- the restatement on the synthetic chain -------------------------------------------------------------------------------------------------------
CHAINS = [(False, 0), (False, 1), (True, 0), (True, 1)]


def test_chain_parameters():
    assert ref.CHAIN_DIRECT == dict(max_history=6, variance_history=3, alpha_min=0.3) and ref.CHAIN_INDIRECT is split_ref.CHAIN_INDIRECT
    shape = (split_ref.CHAIN_H, split_ref.CHAIN_W)
    kinds = set()
    for k in range(5):
        d, i = ref.chain_change_maps(k, shape)
        for seed, m in ((100 + k, d), (200 + k, i)):
            rng = np.random.default_rng(seed)                               # tests/test_gpu_change.py's _change_map, written out
            want = ref.CHANGE_VALUES[rng.integers(0, len(ref.CHANGE_VALUES), shape)]
            want = np.where(rng.uniform(size=shape) < 0.5, F(0), want).astype(F)
            assert m.tobytes() == want.tobytes(), (k, seed)
            kinds |= set(np.unique(m.view(np.uint32)).tolist())
    assert len(ref.CHANGE_VALUES) == 11 and kinds == set(ref.CHANGE_VALUES.view(np.uint32).tolist())
    assert [ref.BRANCHES[b] for b in ref.branch(ref.CHANGE_VALUES)] == ["keep"] * 3 + ["part"] * 4 + ["cut"] * 4
    for n in (1, 15):                                                       # the smallest shapes' maps
        seen = set()
        for shift in range(11 if n < 11 else 1):
            d, i = ref.cyclic_change_maps((n, 1), shift)
            seen |= set(d.view(np.uint32).ravel().tolist())
            assert ref.branch(d)[0, 0] != ref.branch(i)[0, 0]               # four values ahead is always another case
        assert seen == set(ref.CHANGE_VALUES.view(np.uint32).tolist())


@pytest.mark.parametrize("with_motion,demodulate", CHAINS)
def test_chain_exercises_every_pair_of_branches(with_motion, demodulate):
    frames = ref.chain(with_motion, demodulate)
    assert len(frames) == 5 and not frames[0]["fetched"].any()              # frame 0 has no history to fetch
    pairs, count = ref.chain_coverage(frames)
    every = {(a, b) for a in range(3) for b in range(3)}
    for k in range(1, 5):
        assert pairs[k] == every, (k, sorted(every - pairs[k]))             # all nine (direct, indirect) pairs among pixels with a history
    for name, (young, old) in count.items():
        assert young > 0 and old > 0, (name, young, old)                    # shortened histories on both sides of variance_history
    for fr in frames:
        assert not np.isnan(fr["ref"][0]).any()                             # and no history value is a NaN, whatever the maps hold


@pytest.mark.parametrize("with_motion,demodulate", CHAINS)
def test_restatement_zero_one_and_alias(with_motion, demodulate):
    D, I = ref.CHAIN_DIRECT, ref.CHAIN_INDIRECT
    for k, fr in enumerate(ref.chain(with_motion, demodulate)):
        shape = fr["rgb_d"].shape[:2]
        ins = (fr["rgb_d"], fr["rgb_i"], fr["feat"])
        kw = dict(motion=fr["motion"], direct=D, indirect=I, demodulate=demodulate)
        zero, neg, one = np.zeros(shape, F), np.full(shape, -0.0, F), np.ones(shape, F)
        z = ref.accumulate_split_adaptive(*ins, zero, zero.copy(), fr["prev_view"], fr["hist_in"], **kw)
        n = ref.accumulate_split_adaptive(*ins, neg, zero, fr["prev_view"], fr["hist_in"], **kw)
        o = ref.accumulate_split_adaptive(*ins, one, one.copy(), fr["prev_view"], fr["hist_in"], **kw)
        first = split_ref.accumulate_split(*ins, None, None, **kw)
        for name, a, b, c, d, e in zip(ref.NAMES, z, n, fr["plain"], o, first):
            assert a.tobytes() == b.tobytes() == c.tobytes(), (k, name)      # +0 (and -0): the split restatement
            assert d.tobytes() == e.tobytes(), (k, name)                     # 1: the hist_in = None call
        # one change frame for both components is two copies of it, and it moves both components
        both = ref.accumulate_split_adaptive(*ins, fr["chg_d"], fr["chg_d"], fr["prev_view"], fr["hist_in"], **kw)
        copies = ref.accumulate_split_adaptive(*ins, fr["chg_d"], fr["chg_d"].copy(), fr["prev_view"], fr["hist_in"], **kw)
        for name, a, b in zip(ref.NAMES, both, copies):
            assert a.tobytes() == b.tobytes(), (k, name)
        if k:
            assert both[2].tobytes() != fr["plain"][2].tobytes() and both[2].tobytes() != fr["ref"][2].tobytes(), k
        # the packing: each component's part is change_ref.accumulate's history for it
        hd, hi = split_ref.split_parts(fr["ref"][0])
        hin = split_ref.split_parts(fr["hist_in"]) if fr["hist_in"] is not None else (None, None)
        want_d = ref.change_ref.accumulate(fr["rgb_d"], fr["feat"], fr["chg_d"], fr["motion"], fr["prev_view"], hin[0], demodulate=demodulate, **D)
        want_i = ref.change_ref.accumulate(fr["rgb_i"], fr["feat"], fr["chg_i"], fr["motion"], fr["prev_view"], hin[1], demodulate=demodulate, **I)
        assert hd.tobytes() == want_d[0].tobytes() and hi.tobytes() == want_i[0].tobytes(), k
        assert fr["ref"][0][..., 18:20].tobytes() == np.zeros(shape + (2,), F).tobytes(), k
