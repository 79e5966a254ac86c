"""tests/call_history.py checked on its own (no GPU): the sequences cover every ordered pair, the operations' configurations are complete, and the
comparer names the call, the operation and its predecessor when a fake handle leaks one value from the call before."""
import os
import re

import numpy as np
import pytest

import call_history as ch
from conftest import ROOT

SIZES = [1, 2, 3, 7, 20, 41]


# ---- the sequences --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_euler_walks_every_ordered_pair_once(n):
    walk = ch.euler(n, 5)
    assert len(walk) == n * n + 1 and walk[0] == walk[-1] and set(walk) == set(range(n))
    pairs = list(zip(walk, walk[1:]))
    assert len(set(pairs)) == len(pairs) == n * n                       # each of the n * n ordered pairs, loops included, exactly once
    assert ch.euler(n, 5) == walk                                       # from its seed
    if n >= 7:
        assert ch.euler(n, 6) != walk


@pytest.mark.parametrize("n", SIZES[1:])
@pytest.mark.parametrize("k", [2, 3, 10, 64, 10 ** 6])
def test_arcs_lose_no_pair(n, k):
    walk = ch.euler(n, 9)
    cut = ch.arcs(walk, k)
    assert all(2 <= len(a) <= k for a in cut)
    assert all(b[0] == a[-1] for a, b in zip(cut, cut[1:]))             # an arc begins with the arc before's last operation
    assert ch.adjacent_pairs(cut) == {(a, b) for a in range(n) for b in range(n)}
    assert sum(len(a) - 1 for a in cut) == n * n                        # and no pair twice
    assert [cut[0][0]] + [v for a in cut for v in a[1:]] == walk


def test_big_then_small_places_every_operation_after_both():
    ops = [ch.Op("op%d" % i, None) for i in range(9)]
    for o, w in zip(ops, (5, 900, 17, 0, 900, 3, 0, 44, 12)):
        o.work = w
    walk = ch.big_then_small(ops)
    pairs = ch.adjacent_pairs([walk])
    assert all((1, i) in pairs and (3, i) in pairs for i in range(9))   # the first of the largest, the first of the smallest
    assert len(walk) == 4 * 9
    ops[2].work = None
    with pytest.raises(AssertionError):
        ch.big_then_small(ops)


def test_two_handles_alternate_call_by_call():
    a, b = ch.euler(4, 1), ch.euler(3, 2)
    calls = ch.two_handles(a, b)
    assert [i for w, i in calls if w == 0] == a and [i for w, i in calls if w == 1] == b
    assert [w for w, _ in calls[:2 * len(b)]] == [0, 1] * len(b)        # strictly one after the other while both last
    assert all(w == 0 for w, _ in calls[2 * len(b):])


# ---- the configurations ---------------------------------------------------------------------------------------------------------------------------
def names_compared_in(function, src):
    """the string literals the body of `function` in capi.hip compares its name argument with; the body by its braces, wherever the function stands"""
    at = src.index("\nint %s(" % function)
    i, depth = src.index("{", at), 0
    while True:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
        if depth == 0:
            break
    return set(re.findall(r'"(\w+)"', "".join(re.findall(r'n == "\w+"', src[at:i]))))


def test_every_operation_sets_every_option_the_library_accepts(fray, abi):
    """The accepted names are abi.OPTION_NAMES, which Scene.set_option documents and the source of frayhip_scene_set_option must agree with (a handle, which
    needs a GPU, is probed with them in tests/test_gpu_call_history.py): a new option fails here until the operations set it."""
    accepted = set(abi.OPTION_NAMES)
    assert len(abi.OPTION_NAMES) == len(accepted) >= 9 and accepted == set(ch.OPTION_DEFAULTS), accepted ^ set(ch.OPTION_DEFAULTS)
    assert set(abi.FIGURE_NAMES) == set(ch.FIGURES)
    doc = fray.Scene.set_option.__doc__
    assert all('"%s"' % name in doc for name in accepted), [n for n in accepted if '"%s"' % n not in doc]     # and Scene.set_option documents each
    src = open(os.path.join(ROOT, "fray_amd", "csrc", "capi.hip")).read()
    assert names_compared_in("frayhip_scene_set_option", src) == accepted
    assert names_compared_in("frayhip_scene_get_option", src) == accepted | set(abi.FIGURE_NAMES)
    # the defaults a handle is created with: render_state.hpp's
    state = open(os.path.join(ROOT, "fray_amd", "csrc", "render_state.hpp")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, state).group(1))
    member = lambda decl: re.search(r"\b%s = (\w+);" % re.escape(decl), state).group(1)
    assert ch.OPTION_DEFAULTS == dict(pt_lanes=define("FRAY_PT_LANES"), pt_budget_mib=define("FRAY_PT_BUDGET_MIB"), seed_table_mib=define("FRAY_SEED_TABLE_MIB"),
                                      speculate_fans=int(member("bool speculateFans") == "true"), fused_whitted_max=int(member("int fusedWhittedMax")),
                                      fp_contract=int(member("bool fpContract") == "true"), skip_null_segments=int(member("bool skipNullSegments") == "true"),
                                      segment_planes=int(member("bool segmentPlanes") == "true"), certified_segments=int(member("bool certifiedSegments") == "true"))
    # the tight-gates switch is no option name (frayhip_scene_tight_gates): the operations write it all the same, from the default a handle is created with
    assert "tight_gates" not in accepted and ch.TIGHT_GATES_DEFAULT == int(member("bool tightGates") == "true") == 1
    fields = {n for n, _ in abi.Settings._fields_}
    cam = {n for n, _ in abi.Camera._fields_}
    assert set(ch.SETTINGS_SET) <= fields and set(ch.SETTINGS_DEFAULTS) == set(ch.SETTINGS_SET)
    assert set(ch.CAMERA_SET) <= cam and set(ch.CAMERA_DEFAULTS) == set(ch.CAMERA_SET)
    assert set(ch.COUNTERS) == {n for n, _ in abi.Stats._fields_[:len(ch.COUNTERS)]}                           # closest_rays .. texture_fetches
    for name in ch.SCENES:
        ops = ch.operations(name)
        assert len(ops) >= 15 and len({o.name for o in ops}) == len(ops), name
        for o in ops:
            cfg = o.config()
            assert set(cfg["options"]) == accepted, (name, o.name)
            assert cfg["tight_gates"] in (0, 1), (name, o.name)
            assert set(cfg["settings"]) == set(ch.SETTINGS_SET) and set(cfg["camera"]) == set(ch.CAMERA_SET), (name, o.name)
            assert cfg["tables"] in ("original", "edit_node", "edit_other"), (name, o.name)
            assert set(ch.OWNED[o.kind]) <= set(ch.FIGURES), o.name


def test_the_operations_reach_what_the_issue_lists():
    for name in ch.SCENES:
        ops = {o.name: o.config() for o in ch.operations(name)}
        sizes = {(c["settings"]["frameWidth"], c["settings"]["frameHeight"]) for c in ops.values()}
        assert {(64, 48), (97, 61), (33, 17), (32, 24)} <= sizes, name
        for opt, off in (("fp_contract", 1), ("segment_planes", 0), ("certified_segments", 0), ("skip_null_segments", 0), ("seed_table_mib", 0), ("pt_lanes", 1),
                         ("pt_budget_mib", 1), ("fused_whitted_max", 0)):
            assert any(c["options"][opt] == off for c in ops.values()), (name, opt)
        assert any(c["settings"]["maxTraceDepth"] == 40 for c in ops.values()) and any((c["settings"]["maxTraceDepth"] or 0) < 0 for c in ops.values())
        assert any(c["camera"]["stereoSeparation"] for c in ops.values())
        assert {c["tables"] for c in ops.values()} == {"original", "edit_node", "edit_other"}
        assert all(ch.SCENE_FACTS[name][e] for e in ("edit_node", "edit_other"))
    # the tight-gates switch off: one path-traced frame of the scene whose blocks are eligible gates; every other operation writes the default
    for name in ch.SCENES:
        off = [o for o in ch.operations(name) if o.config()["tight_gates"] != ch.TIGHT_GATES_DEFAULT]
        assert [o.name for o in off] == (["pt-no-tight-gates"] if name == "cornell_box" else []), name
        assert all(o.kind == "frame" and o.config()["settings"]["gi"] == 1 and o.config()["options"] == ch.OPTION_DEFAULTS for o in off)


class FakeScene:
    """what Handle.configure and Handle.run call on a fray_amd.Scene, recorded: the switch is state behind the handle as the options are"""
    def __init__(self):
        import types
        self.desc = types.SimpleNamespace(settings=bytearray(8), camera=bytearray(8))
        self.settings, self.camera = types.SimpleNamespace(), types.SimpleNamespace()
        self.options, self.switch, self.log = {}, ch.TIGHT_GATES_DEFAULT, []

    def beginFrame(self):
        self.log.append("beginFrame")

    def set_option(self, name, value):
        self.options[name] = value
        self.log.append("set_option")

    def tight_gates(self, enable=None):
        if enable is not None:
            self.switch = int(bool(enable))
            self.log.append("tight_gates")
        return self.switch, 2

    def get_option(self, name):
        return 0

    def update(self):
        raise AssertionError("no operation here edits a table")


def test_configure_writes_the_switch_before_every_call(monkeypatch):
    """Handle.configure over a fake scene: every operation writes the switch, after the view and the options and before its call -- so the frame of an
    operation does not depend on an earlier operation having flipped it"""
    monkeypatch.setattr(ch.C, "memmove", lambda *a: None)
    monkeypatch.setattr(ch.C, "byref", lambda x: x)
    h = object.__new__(ch.Handle)
    h.s, h.facts, h.settings0, h.camera0, h.tables, h.edited = FakeScene(), ch.SCENE_FACTS["cornell_box"], b"", b"", "original", False
    seen = []
    ops = {o.name: o for o in ch.operations("cornell_box")}
    for name, want in (("pt", 1), ("pt-no-tight-gates", 0), ("pt", 1), ("pt-no-tight-gates", 0), ("pt-no-tight-gates", 0), ("adaptive", 1), ("primary", 1)):
        op = ch.Op(name, lambda hd: seen.append(hd.s.tight_gates()[0]) or {}, ops[name].settings, ops[name].camera, ops[name].options, ops[name].tables,
                   ops[name].kind, ops[name].tight_gates)
        h.s.log = []
        h.run(op)
        assert seen[-1] == want and h.s.switch == want, name
        assert h.s.log.count("tight_gates") == 1 and h.s.log.index("tight_gates") > max(i for i, c in enumerate(h.s.log) if c != "tight_gates"), h.s.log
        assert h.s.options == ch.OPTION_DEFAULTS


# ---- the comparer, over a handle that leaks -----------------------------------------------------------------------------------------------------------
class FakeHandle:
    """render(op) is a function of op alone -- but for one word of its workspace, which `culprit` leaves behind and `victim` reads without writing it"""
    def __init__(self, culprit, victim, name="fake"):
        self.culprit, self.victim, self.word, self.name = culprit, victim, 0.0, name

    def run(self, op):
        i = int(op.name[2:])
        rgb = np.full((4, 5, 3), float(i), np.float32)
        if op.name == self.victim:
            rgb[2, 3, 1] += self.word
        figure = int(self.word * 4)                     # a figure that legitimately tells of the call before
        self.word = 0.25 if op.name == self.culprit else 0.0
        return {"count": 7 * i, "rgb": rgb, "fig:seed_launches": figure}


def test_the_comparer_names_the_call_the_operation_and_its_predecessor():
    n = 6
    ops = [ch.Op("op%d" % i, None) for i in range(n)]
    fresh = [FakeHandle("op4", "op2").run(o) for o in ops]              # every operation as the first call of a handle
    walk = ch.euler(n, 3)
    skip = lambda handle, op: ("fig:seed_launches",)
    found = []
    for a, arc in enumerate(ch.arcs(walk, 8)):
        found += ch.run_walk(FakeHandle("op4", "op2"), ops, arc, fresh, skip, label="arc %d" % a)
    assert len(found) == 1                                              # the pair (op4, op2) is adjacent once in the whole circuit
    f = found[0]
    arc = ch.arcs(walk, 8)[int(f.label.split()[1])]
    assert (f.op, f.predecessor, f.key, f.index) == ("op2", "op4", "rgb", (2, 3, 1))
    assert arc[f.position] == 2 and arc[f.position - 1] == 4
    assert "op2 after op4" in repr(f) and "'rgb'" in repr(f) and "(2, 3, 1)" in repr(f)
    # a handle that leaks nothing: no finding; a figure that is not skipped: found
    assert ch.run_walk(FakeHandle("none", "none"), ops, walk, fresh, skip) == []
    noisy = ch.run_walk(FakeHandle("op4", "none"), ops, walk, fresh)
    assert len(noisy) == n and {(f.key, f.predecessor) for f in noisy} == {("fig:seed_launches", "op4")} and {f.op for f in noisy} == {o.name for o in ops}
    # two handles: the leak stays within its handle, and the predecessor named is the call before on either
    calls = ch.two_handles(walk, walk)
    found = ch.run_two([FakeHandle("op4", "op2", "A"), FakeHandle("none", "none", "B")], [ops, ops], calls, [fresh, fresh], skip)
    assert len(found) == 1 and found[0].op == "A:op2" and found[0].predecessor == "B:op4"          # B's call lies between A's op4 and A's op2


def test_first_difference():
    a = {"x": np.arange(12, dtype=np.float64).reshape(3, 4), "n": 3}
    assert ch.first_difference(a, {"x": a["x"].copy(), "n": 3}) is None
    b = a["x"].copy()
    b[1, 2] = np.nextafter(b[1, 2], 99)
    assert ch.first_difference(a, {"x": b, "n": 3}) == ("x", (1, 2))
    assert ch.first_difference(a, {"x": a["x"].astype(np.float32), "n": 3}) == ("x", None)
    assert ch.first_difference(a, {"x": a["x"], "n": 4}) == ("n", None)
    assert ch.first_difference(a, {"x": a["x"], "n": 4}, skip=("n",)) is None
    assert ch.first_difference(a, {"x": a["x"]}) == ("n", None)
    assert ch.first_difference(a, {"x": a["x"], "n": 3, "more": 1}) == ("more", None)
    z = {"x": np.array([0.0, -0.0])}
    assert ch.first_difference({"x": np.array([0.0, 0.0])}, z) == ("x", (1,))            # bytes, not values
