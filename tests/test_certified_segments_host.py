"""Certified segments on the CPU (option "certified_segments"; DESIGN.md "Certified segments"; tests/native/certseg/certseg_host.cpp).

path_shade stores the term of a next-event segment itself, without a queue entry and without visible(), when the segment's ray is proven to miss every
gate and its ends lie on one side of every plane entry of a scene whose nodes are all plane nodes or exactly gated ones.  The harness runs that rule --
the kernels' own functions of fray_amd/csrc/dev_trace.hpp -- as one lane over the arena that arena_dump writes, beside visible<0>'s answer.  Builds: (a)
AddressSanitizer + UndefinedBehaviorSanitizer, (b) plain, whose result files must be the same bytes, and (c) with the margins of both certificates removed
(-DFRAY_SEGCERT_SCALE=0 -DFRAY_MISSCERT_SCALE=0), which must show a wrong certificate on cornell_box."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hostlane as hl
from conftest import SCENES
from test_gpu_rays import _oracle_visible
from test_gpu_segment_planes import GENERATED as ROOMS

SRC = os.path.join(hl.ROOT, "tests", "native", "certseg", "certseg_host.cpp")
BUILDS = {
    "asan": hl.BUILDS["asan"],
    "plain": hl.BUILDS["plain"],
    "noscale": hl.BUILDS["plain"] + ["-DFRAY_SEGCERT_SCALE=0", "-DFRAY_MISSCERT_SCALE=0"],
}
# what the issue's table states outright; every scene is also checked against the rule restated below
STATED = {"cornell_box": True, "one wall with a transform": False, "a one-triangle and a five-triangle mesh": True}
CASES = ["cornell_box"] + list(ROOMS)


def command(build, exe):
    return [hl.CLANG, "-std=c++17", "-ffp-contract=off"] + BUILDS[build] + hl.INC + [SRC, "-o", exe]


class Harness:
    def __init__(self, root):
        self.root = root
        self.exe = {b: str(root / ("certseg_host_" + b)) for b in BUILDS}
        self.dump = str(root / "arena_dump")
        hl.build_parallel([command(b, self.exe[b]) for b in BUILDS] + [hl.arena_dump_command(self.dump)])
        self.n = 0

    def arena(self, scene_path):
        self.n += 1
        out = str(self.root / ("arena%d.bin" % self.n))
        r = subprocess.run([self.dump, scene_path, out], capture_output=True, text=True, timeout=600,
                           env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr[-3000:]
        return out

    def run(self, build, arena, rays):
        res = str(self.root / ("result_%s.bin" % build))
        r = subprocess.run([self.exe[build], arena, rays, res], capture_output=True, text=True, timeout=600, env={**os.environ, **hl.SAN_ENV})
        assert r.returncode == 0 and r.stderr == "" and r.stdout == "", "build %s: exit %d\n%s" % (build, r.returncode, (r.stdout + r.stderr)[-6000:])
        raw = open(res, "rb").read()
        os.remove(res)
        assert raw[:8] == b"FRAYCSG1"
        n, eligible, n_gates, n_planes = struct.unpack_from("<QQQQ", raw, 8)
        body = np.frombuffer(raw, np.uint8, 4 * n, 40).astype(bool).reshape(4, n)
        assert 40 + 4 * n == len(raw)
        return {"raw": raw, "eligible": bool(eligible), "gates": n_gates, "plane_entries": n_planes,
                "planes": body[0], "gate_free": body[1], "certified": body[2], "vis": body[3]}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(tmp_path_factory.mktemp("certseg"))


def eligible_by_rule(desc):
    """The rule of scene_arena.hpp fill_editable, restated: every node is an untransformed mesh without a KD-tree that is either small (fewer than
    FRAY_GATE_MIN_TRIS = 6 triangles, each with a usable normal: a plane node) or large (a gated node; its gate is exact because it is untransformed), and
    the tables hold them: at most 16 plane nodes, 16 plane entries (triangles with the same N and fl(N . A) share one) and 8 gates.  And the certificate can
    hold for some next-event segment at all: there is a light, and no plane entry contains every light whole (a point light's position, a RectLight's four
    corners, within the entry's least margin t0 = c n1 (Amax + 1), dev_segcert.hpp segcert_make) -- a segment ends on a light, and the rule needs every entry; and some plane node can start one: a segment
    starts 1e-6 off its surface along the unit normal, which clears the node's own planes only where 1e-6 |N|_2 > t0 (a start on a gated node lies in its gate)."""
    planes, plane_nodes, gates, own = {}, 0, 0, []
    for i in range(desc.n_nodes):
        node = desc.nodes[i]
        g = desc.geoms[node.geom]
        identity = list(node.T.offset[:]) == [0.0] * 3 and list(node.T.m[:]) == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0] and list(node.T.invM[:]) == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
        if g.kind != 3 or not identity:
            return False
        m = desc.meshes[g.index]
        if m.has_kd or m.n_triangles <= 0:
            return False
        if m.n_triangles >= 6:
            gates += 1
            continue
        plane_nodes += 1
        own.append(set())
        for t in range(m.n_triangles):
            T = m.triangles[t]
            N = [float(x) for x in T.ABcrossAC[:]]
            A = [float(m.vertices[3 * T.v[0] + q]) for q in range(3)]
            n1 = sum(abs(x) for x in N)
            if not (np.isfinite(N + A).all() and max(abs(x) for x in A) <= 2.0 ** 40 and 2.0 ** -80 <= n1 <= 2.0 ** 90):
                return False
            key = (tuple(N), N[0] * A[0] + N[1] * A[1] + N[2] * A[2])
            planes[key] = max(planes.get(key, 0.0), max(abs(x) for x in A))
            own[-1].add(key)
    if not (plane_nodes <= 16 and len(planes) <= 16 and gates <= 8 and desc.n_lights > 0):
        return False
    points = []
    for i in range(desc.n_lights):
        l = desc.lights[i]
        if l.kind == 0:
            points.append([float(x) for x in l.pos[:]])
        else:
            points += [[px * l.T.m[k] + pz * l.T.m[6 + k] + l.T.offset[k] for k in range(3)] for px in (-0.5, 0.5) for pz in (-0.5, 0.5)]
    t0 = {}
    for (N, k), amax in planes.items():
        t1 = 2.0 ** -36 * sum(abs(x) for x in N) * (1.0 + 2.0 ** -40)
        t0[(N, k)] = t1 * (amax + 1.0) * (1.0 + 2.0 ** -40)
        if not any(abs(N[0] * w[0] + N[1] * w[1] + N[2] * w[2] - k) > t0[(N, k)] for w in points):
            return False
    return any(all(1e-6 * float(np.sqrt(key[0][0] * key[0][0] + key[0][1] * key[0][1] + key[0][2] * key[0][2])) > t0[key] for key in keys) for keys in own)


def scene_and_segments(fray, what, tmp_path):
    path = os.path.join(SCENES, "cornell_box.fray") if what == "cornell_box" else ROOMS[what][0](tmp_path)
    s = fray.Scene.parseScene(path)
    a, b = hl.wall_segments(s.desc, 33, per=60)
    assert len(a) >= 3000
    rays = str(tmp_path / "segments.bin")
    hl.write_rays(rays, np.zeros((0, 3)), np.zeros((0, 3)), a, b)
    return s, path, a, b, rays


@pytest.mark.parametrize("what", CASES, ids=lambda v: v.replace(" ", "_").replace(",", ""))
def test_certified_segments_are_visible(fray, abi, oracle, harness, tmp_path, what):
    """Segments with ends from far outside down to inside the margin on both sides of every wall and block plane: eligibility is what the scene's nodes
    imply; every certified segment is visible to visible<0> and to the CPU oracle; an eligible scene has certified segments and visible ones that are not
    certified; an ineligible scene has none certified."""
    s, path, a, b, rays = scene_and_segments(fray, what, tmp_path)
    arena = harness.arena(path)
    r = harness.run("asan", arena, rays)
    assert harness.run("plain", arena, rays)["raw"] == r["raw"], "the plain build's result differs from the sanitizer build's"
    want = _oracle_visible(oracle, abi, s.desc, a, b)
    eligible = eligible_by_rule(s.desc)
    cert, vis = r["certified"], r["vis"]
    print("%s: eligible %s (%d gates, %d plane entries); %d segments, %.3f visible, planes pass %.3f, gate-free %.3f, certified %.3f, visible and not certified %.3f"
          % (what, r["eligible"], r["gates"], r["plane_entries"], len(a), float(vis.mean()), float(r["planes"].mean()), float(r["gate_free"].mean()),
             float(cert.mean()), float((vis & ~cert).mean())))
    assert r["eligible"] == eligible
    if what in STATED:
        assert eligible == STATED[what]
    assert np.array_equal(vis, want), np.argwhere(vis != want)[:5].ravel()
    assert vis[cert].all() and want[cert].all(), np.argwhere(cert & ~(vis & want))[:5].ravel()
    if eligible:
        assert np.array_equal(cert, r["planes"] & r["gate_free"])
        assert cert.any() and (vis & ~cert).any()
    else:
        assert not cert.any()
    s.close()


def test_without_the_margins_a_wrong_certificate_is_seen(fray, harness, tmp_path):
    """The build with FRAY_SEGCERT_SCALE = FRAY_MISSCERT_SCALE = 0 on cornell_box's segments of the test above: at least one segment is certified although
    visible<0> (the same build's, whose arithmetic the scales do not touch) says occluded -- the harness can see a wrong certificate."""
    s, path, a, b, rays = scene_and_segments(fray, "cornell_box", tmp_path)
    arena = harness.arena(path)
    r, loose = harness.run("plain", arena, rays), harness.run("noscale", arena, rays)
    assert np.array_equal(loose["vis"], r["vis"])
    wrong = loose["certified"] & ~loose["vis"]
    print("cornell_box without the margins: %d of %d segments certified (%d with them), %d of them occluded" % (loose["certified"].sum(), len(a), r["certified"].sum(), wrong.sum()))
    assert not (r["certified"] & ~r["vis"]).any()
    assert wrong.sum() >= 1
    s.close()
