"""Ties the code the sanitizers saw (tests/test_trace_host.py: the traversal headers compiled for the host) to the code the GPU runs: for one scene per
timed flag word, the adversarial rays and segments of the host lane through s.trace_rays(record=True) and s.visible, with and without stats=True,
against the plain -O1 build of tests/native/hostlane/trace_host.cpp -- ids, dist, ip and normal bit for bit, u, v by test_gpu_rays' sphere rule.
The harness never opens the GPU; it and its compiler are started through conftest's run_in_clean_child, never by a fork from this process."""
import os

import numpy as np
import pytest

import hostlane as hl
from conftest import run_in_clean_child
from test_gpu_rays import SPHERE_UV_ULPS, _has_sphere
from test_trace_host import ADVERSARIAL, adversarial_case

pytestmark = pytest.mark.gpu

SCENES_BY_WORD = [("cornell_box", 0), ("boxed", 4), ("csg_nested", 2), ("textured_plain", 8)]
CAP = 4096


def _child(cmd, log, env=None):
    out = run_in_clean_child(cmd, str(log), timeout=300, env=env)
    assert "[exit code 0]" in out, " ".join(cmd) + "\n" + out[-4000:]
    return out.replace("[exit code 0]", "").strip()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    root = tmp_path_factory.mktemp("hostlane_gpu")
    exe, dump = str(root / "trace_host_plain"), str(root / "arena_dump")
    _child(hl.trace_host_command("plain", exe), root / "build_trace.log")
    _child(hl.arena_dump_command(dump, sanitize=False), root / "build_dump.log")
    return root, exe, dump


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("name,word", SCENES_BY_WORD, ids=[n for n, _ in SCENES_BY_WORD])
def test_gpu_answers_equal_the_host_lane(fray, oracle, gpu, built, tmp_path, name, word):
    root, exe, dump = built
    assert ADVERSARIAL[name][1] == word
    s, path, o, d, cat, ids, rec, a, b = adversarial_case(fray, oracle, name, tmp_path)
    # at most CAP of each, every category kept: an even stride over the set
    ko, ka = np.arange(len(o))[::max(1, -(-len(o) // CAP))], np.arange(len(a))[::max(1, -(-len(a) // CAP))]
    o, d, a, b = (np.ascontiguousarray(x) for x in (o[ko], d[ko], a[ka], b[ka]))
    assert 1000 <= len(o) <= CAP and 200 <= len(a) <= CAP
    arena, rays, res = str(tmp_path / "arena.bin"), str(tmp_path / "rays.bin"), str(tmp_path / "result.bin")
    hl.write_rays(rays, o, d, a, b)
    _child([dump, path, arena], tmp_path / "dump.log")
    assert _child([exe, arena, rays, res], tmp_path / "trace.log") == ""
    host = hl.read_result(res)
    assert host["word"] == word

    s.beginRender()
    for stats in (False, True):
        what = "%s stats=%s" % (name, stats)
        g = s.trace_rays(o, d, record=True, stats=stats)
        gid, gdist, grec = g["hit_id"], g["hit_dist"], g["hit_rec"]
        assert np.array_equal(gid, host["hit_id"]), (what, np.argwhere(gid != host["hit_id"])[:5].ravel())
        assert np.array_equal(_bits(gdist), _bits(host["hit_rec"][:, 0])), what
        same7 = (_bits(grec[:, :7]) == _bits(host["hit_rec"][:, :7])).all(axis=1)
        assert same7.all(), (what, "dist / ip / normal differ", np.argwhere(~same7)[:5].ravel())
        # u, v: the device's atan2 / asin are not glibc's in the last place -- a sphere's u, v within SPHERE_UV_ULPS x 2^-52, every other winner's the same bits
        uv_diff = (_bits(grec[:, 7:]) != _bits(host["hit_rec"][:, 7:])).any(axis=1)
        sphere = np.array([i >= 0 and _has_sphere(s.desc, s.desc.nodes[int(i)].geom) for i in gid], bool)
        assert not (uv_diff & ~sphere).any(), (what, "u, v differ on a winner without a sphere", np.argwhere(uv_diff & ~sphere)[:5].ravel())
        if uv_diff.any():
            assert np.abs(grec[uv_diff, 7:] - host["hit_rec"][uv_diff, 7:]).max() <= SPHERE_UV_ULPS * 2.0 ** -52, what
        vis, st = s.visible(a, b, stats=stats)
        assert np.array_equal(vis, host["vis"]), (what, np.argwhere(vis != host["vis"])[:5].ravel())
        if stats:
            assert g["stats"]["closest_rays"] == len(o) and st["shadow_rays"] == len(a)
            for k in ("node_tests", "kd_inner_visits", "leaf_refs", "tri_tests", "prim_tests", "smooth_hits"):
                assert g["stats"][k] == host["cnt_closest"][k], (what, k, g["stats"][k], host["cnt_closest"][k])
        print("%s: %d rays (%d hits), %d segments (%d visible), %d sphere u, v differ (<= %d x 2^-52)"
              % (what, len(o), int((gid != -1).sum()), len(a), int(vis.sum()), int(uv_diff.sum()), SPHERE_UV_ULPS))
    s.close()
