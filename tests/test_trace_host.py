"""The device's traversal code on the CPU, under sanitizers (tests/native/hostlane; DESIGN.md "The traversal on the host").

closest_hit, node_intersect, the KD walk, the CSG paths, finalize_hit, light_record, visible and the segment-plane copy of visible with
segment_skip_nodes are compiled for the host as one lane of a wave, unedited, and run over the scene arena that frayhip_scene_create's own builder
(fray_amd/csrc/scene_arena.hpp) makes, every table in a heap block of its own.  Five builds of the harness:
  (a) AddressSanitizer + UndefinedBehaviorSanitizer (+ float-cast-overflow), (b) MemorySanitizer with origins, (c) / (d) every automatic variable
  preset to a pattern / to zero, (e) the uninitialised-variable warnings as errors.
Every run of (a) and (b) must exit 0 and print nothing; the result files of (a), (b), (c) and (d) must be the same bytes (Lane.trace checks both for
every input of every test below).  The answers are compared with the reference's own records (tests/golden/ref_*.npz) and with the CPU oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hostlane as hl
from conftest import ROOT, SCENES, open_scene
from test_gpu_parity import COUNTERS, TEXTURED_PLAIN_SCENE
from test_gpu_rays import SPHERE_UV_ULPS, _check_records, _oracle_visible, _segments
from test_gpu_segment_planes import GENERATED as ROOMS
from test_oracle_vs_ref import FIXTURES, load_case

COMPARED = ("asan", "msan", "pattern", "zero")
TOTALS = {"rays": {}, "segments": {}, "sphere_uv": 0, "room_segments": 0, "room_skipping": 0, "fixture_words": set(), "fixtures": 0}


class Lane:
    """The built harness.  trace() runs one input through the four compared builds and returns build (a)'s result."""

    def __init__(self, root):
        self.root = root
        self.exe = {b: str(root / ("trace_host_" + b)) for b in COMPARED}
        self.dump = str(root / "arena_dump")
        self.arenas = {}
        self.n = 0
        hl.build_parallel([hl.trace_host_command(b, self.exe[b]) for b in COMPARED] + [hl.warnings_command(str(root / "trace_host_warn.o")),
                                                                                         hl.arena_dump_command(self.dump)])

    def arena(self, scene_path, env_unloaded=False):
        key = (os.path.abspath(scene_path), bool(env_unloaded))
        if key not in self.arenas:
            out = str(self.root / ("arena%d.bin" % len(self.arenas)))
            r = subprocess.run([self.dump] + (["--env-unloaded"] if env_unloaded else []) + [key[0], out], capture_output=True, text=True, timeout=600,
                               env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
            assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr[-3000:]
            self.arenas[key] = out
        return self.arenas[key]

    def trace(self, arena, o, d, a, b, builds=COMPARED):
        self.n += 1
        rays = str(self.root / ("rays%d.bin" % self.n))
        hl.write_rays(rays, o, d, a, b)
        raws, first = [], None
        for bld in builds:
            res = str(self.root / ("result%d_%s.bin" % (self.n, bld)))
            r = subprocess.run([self.exe[bld], arena, rays, res], capture_output=True, text=True, timeout=600, env={**os.environ, **hl.SAN_ENV})
            assert r.returncode == 0 and r.stderr == "" and r.stdout == "", "build %s: exit %d\n%s" % (bld, r.returncode, (r.stdout + r.stderr)[-6000:])
            got = hl.read_result(res)
            raws.append(got["raw"])
            first = first or got
            os.remove(res)
        os.remove(rays)
        for bld, raw in zip(builds[1:], raws[1:]):
            assert raw == raws[0], "the result of build %s differs from build %s's: an uninitialised value reached a result" % (bld, builds[0])
        w = first["word"]
        TOTALS["rays"][w] = TOTALS["rays"].get(w, 0) + len(first["hit_id"])
        TOTALS["segments"][w] = TOTALS["segments"].get(w, 0) + len(first["vis"])
        return first


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    return Lane(tmp_path_factory.mktemp("hostlane"))


def flag_word(desc):
    """entry_support.hpp flag_word for a description: Cube / CSG nodes, else KD meshes, else textures or a loaded environment"""
    if any(desc.geoms[desc.nodes[i].geom].kind in (2, 4) for i in range(desc.n_nodes)):
        return 2
    if any(desc.meshes[i].has_kd for i in range(desc.n_meshes)):
        return 4
    return 8 if desc.n_textures > 0 or (desc.environment.present and desc.environment.loaded) else 0


def check_counting_word(r, what):
    assert np.array_equal(r["hit_id_c"], r["hit_id"]), what
    assert np.array_equal(r["hit_rec_c"].view(np.uint64), r["hit_rec"].view(np.uint64)), what
    assert np.array_equal(r["vis_c"], r["vis"]), what
    assert r["cnt_closest"]["closest_rays"] == len(r["hit_id"]) and r["cnt_visible"]["shadow_rays"] == len(r["vis"]), what
    assert r["cnt_closest"]["envelope"] == 0 and r["cnt_visible"]["envelope"] == 0, what


def check_against_oracle(r, ids, rec, what):
    """ids, dist, ip, normal, u, v of the harness against fray_oracle_probe's, bit for bit (both call glibc); a miss is 1e99 and zeros"""
    assert np.array_equal(r["hit_id"], ids), (what, np.argwhere(r["hit_id"] != ids)[:5].ravel())
    miss, light, node = ids == -1, ids <= -2, ids >= 0
    got = r["hit_rec"]
    assert (got[miss, 0] == 1e99).all() and (got[miss, 1:] == 0).all(), what
    assert np.array_equal(got[light, :7].view(np.uint64), rec[light, :7].view(np.uint64)) and (got[light, 7:] == 0).all(), what
    same = (got[node].view(np.uint64) == rec[node].view(np.uint64)).all(axis=1)
    assert same.all(), (what, "records differ", np.argwhere(node)[~same][:5].ravel())


def check_segments(r, want, what):
    assert np.array_equal(r["vis"], want), (what, np.argwhere(r["vis"] != want)[:5].ravel())
    if r["segp"]:
        assert np.array_equal(r["vis_p"], r["vis"]), (what, "the segment-plane copy of visible() differs", np.argwhere(r["vis_p"] != r["vis"])[:5].ravel())
    else:
        assert not r["vis_p"].any() and not r["skip"].any(), what


# ---- the reference's own records ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[4:-4])
def test_fixture_rays_equal_reference_records(fray, abi, oracle, lane, path):
    z, s = load_case(fray, path)
    name = os.path.basename(path)
    env_unloaded = bool(s.desc.environment.present and not s.desc.environment.loaded)
    a, b = _segments(s.desc, z, 11)
    r = lane.trace(lane.arena(os.path.join(SCENES, str(z["scene"])), env_unloaded), z["ray_start"], z["ray_dir"], a, b)
    assert r["word"] == flag_word(s.desc), name
    TOTALS["fixture_words"].add(r["word"])
    TOTALS["fixtures"] += 1
    # hit_id equal, rec[:7] bit-equal for nodes and lights, u, v bit-equal but for a sphere's within SPHERE_UV_ULPS (counted and printed)
    n = _check_records(s, z, r["hit_id"], r["hit_rec"], name)
    TOTALS["sphere_uv"] += n
    print("%s: word %d, %d rays, %d segments, %d sphere u, v differ (<= %d x 2^-52)" % (name, r["word"], len(r["hit_id"]), len(a), n, SPHERE_UV_ULPS))
    check_counting_word(r, name)
    check_segments(r, _oracle_visible(oracle, abi, s.desc, a, b), name)
    s.close()


# ---- adversarial rays and segments --------------------------------------------------------------------------------------------------------------
def _textured_plain(tmp_path):
    shutil.copy(os.path.join(ROOT, "tests", "scenes", "plates.obj"), tmp_path / "plates.obj")
    f = tmp_path / "textured_plain.fray"
    f.write_text(TEXTURED_PLAIN_SCENE % ("gi off", "plates.obj"))
    return str(f)


ADVERSARIAL = {
    "cornell_box": (lambda p: os.path.join(SCENES, "cornell_box.fray"), 0),
    "boxed": (lambda p: os.path.join(SCENES, "boxed.fray"), 4),
    "forest": (lambda p: os.path.join(SCENES, "forest.fray"), 4),
    "dragon": (lambda p: os.path.join(SCENES, "hw9", "dragon.fray"), 4),
    "csg_nested": (lambda p: os.path.join(ROOT, "tests", "scenes", "csg_nested.fray"), 2),
    "csg_deep": (lambda p: os.path.join(ROOT, "tests", "scenes", "csg_deep.fray"), 2),
    "textured_plain": (_textured_plain, 8),
}


def adversarial_case(fray, oracle, name, tmp_path, seed=20):
    """(scene, its file, rays, their categories, the oracle's ids and records, segments) -- shared with tests/test_gpu_trace_host.py"""
    make, word = ADVERSARIAL[name]
    path = make(tmp_path)
    s = fray.Scene.parseScene(path)
    s.settings.frameWidth, s.settings.frameHeight = 64, 48
    assert flag_word(s.desc) == word
    o, d, cat = hl.adversarial_rays(oracle, s.desc, seed)
    ids, rec = hl.oracle_probe(oracle, s.desc, o, d)
    a, b = _segments(s.desc, {"hit_id": ids, "hit_rec": rec}, seed + 1)
    wa, wb = hl.wall_segments(s.desc, seed + 2)
    return s, path, o, d, cat, ids, rec, np.concatenate([a, wa]), np.concatenate([b, wb])


@pytest.mark.parametrize("name", list(ADVERSARIAL))
def test_adversarial_rays_equal_oracle(fray, abi, oracle, lane, tmp_path, name):
    """Self-hits, exact zero and 1e-300 components, origins at 1e6, rays in bounding-box faces and KD split planes, through vertices and along edges,
    grazing sphere and cube silhouettes, from inside CSG operands (tests/hostlane.py adversarial_rays); segments from hit points to the lights and to
    random points, and around the planes of the tree-less meshes."""
    s, path, o, d, cat, ids, rec, a, b = adversarial_case(fray, oracle, name, tmp_path)
    share = float((ids != -1).mean())
    print("%s: %d rays (%s), hits %.3f; %d segments" % (name, len(o), ", ".join("%s %d" % (c, (cat == c).sum()) for c in sorted(set(cat))), share, len(a)))
    assert len(o) >= 2000 and 0.1 < share < 0.9
    need = {"self-hit", "zero-component", "far-origin", "box-face-or-split-plane", "vertex", "edge"}
    if ADVERSARIAL[name][1] == 2:
        need |= {"silhouette", "inside-csg-operand"}
    if name == "textured_plain":
        need |= {"silhouette"}
    assert need <= set(cat), need - set(cat)
    r = lane.trace(lane.arena(path), o, d, a, b)
    assert r["word"] == ADVERSARIAL[name][1]
    check_against_oracle(r, ids, rec, name)
    check_counting_word(r, name)
    check_segments(r, _oracle_visible(oracle, abi, s.desc, a, b), name)
    s.close()


ROOM_CASES = ["cornell_box"] + list(ROOMS)


@pytest.mark.parametrize("what", ROOM_CASES, ids=lambda v: v.replace(" ", "_").replace(",", ""))
def test_room_segments_and_the_segment_plane_shortcut(fray, abi, oracle, lane, tmp_path, what):
    """Segments with ends from far outside down to inside the certificate's margin on both sides of every wall and block plane, nearly parallel to one,
    and ending on and just beyond a face: visible<0> equals the oracle, the SEGP copy equals visible<0> on every one, and it skips some."""
    path = os.path.join(SCENES, "cornell_box.fray") if what == "cornell_box" else ROOMS[what][0](tmp_path)
    s = fray.Scene.parseScene(path)
    a, b = hl.wall_segments(s.desc, 33, per=60)
    assert len(a) >= 3000
    want = _oracle_visible(oracle, abi, s.desc, a, b)
    r = lane.trace(lane.arena(path), np.zeros((0, 3)), np.zeros((0, 3)), a, b)
    assert r["word"] == 0 and r["segp"]
    check_segments(r, want, what)
    check_counting_word(r, what)
    # One lane is a wave of one segment: nearly every segment leaves some wall wholly on one side, so the share that skips a node is high.  The sets
    # are made so that both halves of visible()'s loop run: segments that skip a node, and segments that must still ask an eligible node (they
    # cross its plane or end within the margin).
    eligible = sum(1 for i in range(s.desc.n_nodes) if s.desc.geoms[s.desc.nodes[i].geom].kind == 3)        # an upper bound: the tree-less meshes
    nskip = np.array([bin(int(v)).count("1") for v in r["skip"]])
    skipping, all_bits = int((nskip > 0).sum()), int(np.bitwise_or.reduce(r["skip"]))
    asking = int((nskip < bin(all_bits).count("1")).sum())
    TOTALS["room_segments"] += len(a)
    TOTALS["room_skipping"] += skipping
    print("%s: %d segments, %.3f visible; the shortcut skipped a node on %.3f of them (%.2f nodes a segment of %d that are ever skipped), and still asked "
          "such a node on %.3f" % (what, len(a), float(want.mean()), skipping / len(a), float(nskip.mean()), bin(all_bits).count("1"), asking / len(a)))
    assert 0.05 < want.mean() < 0.95
    assert skipping > 0 and asking > 0 and bin(all_bits).count("1") <= eligible
    assert (r["skip"] < (1 << 16)).all()                      # at most FRAY_SEG_MAX_NODES bits
    s.close()


# ---- counters ---------------------------------------------------------------------------------------------------------------------------------
# the scenes of test_gpu_parity.test_primary_hits_bit_exact_vs_oracle_ragged_sizes, whose GPU counters equal the oracle's
COUNTER_SCENES = ["boxed.fray", "forest.fray", "smallpt.fray", "hw9/dragon.fray", "cornell_box.fray", "hw12/sphtri.fray", "hw10/bokeh.fray",
                  "hw9/axe_test.fray", "hw9/nonconvex.fray"]
# what closest_hit and the code under it count; shadow_rays, samples and texture_fetches belong to code the harness does not run (zero on both sides
# but for samples, which the frame kernels count per pixel)
TRAVERSAL_COUNTERS = [k for k in COUNTERS if k not in ("samples",)]


@pytest.mark.parametrize("scene", COUNTER_SCENES)
def test_host_counters_equal_oracle(fray, abi, oracle, lane, scene):
    s = open_scene(fray, scene, 64, 48, wantAA=0)
    o, d = hl.camera_rays(oracle, s.desc, 64, 48)
    oi, od, ost = oracle.render(s.desc, abi.MODE_PRIMARY_ID)
    r = lane.trace(lane.arena(os.path.join(SCENES, scene)), o, d, np.zeros((0, 3)), np.zeros((0, 3)))
    assert np.array_equal(r["hit_id"], oi.ravel()) and np.array_equal(r["hit_rec"][:, 0], od.ravel())
    got = dict(r["cnt_closest"], shadow_rays=r["cnt_visible"]["shadow_rays"])
    print(scene, {k: got[k] for k in TRAVERSAL_COUNTERS})
    for k in TRAVERSAL_COUNTERS:
        assert got[k] == ost[k], (k, got[k], ost[k])
    check_counting_word(r, scene)
    s.close()


# ---- the harness sees what it is there for ------------------------------------------------------------------------------------------------------
def test_the_sanitizer_builds_report_a_planted_overrun_and_a_planted_uninitialised_read(lane, tmp_path):
    """trace_host built with HOSTLANE_SELFTEST: (1) the node loop runs one node past the node table -- AddressSanitizer reports it, because the table is
    a heap block of its own; (2) a field of an untraced ray's record that nothing wrote reaches the output -- MemorySanitizer reports it, and the
    pattern and zero builds write different bytes."""
    exe = {k: str(tmp_path / ("selftest_" + k)) for k in ("asan1", "msan2", "pattern2", "zero2")}
    cmds = []
    for k, e in exe.items():
        c = hl.trace_host_command(k[:-1], e)
        cmds.append(c[:-3] + ["-DHOSTLANE_SELFTEST=" + k[-1]] + c[-3:])
    hl.build_parallel(cmds)
    arena = lane.arena(os.path.join(SCENES, "cornell_box.fray"))
    rays = str(tmp_path / "rays.bin")
    hl.write_rays(rays, [[12345.0, 50.0, -100.0], [278.0, 273.0, -800.0]], [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], np.zeros((0, 3)), np.zeros((0, 3)))
    out = {}
    for k, e in exe.items():
        out[k] = subprocess.run([e, arena, rays, str(tmp_path / (k + ".bin"))], capture_output=True, text=True, timeout=300, env={**os.environ, **hl.SAN_ENV})
    assert out["asan1"].returncode != 0 and "heap-buffer-overflow" in out["asan1"].stderr, out["asan1"].stderr[-2000:]
    assert out["msan2"].returncode != 0 and "use-of-uninitialized-value" in out["msan2"].stderr, out["msan2"].stderr[-2000:]
    assert out["pattern2"].returncode == 0 and out["zero2"].returncode == 0
    assert open(tmp_path / "pattern2.bin", "rb").read() != open(tmp_path / "zero2.bin", "rb").read()


def test_no_suppression_names_a_device_header():
    """No ignore-list, suppression file or no_sanitize attribute anywhere in the harness: the device headers are checked as they are."""
    files = [os.path.join(hl.HL, f) for f in os.listdir(hl.HL)] + [os.path.join(hl.HL, "hip", "hip_runtime.h"), hl.__file__.replace(".pyc", ".py")]
    for f in files:
        if os.path.isfile(f):
            text = open(f).read()
            for word in ("no_sanitize", "ignorelist", "blacklist", "suppressions="):
                assert word not in text, (f, word)


def test_host_lane_report(lane):
    """(runs last) the figures the pull request reports"""
    for w in sorted(set(TOTALS["rays"]) | set(TOTALS["segments"])):
        print("flag words %d and %d: %d rays, %d segments through each of the four builds" % (w, w | 1, TOTALS["rays"].get(w, 0), TOTALS["segments"].get(w, 0)))
    if TOTALS["room_segments"]:
        print("the segment-plane shortcut skipped a node on %.3f of %d room segments" % (TOTALS["room_skipping"] / TOTALS["room_segments"], TOTALS["room_segments"]))
    print("sphere u, v differing from the reference's: %d" % TOTALS["sphere_uv"])
    if TOTALS["fixtures"] == len(FIXTURES):                  # the whole module ran: the fixtures cover the four timed flag words
        assert TOTALS["fixture_words"] >= {0, 2, 4, 8}, TOTALS["fixture_words"]
