"""Answers must not depend on who shares a wave (DESIGN.md "What the wave compositions show").

The device lets a lane's control flow depend on its wave: box_test_pre's __any exits, the identity shortcut's !__any(zeros), segment_skip_nodes' ballots
over the live lanes, the path tracer's queue filing by ray_gate_class, dead slots inside live waves, the KD walk's LDS columns.  Each claims not to
change any lane's result bits.  The query entries let the caller choose the waves -- rows [64 t, 64 t + 64) of a call are one wave, a degenerate row is
a lane that never enters the trace, and a path-traced shade_rays starts row i in slot i with the generator of keys[i] -- so here the same rays, segments
and paths run in the row orders of tests/wave_compositions.py.  The natural order is first held to the reference by the suite's own rules (oracle
records by test_gpu_rays._check_records, frames by bits); every other order must then give each base item the natural order's bits."""
import time

import numpy as np
import pytest

import hostlane as hl
import wave_compositions as wc
from conftest import open_scene
from test_gpu_rays import SPHERE_UV_ULPS, _check_records, _oracle_visible
from test_gpu_segment_planes import GENERATED as ROOMS
from test_gpu_shade import jitter, pixel_grid, pt_by_samples, sample_seed, whitted_single_sample
from test_gpu_trace_host import CAP, SCENES_BY_WORD
from test_trace_host import ADVERSARIAL, adversarial_case

pytestmark = pytest.mark.gpu

MAX_ROWS = 262144                 # rows per call: 4096 base items x 64
MIN_CLASS = 16                    # members a class needs before a one_odd pair may use it
SYNTH = 64                        # rays synthesised for a class the scene's set lacks
WORK_COUNTERS = ("node_tests", "kd_inner_visits", "leaf_refs", "tri_tests", "prim_tests", "smooth_hits")
FILL_DIR = (0.0, 0.0, 1.0)
FILL_POINT = (1.0, 2.0, 3.0)      # a filler segment: a == b


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def chunks(m):
    """whole tiles, at most MAX_ROWS rows a call: the tiles of a chunked call are the tiles of the whole"""
    return [(k, min(k + MAX_ROWS, m)) for k in range(0, m, MAX_ROWS)]


# ---- classes, computed from the rays and the description ----------------------------------------------------------------------------------------
def zero_component(o, d):
    """Z: an exact 0 in any of the six components (node_intersect's `zeros`)"""
    return (o == 0).any(axis=1) | (d == 0).any(axis=1)


def treeless_boxes(desc):
    """(node index, lo - 1e-6, hi + 1e-6) of every tree-less mesh node: box_test_pre's `be` (bbox.h:81-83).  The nodes must be untransformed, as word 0's are."""
    out = []
    for ni in range(desc.n_nodes):
        node = desc.nodes[ni]
        g = desc.geoms[node.geom]
        if g.kind != 3 or desc.meshes[g.index].has_kd:
            continue
        m, off = hl._xf(node.T)
        assert np.array_equal(m, np.eye(3)) and not off.any(), "node %d is transformed: its box is in its own space" % ni
        mesh = desc.meshes[g.index]
        out.append((ni, np.array(mesh.bbox_min[:]) - 1e-6, np.array(mesh.bbox_max[:]) + 1e-6))
    return out


def inside_boxes(desc, o):
    """[n, boxes] bool: BBox::inside of the origin for each tree-less mesh node, and the nodes' indices"""
    boxes = treeless_boxes(desc)
    ins = np.stack([((lo <= o) & (o <= hi)).all(axis=1) for _, lo, hi in boxes], axis=1) if boxes else np.zeros((len(o), 0), bool)
    return ins, np.array([ni for ni, _, _ in boxes], np.int64)


def margin_ratio(desc, a, b):
    """The smallest, over the triangle planes of the small tree-less meshes, of min(|sigma_a|, |sigma_b|) / (n1 S) (dev_segcert.hpp's notation): a segment
    is certified against a plane when this exceeds c = 2^-36 on one side for both ends."""
    best = np.full(len(a), np.inf)
    rng = np.random.default_rng(0)
    ainf, binf = np.abs(a).max(axis=1), np.abs(b).max(axis=1)
    for ni in range(desc.n_nodes):
        node = desc.nodes[ni]
        g = desc.geoms[node.geom]
        if g.kind != 3 or desc.meshes[g.index].has_kd or desc.meshes[g.index].n_triangles > 64:
            continue
        A, B, Cc = hl._mesh_arrays(desc.meshes[g.index], rng, 64)
        for t in range(len(A)):
            N = np.cross(B[t] - A[t], Cc[t] - A[t])
            n1 = np.abs(N).sum()
            if not n1 > 0:
                continue
            S = ainf + binf + np.abs(A[t]).max() + 1.0
            sa, sb = np.abs((a - A[t]) @ N), np.abs((b - A[t]) @ N)
            best = np.minimum(best, np.minimum(sa, sb) / (n1 * S))
    return best


def zeroed_smallest_component(o, d, pick):
    """Z rays made of NZ rays: the direction's smallest component set to an exact 0"""
    o2, d2 = o[pick].copy(), d[pick].copy()
    d2[np.arange(len(pick)), np.abs(d2).argmin(axis=1)] = 0.0
    return o2, d2


def even_stride(n, cap):
    return np.arange(n)[::max(1, -(-n // cap))]


def ray_classes(desc, o, d, ids, word):
    """index sets by class; IN / OUT (and the per-node table they come from) only for word 0, whose tree-less meshes are untransformed"""
    z = zero_component(o, d)
    cls = {"Z": np.flatnonzero(z), "NZ": np.flatnonzero(~z), "HIT": np.flatnonzero(ids != -1), "MISS": np.flatnonzero(ids == -1)}
    ins, box_nodes = None, None
    if word == 0:
        ins, box_nodes = inside_boxes(desc, o)
        cls["IN"], cls["OUT"] = np.flatnonzero(ins.any(axis=1)), np.flatnonzero(~ins.any(axis=1))
    return cls, ins, box_nodes


def segment_classes(desc, a, b, want, with_margin):
    cls = {"visible": np.flatnonzero(want), "occluded": np.flatnonzero(~want)}
    if with_margin:
        r = margin_ratio(desc, a, b)
        cls["NEAR"], cls["FAR"] = np.flatnonzero(r <= 2.0 ** -36), np.flatnonzero(r >= 2.0 ** -30)
    return cls


def build_base_set(oracle, abi, s, name, o, d, cat, ids, rec, a, b):
    """At most CAP rays and CAP segments by an even stride (every category kept, as tests/test_gpu_trace_host.py thins them), plus, where a class the
    one_odd pairs need has fewer than MIN_CLASS members, SYNTH rays made for it and asked of the oracle."""
    word = ADVERSARIAL[name][1]
    ko, ka = even_stride(len(o), CAP - SYNTH), even_stride(len(a), CAP - 2 * SYNTH)
    o, d, cat, ids, rec, a, b = o[ko], d[ko], cat[ko], ids[ko], rec[ko], a[ka], b[ka]
    synthesised = {}
    if word in (0, 8):
        z = zero_component(o, d)
        if z.sum() < MIN_CLASS:
            o2, d2 = zeroed_smallest_component(o, d, np.flatnonzero(~z)[:SYNTH])
            i2, r2 = hl.oracle_probe(oracle, s.desc, o2, d2)
            o, d, cat, ids, rec = np.concatenate([o, o2]), np.concatenate([d, d2]), np.concatenate([cat, ["zero-component"] * len(o2)]), np.concatenate([ids, i2]), np.concatenate([rec, r2])
            synthesised["Z"] = len(o2)
    # segments: a miss's ray cut off anywhere is visible, a node hit's ray cut off beyond the hit is occluded (the oracle is asked all the same)
    want = _oracle_visible(oracle, abi, s.desc, a, b)
    unit = d / np.linalg.norm(d, axis=1)[:, None]
    for cls, lacking, pick, length in (("visible", want.sum() < MIN_CLASS, np.flatnonzero(ids == -1)[:SYNTH], None), ("occluded", (~want).sum() < MIN_CLASS, np.flatnonzero(ids >= 0)[:SYNTH], 1.5)):
        if lacking:
            reach = np.full(len(pick), 5.0) if length is None else rec[pick, 0] * length
            a, b = np.concatenate([a, o[pick]]), np.concatenate([b, o[pick] + unit[pick] * reach[:, None]])
            synthesised[cls] = len(pick)
    o, d, a, b = (np.ascontiguousarray(x) for x in (o, d, a, b))
    assert 1000 <= len(o) <= CAP and 200 <= len(a) <= CAP
    return o, d, cat, ids, rec, a, b, synthesised


# ---- running a composition ----------------------------------------------------------------------------------------------------------------------
def run_closest(s, o, d, src, stats=False):
    go, gd = wc.gather(src, o, d, fill=(np.nan, FILL_DIR))
    ids, rec, dist, tot = [], [], [], {}
    for k0, k1 in chunks(len(src)):
        g = s.trace_rays(go[k0:k1], gd[k0:k1], record=True, stats=stats)
        ids.append(g["hit_id"]); rec.append(g["hit_rec"]); dist.append(g["hit_dist"])
        for key, v in g["stats"].items():
            tot[key] = tot.get(key, 0) + v
    return np.concatenate(ids), np.concatenate(rec), np.concatenate(dist), tot


def run_visible(s, a, b, src, stats=False):
    ga, gb = wc.gather(src, a, b, fill=(FILL_POINT, FILL_POINT))
    vis, tot = [], {}
    for k0, k1 in chunks(len(src)):
        v, st = s.visible(ga[k0:k1], gb[k0:k1], stats=stats)
        vis.append(v)
        for key, val in st.items():
            tot[key] = tot.get(key, 0) + val
    return np.concatenate(vis), tot


def check_closest(case, got, src, pairs, what):
    ids, rec, dist, _ = got
    rows, base = pairs[:, 0], pairs[:, 1]
    bad = np.flatnonzero((ids[rows] != case.ids[base]) | (bits64(rec[rows]) != bits64(case.rec[base])).any(axis=1) | (bits64(dist[rows]) != bits64(case.dist[base])))
    assert len(bad) == 0, (what, "%d of %d rows differ from the natural order's answer" % (len(bad), len(rows)), "rows", rows[bad][:5], "base", base[bad][:5],
                           "categories", sorted(set(case.cat[base[bad]]))[:6])
    fill = src < 0
    assert (ids[fill] == -1).all() and (dist[fill] == 1e99).all() and (rec[fill, 0] == 1e99).all() and (bits64(rec[fill, 1:]) == 0).all(), (what, "filler rows")


def check_visible(case, vis, src, pairs, what):
    rows, base = pairs[:, 0], pairs[:, 1]
    bad = np.flatnonzero(vis[rows] != case.vis[base])
    assert len(bad) == 0, (what, "%d of %d segments differ from the natural order's answer" % (len(bad), len(rows)), "rows", rows[bad][:5], "base", base[bad][:5])
    assert vis[src < 0].all(), (what, "filler rows")


class RayCase:
    pass


@pytest.fixture(scope="module")
def ray_case(fray, abi, oracle, gpu, tmp_path_factory):
    """name -> the scene, its base rays and segments, and the natural order's answers held to the oracle; made once a scene, shared by the tests below"""
    made = {}

    def get(name):
        if name in made:
            return made[name]
        c = RayCase()
        s, path, o, d, cat, ids, rec, a, b = adversarial_case(fray, oracle, name, tmp_path_factory.mktemp("wave_" + name))
        c.name, c.word, c.s = name, ADVERSARIAL[name][1], s
        c.o, c.d, c.cat, c.oracle_ids, c.oracle_rec, c.a, c.b, c.synthesised = build_base_set(oracle, abi, s, name, o, d, cat, ids, rec, a, b)
        c.want_vis = _oracle_visible(oracle, abi, s.desc, c.a, c.b)
        s.beginRender()
        n, m = len(c.o), len(c.a)
        c.ids, c.rec, c.dist, _ = run_closest(s, c.o, c.d, wc.natural(n)[0])
        c.vis, _ = run_visible(s, c.a, c.b, wc.natural(m)[0])
        # the baseline against the reference, by the rules the suite has: ids and rec[:7] equal, u, v equal but for a sphere's within SPHERE_UV_ULPS.  A
        # failure is kept for test_natural_order_equals_the_oracle to raise, so that the other tests still say which compositions differ from it.
        c.sphere_uv, c.baseline_error = -1, None
        try:
            c.sphere_uv = _check_records(s, {"hit_id": c.oracle_ids, "hit_rec": c.oracle_rec}, c.ids, c.rec, name)
            assert np.array_equal(bits64(c.dist), bits64(c.rec[:, 0]))
            assert np.array_equal(c.vis, c.want_vis), (name, "visible", np.argwhere(c.vis != c.want_vis)[:5].ravel())
        except AssertionError as e:
            c.baseline_error = e
        c.classes, c.inside, c.box_nodes = ray_classes(s.desc, c.o, c.d, c.oracle_ids, c.word)
        c.seg_classes = segment_classes(s.desc, c.a, c.b, c.want_vis, name == "cornell_box")
        print("%s (word %d): %d rays, %d segments, %d sphere u, v differ from the oracle's (<= %d x 2^-52); classes %s %s; synthesised %s"
              % (name, c.word, n, m, c.sphere_uv, SPHERE_UV_ULPS, {k: len(v) for k, v in c.classes.items()}, {k: len(v) for k, v in c.seg_classes.items()}, c.synthesised))
        made[name] = c
        return c

    yield get
    for c in made.values():
        c.s.close()


def ray_compositions(c):
    n = len(c.o)
    out = [("alone", wc.alone(n)), ("alone_at17", wc.alone_at(n, 17)), ("alone_at63", wc.alone_at(n, 63)), ("permuted1", wc.permuted(n, 1)), ("permuted2", wc.permuted(n, 2)),
           ("grouped", wc.grouped(c.ids)), ("replicated", wc.replicated(n)), ("dead_interleaved", wc.dead_interleaved(n, 3))]
    return out + [("truncated%d" % m, wc.truncated(n, m)) for m in wc.TRUNCATED_SIZES]


def segment_compositions(c):
    n = len(c.a)
    out = [("alone", wc.alone(n)), ("alone_at17", wc.alone_at(n, 17)), ("alone_at63", wc.alone_at(n, 63)), ("permuted1", wc.permuted(n, 1)), ("permuted2", wc.permuted(n, 2)),
           ("grouped", wc.grouped(c.vis)), ("replicated", wc.replicated(n)), ("dead_interleaved", wc.dead_interleaved(n, 3))]
    return out + [("truncated%d" % m, wc.truncated(n, m)) for m in wc.TRUNCATED_SIZES]


# ---- a: closest hit and visibility ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,word", SCENES_BY_WORD, ids=[n for n, _ in SCENES_BY_WORD])
def test_natural_order_equals_the_oracle(ray_case, name, word):
    c = ray_case(name)
    assert c.word == word
    if c.baseline_error is not None:
        raise c.baseline_error
    for k in ("Z", "NZ", "HIT", "MISS", "IN", "OUT"):
        assert k not in c.classes or len(c.classes[k]) >= MIN_CLASS, (name, k, len(c.classes[k]))
    for k, v in c.seg_classes.items():
        assert len(v) >= MIN_CLASS, (name, k, len(v))


@pytest.mark.parametrize("name,word", SCENES_BY_WORD, ids=[n for n, _ in SCENES_BY_WORD])
def test_closest_hit_and_visibility_in_every_composition(ray_case, name, word):
    c = ray_case(name)
    assert c.word == word
    t0 = time.perf_counter()
    rows = 0
    for what, (src, pairs) in ray_compositions(c):
        check_closest(c, run_closest(c.s, c.o, c.d, src), src, pairs, "%s rays %s" % (name, what))
        rows += len(src)
    for what, (src, pairs) in segment_compositions(c):
        check_visible(c, run_visible(c.s, c.a, c.b, src)[0], src, pairs, "%s segments %s" % (name, what))
        rows += len(src)
    print("%s: %d rows in %.2f s" % (name, rows, time.perf_counter() - t0))


@pytest.mark.parametrize("name,word", SCENES_BY_WORD, ids=[n for n, _ in SCENES_BY_WORD])
def test_counting_kernels_in_natural_permuted_and_replicated_order(ray_case, name, word):
    """The odd flag words: the same records, closest_rays / shadow_rays = the live rows, and every work counter -- a sum over rays of what each ray's own
    traversal counts -- the natural order's (64 times it when every ray runs 64 times)."""
    c = ray_case(name)
    n, m = len(c.o), len(c.a)
    t0 = time.perf_counter()
    base_st, base_vst = None, None
    for what, (src, pairs), times in (("natural", wc.natural(n), 1), ("permuted1", wc.permuted(n, 1), 1), ("replicated", wc.replicated(n), 64)):
        got = run_closest(c.s, c.o, c.d, src, stats=True)
        check_closest(c, got, src, pairs, "%s rays %s stats" % (name, what))
        st = got[3]
        assert st["closest_rays"] == int((src >= 0).sum()), (name, what)
        base_st = base_st or st
        for k in WORK_COUNTERS:
            assert st[k] == times * base_st[k], (name, what, k, st[k], times, base_st[k])
    for what, (src, pairs), times in (("natural", wc.natural(m), 1), ("permuted1", wc.permuted(m, 1), 1), ("replicated", wc.replicated(m), 64)):
        vis, vst = run_visible(c.s, c.a, c.b, src, stats=True)
        check_visible(c, vis, src, pairs, "%s segments %s stats" % (name, what))
        assert vst["shadow_rays"] == int((src >= 0).sum()), (name, what)
        base_vst = base_vst or vst
        for k in WORK_COUNTERS:
            assert vst[k] == times * base_vst[k], (name, what, k, vst[k], times, base_vst[k])
    print("%s: closest %s; visible %s; %.2f s" % (name, {k: base_st[k] for k in WORK_COUNTERS}, {k: base_vst[k] for k in WORK_COUNTERS}, time.perf_counter() - t0))


RAY_PAIRS = [("cornell_box", "NZ", "Z"), ("textured_plain", "NZ", "Z"), ("cornell_box", "IN", "OUT")] + [(n, "HIT", "MISS") for n, _ in SCENES_BY_WORD]
SEGMENT_PAIRS = [(n, "occluded", "visible") for n, _ in SCENES_BY_WORD] + [("cornell_box", "NEAR", "FAR")]


@pytest.mark.parametrize("name,P,Q", RAY_PAIRS, ids=["%s-%s-%s" % p for p in RAY_PAIRS])
def test_one_odd_ray_in_a_wave_of_the_other_class(ray_case, name, P, Q):
    c = ray_case(name)
    p, q = c.classes[P], c.classes[Q]
    assert len(p) >= MIN_CLASS and len(q) >= MIN_CLASS, (name, P, len(p), Q, len(q))
    t0 = time.perf_counter()
    n = len(c.o)
    runs = [("%s / %s" % (P, Q), wc.one_odd(n, p, q, 5))]
    if (P, Q) == ("IN", "OUT"):
        # box_test_pre's first exit is per node: a wave whose lanes all start inside node j's box but one, which starts outside every box and whose
        # closest hit is node j (the lane that needs the box test's answer), and the mirror
        for j, ni in enumerate(c.box_nodes):
            pj, qj = np.flatnonzero(c.inside[:, j]), np.intersect1d(q, np.flatnonzero(c.oracle_ids == ni))
            if len(pj) and len(qj):
                runs.append(("inside node %d / outside, hitting it" % ni, wc.one_odd(n, pj, qj, 6 + j, tiles=min(256, max(len(pj), len(qj))))))
        assert len(runs) >= 3, "fewer than two nodes have both rays starting in their box and rays hitting them from outside"
    for what, (src, pairs) in runs:
        check_closest(c, run_closest(c.s, c.o, c.d, src), src, pairs, "%s one_odd %s" % (name, what))
    print("%s one_odd %s %d / %s %d: %d runs, %.2f s" % (name, P, len(p), Q, len(q), len(runs), time.perf_counter() - t0))


@pytest.mark.parametrize("name,P,Q", SEGMENT_PAIRS, ids=["%s-%s-%s" % p for p in SEGMENT_PAIRS])
def test_one_odd_segment_in_a_wave_of_the_other_class(ray_case, name, P, Q):
    c = ray_case(name)
    p, q = c.seg_classes[P], c.seg_classes[Q]
    assert len(p) >= MIN_CLASS and len(q) >= MIN_CLASS, (name, P, len(p), Q, len(q))
    t0 = time.perf_counter()
    src, pairs = wc.one_odd(len(c.a), p, q, 5)
    check_visible(c, run_visible(c.s, c.a, c.b, src)[0], src, pairs, "%s one_odd %s / %s" % (name, P, Q))
    print("%s one_odd %s %d / %s %d: %.2f s" % (name, P, len(p), Q, len(q), time.perf_counter() - t0))


# ---- b: path-traced radiance ------------------------------------------------------------------------------------------------------------------------
COPLANAR, ELIGIBLE = "coplanar quads, the light in their plane", "a one-triangle and a five-triangle mesh"
PT_SCENES = ["cornell_box", COPLANAR, ELIGIBLE]
PT_IDS = [v.replace(" ", "_").replace(",", "") for v in PT_SCENES]
SPP = 2


class PathCase:
    pass


def run_shade(s, o, d, keys, src, k, spp=1, rng_skip=2, stats=False):
    go, gd, gk = wc.gather(src, o, d, keys, fill=(np.nan, FILL_DIR, 0))
    rgb, tot = [], {}
    for k0, k1 in chunks(len(src)):
        r = s.shade_rays(go[k0:k1], gd[k0:k1], spp=spp, seed=42, sample_first=k, rng_skip=rng_skip, keys=gk[k0:k1], stats=stats)
        if stats:
            r, st = r
            for key, v in st.items():
                tot[key] = tot.get(key, 0) + v
        rgb.append(r)
    return np.concatenate(rgb), tot


def check_shade(base, rgb, src, pairs, what):
    rows, bi = pairs[:, 0], pairs[:, 1]
    bad = np.flatnonzero((bits32(rgb[rows]) != bits32(base[bi])).any(axis=1))
    assert len(bad) == 0, (what, "%d of %d rows differ from the natural order's colour" % (len(bad), len(rows)), "rows", rows[bad][:5], "base", bi[bad][:5])
    assert (rgb[src < 0] == 0).all(), (what, "filler rows are not black")


@pytest.fixture(scope="module")
def path_case(fray, abi, oracle, gpu, tmp_path_factory):
    """name -> a path-traced scene, the jittered camera rays of each of its SPP samples, and each sample's colours in natural order, whose mean is held
    to the frame and to the oracle's frame by bits"""
    made = {}

    def get(name):
        if name in made:
            return made[name]
        c = PathCase()
        if name == "cornell_box":
            s = open_scene(fray, "cornell_box.fray", 64, 48, gi=1, numPaths=SPP, wantAA=0)
        else:
            s = fray.Scene.parseScene(ROOMS[name][0](tmp_path_factory.mktemp("wave_room")))            # 48 x 48, gi on, wantAA off
            s.settings.numPaths = SPP
        assert s.settings.gi and not s.settings.wantAA and not s.camera.dof
        s.beginRender()
        c.name, c.s = name, s
        c.eligible = s.get_option("certified_segments_eligible")
        W, H = s.frame_size
        c.n = W * H
        c.keys = np.arange(c.n, dtype=np.uint32)
        xs, ys = pixel_grid(W, H)
        c.o, c.d, c.base, c.first = [], [], [], []
        for k in range(SPP):
            j = jitter(fray, sample_seed(42, c.keys, k)).reshape(H, W, 2)
            xy = np.stack([(xs + j[..., 0]).astype(np.float64), (ys + j[..., 1]).astype(np.float64)], axis=-1)
            o, d = s.camera_rays(xy)
            o, d = np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))
            c.o.append(o); c.d.append(d)
            c.base.append(run_shade(s, o, d, c.keys, wc.natural(c.n)[0], k)[0])
            c.first.append(s.trace_rays(o, d)["hit_id"])
        c.frame, _ = s.render(seed=42)
        c.baseline_error = None
        try:
            acc = np.zeros((c.n, 3), np.float32)
            for k in range(SPP):
                acc = acc + c.base[k]
            mean = (acc / np.float32(SPP)).reshape(H, W, 3)
            ref, _ = oracle.render(s.desc, abi.MODE_RENDER, seed=42)
            img, _ = pt_by_samples(fray, s, SPP)
            assert np.array_equal(bits32(img), bits32(c.frame)), (name, "pt_by_samples differs from the frame")
            assert np.array_equal(bits32(mean), bits32(c.frame)), (name, "the mean of the samples with explicit keys differs from the frame")
            assert np.array_equal(bits32(c.frame), bits32(ref)), (name, "the frame differs from the oracle's", int((bits32(c.frame) != bits32(ref)).any(axis=2).sum()))
        except AssertionError as e:
            c.baseline_error = e
        made[name] = c
        return c

    yield get
    for c in made.values():
        c.s.close()


def wall_and_block_classes(first):
    """P: first hit on a wall (nodes 0-4 of cornell_box.fray and of the generated rooms: floor, ceiling, back, right, left); Q: on a block, an added mesh or the light"""
    wall = (first >= 0) & (first < 5)
    return np.flatnonzero(wall), np.flatnonzero((first >= 5) | (first <= -2))


def path_compositions(c, k):
    n = c.n
    P, Q = wall_and_block_classes(c.first[k])
    assert len(P) >= MIN_CLASS and len(Q) >= MIN_CLASS, (c.name, len(P), len(Q))
    return [("permuted1", wc.permuted(n, 1)), ("permuted2", wc.permuted(n, 2)), ("grouped", wc.grouped(c.first[k])), ("replicated", wc.replicated(n)), ("alone", wc.alone(n)),
            ("alone_at63", wc.alone_at(n, 63)), ("dead_interleaved", wc.dead_interleaved(n, 3)), ("one_odd wall / block or light", wc.one_odd(n, P, Q, 5))]


@pytest.mark.parametrize("name", PT_SCENES, ids=PT_IDS)
def test_path_traced_natural_order_is_the_frame_and_the_oracle(path_case, name):
    c = path_case(name)
    assert c.eligible == (0 if name == COPLANAR else 1)
    if c.baseline_error is not None:
        raise c.baseline_error


@pytest.mark.parametrize("name", PT_SCENES, ids=PT_IDS)
def test_path_traced_radiance_in_every_composition(path_case, name):
    c = path_case(name)
    t0 = time.perf_counter()
    rows = 0
    for k in range(SPP):
        for what, (src, pairs) in path_compositions(c, k):
            rgb, _ = run_shade(c.s, c.o[k], c.d[k], c.keys, src, k)
            check_shade(c.base[k], rgb, src, pairs, "%s sample %d %s" % (name, k, what))
            rows += len(src)
    print("%s: %d paths in %.2f s" % (name, rows, time.perf_counter() - t0))


@pytest.mark.parametrize("name", PT_SCENES, ids=PT_IDS)
def test_path_traced_options_counters_and_two_samples_in_one_call(path_case, name):
    c = path_case(name)
    s, n = c.s, c.n
    t0 = time.perf_counter()
    orders = [("permuted1", wc.permuted(n, 1)), ("dead_interleaved", wc.dead_interleaved(n, 3))]
    # the shortcuts off: what each proves is that it changes nothing
    for option in ("segment_planes", "certified_segments"):
        assert s.get_option(option) == 1
        s.set_option(option, 0)
        try:
            for k in range(SPP):
                for what, (src, pairs) in orders:
                    check_shade(c.base[k], run_shade(s, c.o[k], c.d[k], c.keys, src, k)[0], src, pairs, "%s sample %d %s, %s 0" % (name, k, what, option))
        finally:
            s.set_option(option, 1)
    # the counting kernels: the same colours; samples = the live rows; the work counters, sums over paths, the natural order's
    for k in range(SPP):
        nat, base_st = run_shade(s, c.o[k], c.d[k], c.keys, wc.natural(n)[0], k, stats=True)
        assert np.array_equal(bits32(nat), bits32(c.base[k])), (name, k, "the counting kernels' colours")
        assert base_st["samples"] == n
        for what, (src, pairs) in orders:
            rgb, st = run_shade(s, c.o[k], c.d[k], c.keys, src, k, stats=True)
            check_shade(c.base[k], rgb, src, pairs, "%s sample %d %s stats" % (name, k, what))
            assert st["samples"] == int((src >= 0).sum()), (name, what, st["samples"])
            keys5 = ("closest_rays", "shadow_rays", "node_tests", "tri_tests", "prim_tests")
            if what == "permuted1":
                for key in keys5:
                    assert st[key] == base_st[key], (name, k, what, key, st[key], base_st[key])
            else:
                # dead_interleaved runs every path once or twice: the natural order's counters plus those of the paths that run twice, which a run
                # of those alone (every other row filler) gives
                src2 = np.where(np.bincount(src[src >= 0], minlength=n) == 2, np.arange(n), wc.FILL)
                _, st2 = run_shade(s, c.o[k], c.d[k], c.keys, src2, k, stats=True)
                for key in keys5:
                    assert st[key] == base_st[key] + st2[key], (name, k, what, key, st[key], base_st[key], st2[key])
    # two samples in one call, not two calls of one
    src, pairs = wc.permuted(n, 2)
    go, gd, gk = wc.gather(src, c.o[0], c.d[0], c.keys, fill=(np.nan, FILL_DIR, 0))
    two = s.shade_rays(go, gd, spp=2, seed=42, sample_first=0, rng_skip=2, keys=gk)
    one = [s.shade_rays(c.o[0], c.d[0], spp=1, seed=42, sample_first=k, rng_skip=2, keys=c.keys) for k in range(2)]          # (sample 1 along sample 0's rays)
    want = (np.zeros((n, 3), np.float32) + one[0] + one[1]) / np.float32(2)
    assert np.array_equal(bits32(one[0]), bits32(c.base[0]))
    check_shade(want, two, src, pairs, "%s spp 2 in one call, permuted" % name)
    print("%s: %.2f s" % (name, time.perf_counter() - t0))


# ---- c: Whitted radiance -----------------------------------------------------------------------------------------------------------------------------
WHITTED = [("boxed", 4), ("csg_nested", 2)]


@pytest.mark.parametrize("name,word", WHITTED, ids=[n for n, _ in WHITTED])
def test_whitted_radiance_in_permuted_replicated_and_dead_interleaved_order(fray, gpu, tmp_path, name, word):
    """k_whitted_rays schedules its lanes by ballots of its own (shade_variant.hip)"""
    s = fray.Scene.parseScene(ADVERSARIAL[name][0](tmp_path))
    s.settings.frameWidth, s.settings.frameHeight, s.settings.wantAA, s.settings.gi = 64, 48, 0, 0
    s.camera.dof = 0
    s.beginRender()
    t0 = time.perf_counter()
    frame, _ = s.render(seed=42)
    o, d = s.camera_rays()
    o, d = np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))
    n = len(o)
    keys = np.arange(n, dtype=np.uint32)
    base, _ = run_shade(s, o, d, keys, wc.natural(n)[0], 0, rng_skip=0)
    assert np.array_equal(bits32(base), bits32(frame.reshape(-1, 3))), (name, "the natural order differs from the frame")
    assert np.array_equal(bits32(whitted_single_sample(s)), bits32(frame))
    for what, (src, pairs) in (("permuted1", wc.permuted(n, 1)), ("permuted2", wc.permuted(n, 2)), ("replicated", wc.replicated(n)), ("dead_interleaved", wc.dead_interleaved(n, 3))):
        rgb, _ = run_shade(s, o, d, keys, src, 0, rng_skip=0)
        check_shade(base, rgb, src, pairs, "%s Whitted %s" % (name, what))
    rgb, st = run_shade(s, o, d, keys, wc.dead_interleaved(n, 3)[0], 0, rng_skip=0, stats=True)
    assert st["samples"] == int((wc.dead_interleaved(n, 3)[0] >= 0).sum())
    print("%s Whitted: %.2f s" % (name, time.perf_counter() - t0))
    s.close()
