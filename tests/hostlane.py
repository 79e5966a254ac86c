"""The host lane (tests/native/hostlane): builds arena_dump and trace_host, writes ray files, reads result files, and makes the adversarial rays and
segments that tests/test_trace_host.py (CPU) and tests/test_gpu_trace_host.py (GPU) feed it.  Not a test module."""
import math
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HL = os.path.join(ROOT, "tests", "native", "hostlane")
CSRC = os.path.join(ROOT, "fray_amd", "csrc")
INC = ["-I" + HL, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
# ROCm's own clang: g++ cannot compile the device headers, and this clang ships the x86-64 sanitizer runtimes
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")

WARN = ["-Wall", "-Wuninitialized", "-Wsometimes-uninitialized", "-Wconditional-uninitialized", "-Werror"]
# Every build of trace_host is compiled without contraction, as the library is.  The builds whose outputs are compared take different poison bytes for
# the locals the harness hands to the code under test (trace_host.cpp): a result made of such a byte differs between them.
BUILDS = {
    "asan": ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-DHOSTLANE_POISON_BYTE=0xA5"],
    "msan": ["-O1", "-g", "-fsanitize=memory", "-fsanitize-memory-track-origins"],
    "pattern": ["-O2", "-ftrivial-auto-var-init=pattern", "-DHOSTLANE_POISON_BYTE=0xAA"],
    "zero": ["-O2", "-ftrivial-auto-var-init=zero", "-DHOSTLANE_POISON_BYTE=0x00"],
    "plain": ["-O1", "-DHOSTLANE_POISON_BYTE=0x5A"],
}
# (leak checking off: it needs ptrace, which a sandboxed test run may not have; the harness frees what it allocates all the same)
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "MSAN_OPTIONS": "abort_on_error=0"}


def trace_host_command(build, exe):
    return [CLANG, "-std=c++17", "-ffp-contract=off"] + BUILDS[build] + INC + [os.path.join(HL, "trace_host.cpp"), "-o", exe]


def warnings_command(obj):
    """build (e): the translation unit with the uninitialised-variable warnings as errors"""
    return [CLANG, "-std=c++17", "-ffp-contract=off", "-O1"] + WARN + INC + ["-c", os.path.join(HL, "trace_host.cpp"), "-o", obj]


def arena_dump_command(exe, sanitize=True):
    src = [os.path.join(HL, "arena_dump.cpp")] + [os.path.join(CSRC, f) for f in ("host_scene.cpp", "host_loaders.cpp", "host_exr.cpp")]
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    return ["g++", "-std=c++17", "-O1", "-ffp-contract=off"] + san + INC[1:] + ["-I" + HL] + src + ["-o", exe]


def build_parallel(commands):
    """Runs the compile commands side by side (CPU tests); raises with the compiler's output on a failure."""
    procs = [subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for c in commands]
    for c, p in zip(commands, procs):
        out, _ = p.communicate()
        assert p.returncode == 0, " ".join(c) + "\n" + out[-6000:]


# ---- files (tests/native/hostlane/hostlane_format.h) ---------------------------------------------------------------------------------------
def write_rays(path, o, d, a, b):
    o, d, a, b = (np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1, 3)) for x in (o, d, a, b))
    assert len(o) == len(d) and len(a) == len(b)
    with open(path, "wb") as f:
        f.write(b"FRAYRAY1" + struct.pack("<QQ", len(o), len(a)))
        for x in (o, d, a, b):
            f.write(x.tobytes())


COUNTER_NAMES = ("closest_rays", "shadow_rays", "node_tests", "kd_inner_visits", "leaf_refs", "tri_tests", "prim_tests", "smooth_hits", "samples",
                 "texture_fetches", "envelope")


def read_result(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"FRAYRES1", raw[:8]
    word, n, m, segp = struct.unpack_from("<QQQQ", raw, 8)
    pos = [40]

    def take(dtype, count):
        x = np.frombuffer(raw, dtype, count, pos[0])
        pos[0] += x.nbytes
        return x

    r = {"word": word, "segp": bool(segp), "raw": raw}
    r["hit_id"], r["hit_rec"] = take(np.int32, n), take(np.float64, 9 * n).reshape(n, 9)
    r["hit_id_c"], r["hit_rec_c"] = take(np.int32, n), take(np.float64, 9 * n).reshape(n, 9)
    r["cnt_closest"] = dict(zip(COUNTER_NAMES, (int(v) for v in take(np.uint64, 11))))
    r["vis"], r["vis_c"] = take(np.uint8, m).astype(bool), take(np.uint8, m).astype(bool)
    r["cnt_visible"] = dict(zip(COUNTER_NAMES, (int(v) for v in take(np.uint64, 11))))
    r["vis_p"], r["skip"] = take(np.uint8, m).astype(bool), take(np.uint32, m)
    assert pos[0] == len(raw)
    return r


# ---- the oracle's answers ------------------------------------------------------------------------------------------------------------------
def oracle_probe(oracle, desc, o, d):
    """ids and 9-double records of fray_oracle_probe for each ray"""
    o, d = np.ascontiguousarray(o, np.float64), np.ascontiguousarray(d, np.float64)
    ids, rec, out = np.zeros(len(o), np.int32), np.zeros((len(o), 9)), np.zeros(9)
    for i in range(len(o)):
        ids[i] = oracle.lib.fray_oracle_probe(desc, o[i].ctypes.data, d[i].ctypes.data, out.ctypes.data)
        rec[i] = out
    return ids, rec


def camera_rays(oracle, desc, W, H, step=1):
    o, d = np.zeros((H // step, W // step, 3)), np.zeros((H // step, W // step, 3))
    so, sd = np.zeros(3), np.zeros(3)
    for y in range(H // step):
        for x in range(W // step):
            oracle.lib.fray_oracle_camera_ray(desc, float(x * step), float(y * step), so.ctypes.data, sd.ctypes.data)
            o[y, x], d[y, x] = so, sd
    return o.reshape(-1, 3), d.reshape(-1, 3)


def passes_query_filter(o, d):
    """query_variant.hip: finite origin, 0 < |d|^2 <= DBL_MAX"""
    with np.errstate(over="ignore", invalid="ignore"):
        dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return np.isfinite(o).all(axis=1) & (dd > 0) & np.isfinite(dd)


# ---- adversarial rays ----------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _xf(T):
    return np.array(T.m[:]).reshape(3, 3), np.array(T.offset[:])


def _to_world(T, p, is_dir=False):
    """Transform::transformPoint / transformDir: row vector times m (+ offset)"""
    m, off = _xf(T)
    return p @ m if is_dir else p @ m + off


def _leaves(desc, g, depth=0):
    """(kind, index) of the plain geometries under geometry g"""
    ref = desc.geoms[g]
    if ref.kind != 4:
        return [(ref.kind, ref.index)]
    if depth > 20:
        return []
    c = desc.csgs[ref.index]
    return _leaves(desc, c.left, depth + 1) + _leaves(desc, c.right, depth + 1)


def _mesh_arrays(m, rng, cap):
    """up to `cap` triangles of a mesh as (A, B, C) arrays"""
    nt = m.n_triangles
    if nt == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))
    V = np.ctypeslib.as_array(m.vertices, shape=(m.n_vertices * 3,)).reshape(-1, 3)
    pick = np.arange(nt) if nt <= cap else rng.choice(nt, cap, replace=False)
    idx = np.array([m.triangles[int(t)].v[:] for t in pick])
    return V[idx[:, 0]], V[idx[:, 1]], V[idx[:, 2]]


def adversarial_rays(oracle, desc, seed, per=300):
    """The rays of the issue's list for one scene, a few thousand: (origins, directions, the category of each ray)."""
    rng = np.random.default_rng(seed)
    W, H = desc.settings.frameWidth, desc.settings.frameHeight
    co, cd = camera_rays(oracle, desc, W, H, step=max(1, int(math.sqrt(W * H / 600.0))))
    cid, crec = oracle_probe(oracle, desc, co, cd)
    hit = cid >= 0
    assert hit.sum() >= 20, "the camera sees too little of the scene to seed the rays"
    P, Nn, Din = crec[hit, 1:4], crec[hit, 4:7], cd[hit]
    eye = co[0]
    scale = float(np.median(crec[hit, 0]))
    O, D, cat = [], [], []

    def add(name, o, d):
        o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
        O.append(o); D.append(d); cat.extend([name] * len(o))

    k = rng.integers(0, len(P), per)
    # origins on earlier hit points: into the half space of the normal, into the surface, straight on, straight back, along the surface
    u = _unit(rng, per)
    add("self-hit", P[k], u)
    add("self-hit", P[k[:per // 2]], Din[k[:per // 2]])
    add("self-hit", P[k[:per // 2]], -Din[k[:per // 2]])
    add("self-hit", P[k[:per // 2]], np.cross(Nn[k[:per // 2]], u[:per // 2]))
    # directions with exact zero components and with components of 1e-300: from the eye and from hit points
    for tiny in (0.0, 1e-300, -1e-300):
        src = np.where(rng.random(per // 2)[:, None] < 0.5, eye[None, :] + rng.normal(size=(per // 2, 3)) * 0.01 * scale, P[k[:per // 2]])
        d = P[rng.integers(0, len(P), per // 2)] - src
        d[d == 0] = 1.0
        ax = rng.integers(0, 3, per // 2)
        d[np.arange(per // 2), ax] = tiny
        two = rng.random(per // 2) < 0.3
        d[two, (ax[two] + 1) % 3] = tiny
        add("zero-component", src, d)
    # origins a million units out: aimed at hit points, and aimed anywhere
    far = _unit(rng, per)
    add("far-origin", P[k] + far * 1e6, -far)
    add("far-origin", P[k[:per // 3]] + far[:per // 3] * 1e6, _unit(rng, per // 3))
    # away from everything: from above the scene upwards and outwards (the misses of a closed room)
    up = _unit(rng, per)
    up[:, 1] = np.abs(up[:, 1]) + 0.2
    add("leaving", P[k] + np.array([0, 1, 0]) * (np.abs(P[:, 1]).max() + 10 * scale) + rng.normal(size=(per, 3)) * scale, up)

    for ni in range(desc.n_nodes):
        node = desc.nodes[ni]
        T = node.T
        for kind, index in _leaves(desc, node.geom):
            if kind == 3:
                m = desc.meshes[index]
                lo, hi = np.array(m.bbox_min[:]), np.array(m.bbox_max[:])
                ext = np.maximum(hi - lo, 1e-9)
                # rays lying in the faces of the bounding box, and in KD split planes: the coordinate of the plane exactly, no component along its axis
                planes = [(ax, v) for ax in range(3) for v in (lo[ax], hi[ax])]
                inner = [j for j in range(m.n_kdnodes) if m.kdnodes[j].axis < 3]
                for j in (inner[:3] + [inner[int(q)] for q in rng.integers(0, len(inner), 9)] if inner else []):
                    planes.append((m.kdnodes[j].axis, m.kdnodes[j].split))
                n_each = max(4, per // (2 * len(planes)))
                for ax, v in planes:
                    a = lo + rng.random((n_each, 3)) * ext
                    b = lo + rng.random((n_each, 3)) * ext
                    a[:, ax] = v
                    b[:, ax] = v
                    d = b - a
                    d[:, ax] = 0.0
                    o = a - d * rng.uniform(0.0, 2.0, (n_each, 1))
                    o[:, ax] = v
                    add("box-face-or-split-plane", _to_world(T, o), _to_world(T, d, True))
                # through vertices, through points of edges, and along edges
                A, B, Cc = _mesh_arrays(m, rng, max(8, per // 4))
                if len(A):
                    src = _to_world(T, A) + _unit(rng, len(A)) * ext.max() * rng.uniform(0.5, 3.0, (len(A), 1))
                    add("vertex", src, _to_world(T, A) - src)
                    t = rng.random((len(A), 1))
                    e = _to_world(T, A + (B - A) * t)
                    add("edge", src, e - src)
                    add("edge", _to_world(T, A - (B - A) * rng.uniform(0.0, 1.5, (len(A), 1))), _to_world(T, B - A, True))
                    add("edge", _to_world(T, Cc + (Cc - B) * 0.5), _to_world(T, B - Cc, True))
            elif kind in (1, 2):
                # grazing the silhouette: rays whose distance from the centre (sphere) or whose offset from a face plane (cube) is the radius / half side
                # times 1 +- eps
                if kind == 1:
                    ctr, R = np.array(desc.spheres[index].O[:]), abs(desc.spheres[index].R)
                else:
                    ctr, R = np.array(desc.cubes[index].O[:]), abs(desc.cubes[index].halfSide)
                n_g = per // 2 if desc.geoms[node.geom].kind != 4 else max(10, per // 6)          # (a CSG tree has many leaves)
                eps = rng.choice([0.0, 1e-16, -1e-16, 1e-13, -1e-13, 1e-9, -1e-9, 1e-5, -1e-5, 1e-2, -1e-2], n_g)
                if kind == 1:
                    p = _unit(rng, n_g)
                    q = np.cross(p, _unit(rng, n_g))
                    q /= np.linalg.norm(q, axis=1)[:, None]
                else:
                    ax = rng.integers(0, 3, n_g)
                    p = np.zeros((n_g, 3))
                    p[np.arange(n_g), ax] = rng.choice([-1.0, 1.0], n_g)
                    q = _unit(rng, n_g)
                    q[np.arange(n_g), ax] = 0.0                       # in the face's plane ...
                    along = rng.random(n_g) < 0.5
                    q[along, (ax[along] + 1) % 3] = 0.0               # ... half of them along an edge direction
                touch = ctr + p * (R * (1.0 + eps))[:, None]
                if kind == 2:
                    touch = touch + rng.uniform(-1.2, 1.2, (n_g, 3)) * R * (p == 0)          # anywhere on the face's plane, also beside the face
                o = touch - q * (R * rng.uniform(1.5, 4.0, (n_g, 1)))
                add("silhouette", _to_world(T, o), _to_world(T, q, True))
                if desc.geoms[node.geom].kind == 4:
                    # from inside a CSG operand: the centre, points inside, points on its surface
                    n_i = max(10, per // 5)
                    inside = ctr + _unit(rng, n_i) * R * rng.choice([0.0, 0.3, 0.9, 1.0], (n_i, 1))
                    add("inside-csg-operand", _to_world(T, inside), _to_world(T, _unit(rng, n_i), True))
    O, D, cat = np.concatenate(O), np.concatenate(D), np.array(cat)
    ok = passes_query_filter(O, D)
    return np.ascontiguousarray(O[ok]), np.ascontiguousarray(D[ok]), cat[ok]


# ---- adversarial segments ------------------------------------------------------------------------------------------------------------------
def wall_segments(desc, seed, per=40):
    """For every triangle plane of every small tree-less untransformed mesh (the nodes the segment-plane shortcut may skip) and of the larger tree-less
    ones (the blocks): segments whose ends lie from far outside down to inside the certificate's margin on both sides of the plane, segments nearly
    parallel to it, and segments ending on and just beyond it."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for ni in range(desc.n_nodes):
        node = desc.nodes[ni]
        g = desc.geoms[node.geom]
        if g.kind != 3 or desc.meshes[g.index].has_kd or desc.meshes[g.index].n_triangles > 64:
            continue
        m = desc.meshes[g.index]
        A, B, Cc = _mesh_arrays(m, rng, 64)
        A, B, Cc = _to_world(node.T, A), _to_world(node.T, B), _to_world(node.T, Cc)
        lo, hi = np.minimum(np.minimum(A, B), Cc).min(axis=0), np.maximum(np.maximum(A, B), Cc).max(axis=0)
        size = float(np.max(hi - lo)) or 1.0
        for t in range(len(A)):
            n = np.cross(B[t] - A[t], Cc[t] - A[t])
            ln = np.linalg.norm(n)
            if not ln > 0:
                continue
            n = n / ln
            w = rng.dirichlet([1, 1, 1], per)
            inside = w[:, :1] * A[t] + w[:, 1:2] * B[t] + w[:, 2:] * Cc[t]
            beside = inside + (inside - A[t]) * rng.uniform(1.0, 2.0, (per, 1))          # in the plane, mostly off the triangle
            # the offsets of the two ends from the plane: from far outside to inside the margin (2^-36 |N|_1 (|a| + |b| + ...), dev_segcert.hpp), both signs
            offs = size * rng.choice([1.0, 1e-2, 1e-5, 1e-8, 1e-10, 1e-12, 1e-14, 0.0], (per, 2)) * rng.choice([-1.0, 1.0], (per, 2))
            p0 = np.where(rng.random((per, 1)) < 0.5, inside, beside) + n * offs[:, :1] + rng.normal(size=(per, 3)) * size * 0.2 * (1 - np.abs(n))
            p1 = np.where(rng.random((per, 1)) < 0.5, inside, beside) + n * offs[:, 1:]
            a.append(p0); b.append(p1)
            # nearly parallel to the plane: a chord of the plane lifted by a tiny angle
            tilt = size * rng.choice([0.0, 1e-15, 1e-12, 1e-9, 1e-6, 1e-3], (per // 2, 1)) * rng.choice([-1.0, 1.0], (per // 2, 1))
            lift = size * rng.choice([0.0, 1e-12, 1e-6, 1e-2], (per // 2, 1)) * rng.choice([-1.0, 1.0], (per // 2, 1))
            a.append(beside[:per // 2] + n * lift); b.append(inside[:per // 2] + n * (lift + tilt))
            # ending on the face and just beyond it, from a point off the plane
            src = inside[:per // 2] + n * size * rng.uniform(0.05, 1.0, (per // 2, 1)) * rng.choice([-1.0, 1.0], (per // 2, 1)) + rng.normal(size=(per // 2, 3)) * size * 0.1
            beyond = rng.choice([0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, 1e-3], (per // 2, 1))
            a.append(src); b.append(inside[per // 2:per // 2 * 2] + (inside[per // 2:per // 2 * 2] - src) * beyond)
    if not a:
        return np.zeros((0, 3)), np.zeros((0, 3))
    return np.ascontiguousarray(np.concatenate(a)), np.ascontiguousarray(np.concatenate(b))
