"""The chain of a specular feature frame (include/frayhip.h "specular feature frames") restated in numpy, fed by callables.  Not a test module.

walk_chain follows the rays of ONE camera sample through Refl / Refr nodes; what it asks of the scene is a callable trace(o, d) -> (hit_id,
rec[n, 9]) -- the ray queries (query_trace: Scene.trace_rays(record=True), on the GPU) or the CPU oracle (oracle_trace: hostlane.oracle_probe, no
GPU).  The traversal behind both is pinned to the reference bit for bit elsewhere; what this file is independent in is the chain logic: the step
rule, T, the product A, the unfolding matrix M, the terminal's row and the sample reduction, restated from the header.
K = 0 is the first-hit rule: frayhip_render_features' row.
Film positions of sample i (aa_positions, jittered_positions): the integer pixels plus the AA offset (Whitted with wantAA) or plus the first two floats of the
generator seeded with sample_seed(seed, p, i) (gi frames), both added in float32 and widened, as the kernels do.  The thin-lens rays of a DOF frame
are NOT restated here: no walk in this file stands for a DOF sample.
A bump map is not restated either: walk_chain refuses a scene with one."""
import numpy as np

from test_gpu_shade import AA_OFFSETS, pixel_grid

F32 = np.float32


# ---- dev_math.hpp's operation order: dot = (x + y) + z, V3 * double componentwise, no contraction (numpy's ufuncs round every operation) ----
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _faceforward(d, n):
    return np.where((_dot(d, n) < 0)[:, None], n, -n)


def _reflect(i, n):
    return i + (2 * _dot(-i, n))[:, None] * n


def _normalized(a):
    m = 1.0 / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    return a * m[:, None]


def _refract(i, n, ior):
    """(direction, total internal reflection): refract() returns the zero vector there"""
    ndi = _dot(i, n)
    k = 1 - (ior * ior) * (1 - ndi * ndi)
    tir = k < 0.0
    with np.errstate(invalid="ignore"):
        out = _normalized(ior[:, None] * i - (ior * ndi + np.sqrt(k))[:, None] * n)
    return np.where(tir[:, None], 0.0, out), tir


def _checker(tex, u, v):
    """CheckerTexture::sample (shading.cpp:40-46): int(floor(u * scaling) / 5.0), C++ truncation and remainder."""
    ix = np.trunc(np.floor(u * tex.scaling) / 5.0).astype(np.int64)
    iy = np.trunc(np.floor(v * tex.scaling) / 5.0).astype(np.int64)
    even = np.fmod(ix + iy, 2) == 0
    c1, c2 = np.array(tex.color1[:], np.float32), np.array(tex.color2[:], np.float32)
    return np.where(even[..., None], c1, c2)


def has_environment(desc):
    return bool(desc.environment.present and desc.environment.loaded)


def restated_shader(desc, i):
    """whether _known_albedo knows the albedo of shader i"""
    sh = desc.shaders[i]
    if sh.kind in (0, 3, 4):
        return True
    return sh.kind in (1, 2) and (sh.texture < 0 or desc.textures[sh.texture].kind == 0)


def _known_albedo(desc, hid, rec, o, d, env):
    """(albedo float32 [n, 3], known [n]) by the first-hit rule where this file can restate it: Const colour, Lambert / Phong colour (times a
    CheckerTexture's sample at the record's u, v), Refl / Refr mult, a light's colour; at a miss black without a loaded environment, else
    env(o, d), the environment's colour along the ray, where the caller has one to give.  BitmapTexture and Layered stay unknown."""
    alb, known = np.zeros((len(hid), 3), F32), np.zeros(len(hid), bool)
    for i in np.unique(hid):
        px = hid == i
        if i >= 0:
            sh = desc.shaders[desc.nodes[int(i)].shader]
            if not restated_shader(desc, desc.nodes[int(i)].shader):
                continue
            if sh.kind in (3, 4):
                alb[px] = np.array(sh.mult[:], F32)
            elif sh.kind == 0 or sh.texture < 0:
                alb[px] = np.array(sh.color[:], F32)
            else:
                alb[px] = np.array(sh.color[:], F32) * _checker(desc.textures[sh.texture], rec[px][:, 7], rec[px][:, 8])
        elif i <= -2:
            alb[px] = np.array(desc.lights[-2 - int(i)].color[:], F32)
        elif has_environment(desc):
            if env is None:
                continue
            alb[px] = env(o[px], d[px])
        known[px] = True
    return alb, known


def walk_chain(desc, o0, d0, K, trace, env=None):
    """The chains of the rays (o0, d0) [n, 3] FP64 of one camera sample, at most K >= 0 steps each.  trace(o, d) -> (hit_id [m], rec [m, 9] = dist,
    ip, norm, u, v); env(o, d) -> float32 [m, 3], the environment's colour for rays that miss (None: such albedos are unknown).
    Returns flat arrays: the FP64 rows as the header defines them (pos, nrm, depth), alb (float32) and alb_known, b, the terminal hit's id / ip /
    normal, the first hit's id, the first step's ip and normal, the flags tir / limit, and the rays."""
    assert not any(desc.nodes[i].bump_tex >= 0 for i in range(desc.n_nodes)), "this walk applies no bump"
    assert K >= 0
    o0, d0 = np.ascontiguousarray(o0, np.float64), np.ascontiguousarray(d0, np.float64)
    n = len(o0)
    assert o0.shape == (n, 3) and d0.shape == (n, 3)
    kind = np.array([desc.shaders[desc.nodes[i].shader].kind for i in range(desc.n_nodes)])
    mult = np.array([desc.shaders[desc.nodes[i].shader].mult[:] for i in range(desc.n_nodes)], F32)
    ior = np.array([desc.shaders[desc.nodes[i].shader].ior for i in range(desc.n_nodes)], np.float64)
    o, d = o0.copy(), d0.copy()
    T, b = np.zeros(n), np.zeros(n, np.int32)
    A = np.ones((n, 3), F32)
    M = np.tile(np.eye(3), (n, 1, 1))
    live = np.ones(n, bool)
    pos, nrm, alb, depth = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3), F32), np.zeros(n)
    alb_known, tir_end, limit_end = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    t_id, t_ip, t_n = np.full(n, -1, np.int32), np.zeros((n, 3)), np.zeros((n, 3))
    m_ip, m_n, f_id = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, -1, np.int32)
    for seg in range(K + 1):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        hid, rec = trace(o[idx], d[idx])
        dist, ip, nm = rec[:, 0], rec[:, 1:4], rec[:, 4:7]
        if seg == 0:
            f_id[idx] = hid
        node = np.where(hid >= 0, hid, 0)
        spec = (hid >= 0) & np.isin(kind[node], (3, 4))
        want = spec & (b[idx] < K)
        di = d[idx]
        nf = _faceforward(di, nm)
        # Refraction::spawnRay: from outside 1 / ior, from inside ior / 1
        with np.errstate(divide="ignore"):
            my = np.where(_dot(nf, nm) > 0, 1.0 / ior[node], ior[node] / 1.0)
        rd, tir = _refract(di, nf, my)
        is_refr = kind[node] == 4
        step = want & ~(is_refr & tir)
        # the terminal rows
        e = ~step
        g = idx[e]
        first, hit = b[g] == 0, hid[e] != -1
        a0, known = _known_albedo(desc, hid[e], rec[e], o[g], di[e], env)
        Tn = T[g] + dist[e]
        virt = o0[g] + d0[g] * Tn[:, None]
        Mg, q = M[g], nm[e]
        unf = np.stack([(Mg[:, i, 0] * q[:, 0] + Mg[:, i, 1] * q[:, 1]) + Mg[:, i, 2] * q[:, 2] for i in range(3)], axis=1)
        z3 = np.zeros((len(g), 3))
        pos[g] = np.where(hit[:, None], np.where(first[:, None], ip[e], virt), z3)
        nrm[g] = np.where(hit[:, None], np.where(first[:, None], q, unf), z3)
        depth[g] = np.where(hit, np.where(first, dist[e], Tn), 0.0)
        alb[g] = np.where(first[:, None], a0, A[g] * a0)
        alb_known[g] = known
        tir_end[g] = (want & is_refr & tir)[e]
        limit_end[g] = (spec & ~want)[e]
        t_id[g], t_ip[g], t_n[g] = hid[e], ip[e], nm[e]
        live[g] = False
        # the steps
        g = idx[step]
        was_first = b[g] == 0
        m_ip[g[was_first]], m_n[g[was_first]] = ip[step][was_first], nm[step][was_first]
        A[g] = np.where(was_first[:, None], mult[node[step]], A[g] * mult[node[step]])
        T[g] = T[g] + dist[step]
        refl = kind[node[step]] == 3
        m = nm[step]
        Mg = M[g]
        u = np.stack([(Mg[:, i, 0] * m[:, 0] + Mg[:, i, 1] * m[:, 1]) + Mg[:, i, 2] * m[:, 2] for i in range(3)], axis=1)
        M[g] = np.where(refl[:, None, None], Mg - (2 * u)[:, :, None] * m[:, None, :], Mg)
        o[g] = np.where(refl[:, None], ip[step] + nf[step] * 1e-6, ip[step] - nf[step] * 1e-6)
        d[g] = np.where(refl[:, None], _reflect(di[step], m), rd[step])
        b[g] = b[g] + 1
    assert not live.any()
    return dict(pos=pos, nrm=nrm, alb=alb, alb_known=alb_known, depth=depth, b=b, tir=tir_end, limit=limit_end,
                t_id=t_id, t_ip=t_ip, t_n=t_n, f_id=f_id, m_ip=m_ip, m_n=m_n, o0=o0, d0=d0)


def reshaped(ch, shape):
    """a walk's flat arrays as [shape..., ...]"""
    return {k: a.reshape(tuple(shape) + a.shape[1:]) for k, a in ch.items()}


# ---- the two traces ------------------------------------------------------------------------------------------------------------------------------
def query_trace(s):
    """the ray queries of an uploaded scene"""
    def trace(o, d):
        r = s.trace_rays(o, d, record=True)
        return r["hit_id"], r["hit_rec"]
    return trace


def oracle_trace(oracle, desc):
    """the CPU oracle's closest hit, one ray at a time"""
    import hostlane

    def trace(o, d):
        return hostlane.oracle_probe(oracle, desc, o, d)
    return trace


def shade_env(s):
    """The environment's colour along rays that miss, as Scene.shade_rays gives it on a Whitted scene (gi 0): raytrace() of a ray that hits
    nothing returns the environment's colour."""
    assert not s.settings.gi

    def env(o, d):
        return s.shade_rays(o, d) if len(o) else np.zeros((0, 3), F32)
    return env


def walk_frame(s, K, xy=None, env=None):
    """walk_chain over an uploaded scene's camera rays through the film positions xy [H, W, 2] (None: every integer pixel, sample 0 of a Whitted
    frame without AA or DOF), fed by the ray queries; arrays shaped [H, W, ...]."""
    o0, d0 = s.camera_rays(xy)
    shape = o0.shape[:-1]
    return reshaped(walk_chain(s.desc, o0.reshape(-1, 3), d0.reshape(-1, 3), K, query_trace(s), env), shape)


# ---- samples --------------------------------------------------------------------------------------------------------------------------------------
def aa_positions(W, H, i):
    """film positions [H, W, 2] FP64 of sample i of a Whitted frame with wantAA: (float)x + (float)offset, widened"""
    xs, ys = pixel_grid(W, H)
    ox, oy = AA_OFFSETS[i]
    return np.stack([(xs + F32(ox)).astype(np.float64), (ys + F32(oy)).astype(np.float64)], axis=-1)


def jittered_positions(W, H, i, seed, sample_seed, jitter):
    """Film positions [H, W, 2] FP64 of sample i of a gi frame.  sample_seed(seed, pixels, i) -> uint32 seeds and jitter(seeds) -> float32 [n, 2],
    the first two floats of each seed's generator, are the caller's (tests/test_gpu_shade.py's on the GPU, the oracle's generator on the CPU)."""
    xs, ys = pixel_grid(W, H)
    j = np.asarray(jitter(sample_seed(seed, np.arange(W * H, dtype=np.uint32), i)), F32).reshape(H, W, 2)
    return np.stack([(xs + j[..., 0]).astype(np.float64), (ys + j[..., 1]).astype(np.float64)], axis=-1)


def reduce_samples(rows):
    """The feature channels' reduction over a pixel's samples (k_features, k_features_specular): every sample's row converted to float32, summed in
    float32 in sample order starting FROM sample 0's row (not from zero: -0.0 stays -0.0), divided once by float32(n) when n > 1."""
    rows = [np.asarray(r).astype(F32) for r in rows]
    acc = rows[0]
    for r in rows[1:]:
        acc = acc + r
    return acc / F32(len(rows)) if len(rows) > 1 else acc


def reduce_walks(walks):
    """reduce_samples over the rows of the samples' walks: (feat [..., 10], bounces [...], known [...]: every sample's albedo is known)"""
    rows = [np.concatenate([ch["pos"], ch["nrm"], ch["alb"], ch["depth"][..., None]], axis=-1) for ch in walks]
    known = np.all([ch["alb_known"] for ch in walks], axis=0)
    return reduce_samples(rows), reduce_samples([ch["b"] for ch in walks]), known


# ---- the kernel flag word ---------------------------------------------------------------------------------------------------------------------------
def flag_word(desc):
    """The even kernel flag word a scene is created with (entry_support.hpp flag_word; the facts of scene_arena.hpp): a Cube / CSG geometry on a
    node 2, else a mesh with a KD-tree (the mesh record's has_kd) 4, else a texture or a loaded environment 8, else 0."""
    if any(desc.geoms[desc.nodes[i].geom].kind in (2, 4) for i in range(desc.n_nodes)):
        return 2
    if any(desc.meshes[i].has_kd for i in range(desc.n_meshes)):
        return 4
    if desc.n_textures > 0 or has_environment(desc):
        return 8
    return 0
