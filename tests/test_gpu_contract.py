"""Option "fp_contract" (include/frayhip.h): the relaxed primitives of fray_amd/csrc/render_contract.hip measured against 200-bit references, and
contracted frames against the CPU oracle, whose arithmetic stays the reference's.

Part 1 runs the primitives through frayhip_debug_arith, which is compiled in the same translation unit, with the same flags, as the contracted kernels
(-ffp-contract=fast -DFRAY_ARITH=1) and calls the same inline functions.  Errors are counted in units in the last place of the correctly rounded result.
Part 2 renders path-traced frames with the option on: colour within north_star's 1e-4 RMS per channel, nearly every pixel within 1e-5, the oracle's
sample count, and launches of the contracted kernels.  Part 3 asserts the invariances a contracted frame keeps and the exclusions the header states."""
import math
import os

import numpy as np
import pytest

from conftest import ROOT, bucket_xy, open_scene

from mpmath import libmp, mp, mpf

RMS_TOL = 1e-4                      # per channel, north_star (include/frayhip.h, option "fp_contract")
PIX_TOL = 1e-5                      # a pixel is "close" when every channel is within PIX_TOL * max(1, |ref|)
ULP_TOL = 2                         # dev_math.hpp: "an ulp or two"
OP_RCP, OP_DIV, OP_RSQRT, OP_SQRT, OP_NORM, OP_SEG, OP_SINCOS, OP_ACOS_SINCOS = range(8)
DBL_MIN, DBL_MAX, DBL_TRUE_MIN = 2.0 ** -1022, float(np.finfo(np.float64).max), 2.0 ** -1074
TWO_PI = 2 * math.pi


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------------------

def arith(fray, op, a, b=None):
    """frayhip_debug_arith on host arrays; a (and b) are [n] or [n, 3]."""
    a = np.ascontiguousarray(a, np.float64)
    n = a.shape[0]
    width = {OP_NORM: 3, OP_SEG: 3, OP_SINCOS: 2, OP_ACOS_SINCOS: 2}.get(op, 1)
    out = np.full((n, width) if width > 1 else (n,), np.nan, np.float64)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, np.float64)
        assert b.shape == a.shape
        bp = b.ctypes.data
    rc = fray.lib.frayhip_debug_arith(op, n, a.ctypes.data, bp, out.ctypes.data)
    assert rc == 0, fray.lib.frayhip_last_error()
    return out


def rnd(x):
    """An mpf rounded once, to nearest, to a double."""
    return libmp.to_float(mpf(x)._mpf_, rnd="n")


def ordered(x):
    k = np.asarray(x, np.float64).view(np.int64)
    return np.where(k < 0, -(k & 0x7FFFFFFFFFFFFFFF), k)


def ulps(got, want):
    """Distance in representable doubles (want: the correctly rounded result)."""
    return np.abs(ordered(got) - ordered(want))


def ref_map(f, *cols):
    with mp.workprec(200):
        return np.array([rnd(f(*[mpf(float(c)) for c in args])) for args in zip(*cols)], np.float64)


def report(name, u):
    print("%-22s %7d operands: max %d ulp, %.4f %% correctly rounded" % (name, u.size, int(u.max()), 100 * float((u == 0).mean())))


def log_uniform(rng, n, lo, hi, signs=True):
    x = np.exp2(rng.uniform(lo, hi, n))
    if signs:
        x *= rng.choice([-1.0, 1.0], n)
    return x


def adversarial_mantissas():
    one = 1.0
    m = [one, 2.0 - np.spacing(1.0), 1.5, 1.5 + np.spacing(1.5), 1.5 - np.spacing(1.5)]
    for k in range(1, 9):
        m += [one + k * np.spacing(one), one - k * np.spacing(one) / 2]
    scales = [2.0 ** e for e in (-1000, -600, -300, -40, -12, -1, 0, 1, 7, 20, 300, 600, 999)]
    return np.array(sorted({s * v for s in scales for v in m}), np.float64)


def operands(seed, positive=False):
    """Log-uniform magnitudes over [2^-1000, 2^1000], the ranges the kernels see, and adversarial mantissas."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([log_uniform(rng, 6000, -1000, 1000),
                        rng.uniform(-1, 1, 3000),                              # direction components
                        log_uniform(rng, 3000, math.log2(1e-12), math.log2(1e6), signs=False),   # lengths, determinants
                        adversarial_mantissas(), -adversarial_mantissas()])
    x = x[x != 0]
    return np.abs(x) if positive else x


# ---- part 1: the primitives --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rcp", "div", "rsqrt", "sqrt"])
def test_relaxed_scalar_primitives_within_two_ulps(fray, gpu, name):
    """fray_rcp / fray_div / fray_rsqrt / fray_sqrt on normal operands whose results are normal: at most two ulps from the correctly rounded value."""
    if name == "rcp":
        a = operands(1)
        got, want = arith(fray, OP_RCP, a), ref_map(lambda x: 1 / x, a)
    elif name == "div":
        a, b = operands(2), operands(3)
        k = min(len(a), len(b))
        rng = np.random.default_rng(4)
        a, b = rng.permutation(a)[:k], rng.permutation(b)[:k]
        ok = np.abs(np.log2(np.abs(a)) - np.log2(np.abs(b))) < 1000          # quotient normal
        a, b = a[ok], b[ok]
        got, want = arith(fray, OP_DIV, a, b), ref_map(lambda x, y: x / y, a, b)
    elif name == "rsqrt":
        a = operands(5, positive=True)
        got, want = arith(fray, OP_RSQRT, a), ref_map(lambda x: 1 / mp.sqrt(x), a)
    else:
        a = operands(6, positive=True)
        got, want = arith(fray, OP_SQRT, a), ref_map(mp.sqrt, a)
    normal = (np.abs(want) >= DBL_MIN) & np.isfinite(want)
    assert normal.mean() > 0.99
    assert np.all(np.isfinite(got[normal])), a[normal][~np.isfinite(got[normal])][:5]
    u = ulps(got[normal], want[normal])
    report(name, u)
    worst = np.argsort(u)[-3:]
    assert u.max() <= ULP_TOL, (name, int(u.max()), a[normal][worst])


def vectors(seed):
    """Random, nearly axis-aligned, with one or two exact zero components; magnitudes 2^-30 .. 2^30."""
    rng = np.random.default_rng(seed)
    v = [rng.normal(size=(4000, 3))]
    near = np.zeros((1500, 3))
    ax = rng.integers(0, 3, 1500)
    near[np.arange(1500), ax] = rng.choice([-1.0, 1.0], 1500)
    near += rng.normal(size=(1500, 3)) * np.exp2(rng.uniform(-40, -8, (1500, 1)))
    v.append(near)
    for zeros in (1, 2):
        z = rng.normal(size=(1000, 3))
        for i in range(1000):
            z[i, rng.permutation(3)[:zeros]] = 0.0
        v.append(z)
    v.append(np.eye(3))
    v.append(-np.eye(3))
    v = np.concatenate(v)
    return v * np.exp2(rng.uniform(-30, 30, (len(v), 1)))


def check_unit(name, got, v):
    """Each component within two ulps of v_i / |v|; | |n|^2 - 1 | <= 2^-50."""
    want = np.empty_like(got)
    dev = 0.0
    with mp.workprec(200):
        for i in range(len(v)):
            x, y, z = (mpf(float(c)) for c in v[i])
            r = mp.sqrt(x * x + y * y + z * z)
            want[i] = [rnd(x / r), rnd(y / r), rnd(z / r)]
            gx, gy, gz = (mpf(float(c)) for c in got[i])
            dev = max(dev, float(abs(gx * gx + gy * gy + gz * gz - 1)))
    u = ulps(got, want)
    report(name, u)
    print("%-22s max | |n|^2 - 1 | = 2^%.2f" % (name, math.log2(dev) if dev else -math.inf))
    assert np.array_equal(got == 0, want == 0)                  # exact zero components stay exact zeros
    assert u.max() <= ULP_TOL, (name, int(u.max()), v[np.argmax(u.max(axis=1))])
    # dev_trace.hpp node_intersect under FRAY_ARITH: an untransformed node takes the direction as it comes and returns dist = t -- unit length is its precondition
    assert dev <= 2.0 ** -50, dev


@pytest.mark.gpu
def test_relaxed_normalized_gives_unit_vectors(fray, gpu):
    v = vectors(11)
    check_unit("normalized", arith(fray, OP_NORM, v), v)


@pytest.mark.gpu
def test_relaxed_segment_direction_gives_unit_vectors(fray, gpu):
    """visible(a, b)'s direction: d = b - a, d * fray_rcp(length(d)) (dev_trace.hpp), against (b - a) / |b - a| of the same double difference."""
    rng = np.random.default_rng(12)
    v = vectors(13)
    a = rng.normal(size=v.shape) * 10
    a[: len(a) // 4] = 0.0                                      # points at the origin: b - a is v itself
    b = a + v
    got = arith(fray, OP_SEG, a, b)
    check_unit("segment direction", got, b - a)


def sincos_operands():
    rng = np.random.default_rng(21)
    x = [rng.uniform(0, TWO_PI, 12000), rng.uniform(0, math.pi / 64, 2000), np.array([0.0, np.nextafter(TWO_PI, 0), TWO_PI / 2])]
    with mp.workprec(200):
        for k in range(256):                                    # the reduction's boundaries: multiples of pi/128, one and two ulps either side
            c = rnd(k * mp.pi / 128)
            x.append(np.array([c, np.nextafter(c, 0), np.nextafter(c, 9), np.nextafter(np.nextafter(c, 0), 0), np.nextafter(np.nextafter(c, 9), 9)]))
    x = np.concatenate(x)
    return x[(x >= 0) & (x < TWO_PI)]


@pytest.mark.gpu
def test_relaxed_sincos_on_the_samplers_range(fray, gpu):
    """The relaxed fray_sincos on [0, 2 pi): absolute error at most 2^-51 (two ulps of a value in [0.5, 1], a direction component).  Away from the zeros
    of the result (|value| >= 2^-7), where the plain-double reduction's missing third part of pi/128 does not dominate, also within two ulps."""
    x = sincos_operands()
    got = arith(fray, OP_SINCOS, x)
    ws, wc = np.empty_like(x), np.empty_like(x)
    es, ec, norm = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    with mp.workprec(200):
        for i, xv in enumerate(x):
            s, c = mp.sin(mpf(float(xv))), mp.cos(mpf(float(xv)))
            ws[i], wc[i] = rnd(s), rnd(c)
            gs, gc = mpf(float(got[i, 0])), mpf(float(got[i, 1]))
            es[i], ec[i] = float(abs(gs - s)), float(abs(gc - c))
            norm[i] = float(gs * gs + gc * gc - 1)
    print("relaxed sin / cos      %7d operands: max abs error 2^%.2f / 2^%.2f; sin^2 + cos^2 - 1 in [%.3g, %.3g]"
          % (len(x), math.log2(es.max()), math.log2(ec.max()), norm.min(), norm.max()))
    assert es.max() <= 2.0 ** -51, x[np.argmax(es)]
    assert ec.max() <= 2.0 ** -51, x[np.argmax(ec)]
    for name, g, w in (("relaxed sin", got[:, 0], ws), ("relaxed cos", got[:, 1], wc)):
        big = np.abs(w) >= 2.0 ** -7
        u = ulps(g[big], w[big])
        report(name + " |v|>=2^-7", u)
        assert u.max() <= ULP_TOL, (name, int(u.max()), x[big][np.argmax(u)])
    z = np.flatnonzero(x == 0)
    assert len(z) and np.all(got[z, 0] == 0) and np.all(got[z, 1] == 1)     # x = 0


@pytest.mark.gpu
def test_relaxed_acos_sincos(fray, gpu):
    """fray_acos_sincos(v): c is v exactly, s within two ulps of sqrt(1 - v^2)."""
    rng = np.random.default_rng(31)
    one_minus = np.nextafter(1.0, 0)
    v = np.concatenate([rng.uniform(-1, 1, 12000), 1 - np.exp2(rng.uniform(-52, -1, 1000)), -1 + np.exp2(rng.uniform(-52, -1, 1000)),
                        [-1.0, one_minus, 0.0, -0.0, 2.0 ** -30, -(2.0 ** -30), np.nextafter(-1.0, 0)]])
    v = v[(v >= -1) & (v < 1)]
    got = arith(fray, OP_ACOS_SINCOS, v)
    assert np.array_equal(got[:, 1], v) and np.array_equal(np.signbit(got[:, 1]), np.signbit(v))
    want = ref_map(lambda x: mp.sqrt(1 - x * x), v)
    u = ulps(got[:, 0], want)
    report("acos_sincos s", u)
    assert u.max() <= ULP_TOL, (int(u.max()), v[np.argmax(u)])


def cls(x):
    if math.isnan(x):
        return "nan"
    sign = "-" if math.copysign(1.0, x) < 0 else "+"
    if math.isinf(x):
        return sign + "inf"
    if x == 0:
        return sign + "0"
    return sign + ("sub" if abs(x) < DBL_MIN else "normal")


SPECIALS = [0.0, -0.0, math.inf, -math.inf, math.nan, DBL_TRUE_MIN, DBL_MIN, 2.0 ** 1022, DBL_MAX]
SPECIAL_NAMES = ["+0", "-0", "+inf", "-inf", "nan", "2^-1074", "2^-1022", "2^1022", "DBL_MAX"]
# What the device returns for each special operand, beside IEEE's result (classes: nan, +-inf, +-0, +-sub(normal), +-normal; a normal result is also within
# two ulps of the correctly rounded one).  The refinement steps turn the hardware's inf / 0 at a zero, infinite or too small operand into NaN
# (-x * r = -0 * inf).  Where the classes differ, every call site of the primitive keeps the operand out or ends with the same answer under IEEE
# (the audit is in dev_math.hpp beside the primitives).
SPECIAL_TABLE = {
    #          +0        -0        +inf      -inf      nan    2^-1074   2^-1022    2^1022     DBL_MAX
    "rcp":   ["nan",    "nan",    "nan",    "nan",    "nan", "nan",    "+normal", "+normal", "+sub"],
    "div1":  ["nan",    "nan",    "nan",    "nan",    "nan", "nan",    "+normal", "+normal", "+sub"],
    "rsqrt": ["nan",    "nan",    "nan",    "nan",    "nan", "+normal", "+normal", "+normal", "+normal"],
    "sqrt":  ["+0",     "-0",     "nan",    "nan",    "nan", "+normal", "+normal", "+normal", "+normal"],
}
IEEE_TABLE = {
    "rcp":   ["+inf",   "-inf",   "+0",     "-0",     "nan", "+inf",   "+normal", "+normal", "+sub"],
    "div1":  ["+inf",   "-inf",   "+0",     "-0",     "nan", "+inf",   "+normal", "+normal", "+sub"],
    "rsqrt": ["+inf",   "-inf",   "+0",     "nan",    "nan", "+normal", "+normal", "+normal", "+normal"],
    "sqrt":  ["+0",     "-0",     "+inf",   "nan",    "nan", "+normal", "+normal", "+normal", "+normal"],
}


@pytest.mark.gpu
def test_relaxed_primitives_on_special_operands(fray, gpu):
    """The special operands: +-0, +-inf, NaN, the smallest subnormal, 2^-1022, 2^1022 and DBL_MAX -- the device's results as a table, beside IEEE's."""
    x = np.array(SPECIALS, np.float64)
    got = {"rcp": arith(fray, OP_RCP, x), "div1": arith(fray, OP_DIV, np.ones_like(x), x), "rsqrt": arith(fray, OP_RSQRT, x), "sqrt": arith(fray, OP_SQRT, x)}
    refs = {"rcp": lambda v: 1 / v, "div1": lambda v: 1 / v, "rsqrt": lambda v: 1 / mp.sqrt(v), "sqrt": mp.sqrt}
    with np.errstate(all="ignore"):
        ieee = {"rcp": 1.0 / x, "div1": 1.0 / x, "rsqrt": 1.0 / np.sqrt(x), "sqrt": np.sqrt(x)}
    print("%-6s" % "op" + "".join("%18s" % n for n in SPECIAL_NAMES))
    for op in got:
        print("%-6s" % op + "".join("%18s" % ("%s (%s)" % (cls(g), cls(i))) for g, i in zip(got[op], ieee[op])) + "     device (IEEE)")
    for op in got:
        assert [cls(v) for v in ieee[op]] == IEEE_TABLE[op], op
        assert [cls(v) for v in got[op]] == SPECIAL_TABLE[op], (op, [cls(v) for v in got[op]])
        for k, v in enumerate(got[op]):
            if cls(v).endswith("normal"):
                with mp.workprec(200):
                    w = rnd(refs[op](mpf(float(x[k]))))
                assert ulps(np.array([v]), np.array([w]))[0] <= ULP_TOL, (op, SPECIAL_NAMES[k], v, w)
    # the zero vector and a segment of length zero (visible() with a == b): NaN, as under IEEE (0 * inf)
    z = np.zeros((1, 3))
    assert np.all(np.isnan(arith(fray, OP_NORM, z))) and np.all(np.isnan(arith(fray, OP_SEG, z + 1.5, z + 1.5)))


def test_debug_arith_rejects_bad_arguments(fray, abi):
    """Argument checks come before any HIP call: no GPU needed."""
    a = np.ones(3)
    out = np.zeros(3)
    f = fray.lib.frayhip_debug_arith
    assert f(8, 1, a.ctypes.data, None, out.ctypes.data) == abi.E_ARG
    assert f(-1, 1, a.ctypes.data, None, out.ctypes.data) == abi.E_ARG
    assert f(OP_RCP, 0, a.ctypes.data, None, out.ctypes.data) == abi.E_ARG
    assert f(OP_RCP, (1 << 22) + 1, a.ctypes.data, None, out.ctypes.data) == abi.E_ARG
    assert f(OP_RCP, 1, None, None, out.ctypes.data) == abi.E_ARG
    assert f(OP_RCP, 1, a.ctypes.data, None, None) == abi.E_ARG
    assert f(OP_DIV, 1, a.ctypes.data, None, out.ctypes.data) == abi.E_ARG          # b is read by ops 1 and 5
    assert f(OP_SEG, 1, a.ctypes.data, None, out.ctypes.data) == abi.E_ARG
    assert b"frayhip_debug_arith" in fray.lib.frayhip_last_error()


# ---- part 2: contracted frames against the oracle ----------------------------------------------------------------------------------------------------

def check_contracted(name, s, img, st, ref, ost, eyes=None):
    """st: the counting kernels' figures (None for a timed frame, which counts nothing)."""
    assert np.all(np.isfinite(img)), name
    r = np.sqrt(((img.astype(np.float64) - ref) ** 2).mean(axis=(0, 1)))
    far = int((np.abs(img.astype(np.float64) - ref) > PIX_TOL * np.maximum(1.0, np.abs(ref))).any(axis=2).sum())
    npix = img.shape[0] * img.shape[1]
    same = float((img == ref).all(axis=2).mean())
    n = s.get_option("contracted_launches")
    print("%s: rms %s, %.3f %% bit-identical, %d pixels beyond 1e-5, %d contracted launches" % (name, r, 100 * same, far, n))
    assert np.all(r <= RMS_TOL), (name, r)
    assert far <= max(1, npix // 1000), (name, far)
    if st is not None:
        assert st["samples"] == ost["samples"] == img.shape[0] * img.shape[1] * s.samples_per_pixel() * eyes, name
    assert n > 0, name


def PT_CASES():
    from test_gpu_parity import PT
    return PT


@pytest.mark.gpu
@pytest.mark.parametrize("scene,W,H,over", PT_CASES(), ids=lambda v: v if isinstance(v, str) else None)
def test_contracted_path_traced_frames_vs_oracle(fray, abi, oracle, gpu, scene, W, H, over):
    """The path-traced cases of test_gpu_parity (stereo, DOF, saturation, three RectLights, Phong under gi, depth 2) with the option on; timed and counting kernels."""
    s = open_scene(fray, scene, W, H, gi=1, **{k: v for k, v in over.items() if k != "gi"})
    s.beginRender()
    s.set_option("fp_contract", 1)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42, threads=16)
    eyes = 2 if s.camera.stereoSeparation > 0 else 1
    imgs = []
    for stats in (False, True):
        img, st = s.render(seed=42, stats=stats)
        check_contracted("%s %s stats=%d" % (scene, over, stats), s, img, st if stats else None, ref, ost, eyes)
        imgs.append(img)
    assert np.array_equal(imgs[0], imgs[1])                    # the counting twin renders the same contracted picture
    if scene == "zaphod.fray":                                  # PointLight only: the reference's path tracer sees no light at all
        assert ref.max() == 0 and imgs[0].max() == 0
    else:
        assert ref.mean() > 1e-3
    s.close()


# Fixed before any result was seen: flavour 1 = KD meshes (flag words 4 / 5), flavour 2 = lean, textured, bump maps (8 / 9)
GEN_SEEDS = {1: list(range(300, 310)), 2: list(range(400, 410))}


def generated(fray, tmp_path, seed, flavour, gi=1):
    from test_fuzz_parity import random_scene
    rng = np.random.default_rng(1000 + seed)
    return fray.Scene.parseScene(random_scene(rng, tmp_path, gi, flavour=flavour))


def test_generated_seeds_cover_what_they_claim(fray, tmp_path):
    """The fixed seeds' scenes (no GPU): every flavour-2 set holds bump maps and bitmap textures somewhere, flavour 1 holds a mesh big enough for a KD-tree."""
    from test_fuzz_parity import random_scene
    bumps = 0
    for fl, seeds in GEN_SEEDS.items():
        for seed in seeds:
            d = tmp_path / ("%d_%d" % (fl, seed))
            d.mkdir()
            text = open(random_scene(np.random.default_rng(1000 + seed), d, 1, flavour=fl)).read()
            assert "Cube" not in text and "Csg" not in text
            if fl == 2:
                bumps += "bump dents" in text
    assert bumps >= 3, bumps


@pytest.mark.gpu
@pytest.mark.parametrize("flavour,seed", [(fl, sd) for fl, seeds in GEN_SEEDS.items() for sd in seeds])
def test_contracted_generated_scenes_vs_oracle(fray, abi, oracle, gpu, tmp_path, flavour, seed):
    s = generated(fray, tmp_path, seed, flavour)
    s.beginRender()
    s.set_option("fp_contract", 1)
    img, st = s.render(seed=seed, stats=True)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=seed, threads=16)
    assert (ost["kd_inner_visits"] > 0) == (flavour == 1)       # the flag word the flavour claims: KD walk or none
    eyes = 2 if s.camera.stereoSeparation > 0 else 1
    check_contracted("generated flavour %d seed %d" % (flavour, seed), s, img, st, ref, ost, eyes)
    img2, _ = s.render(seed=seed)
    assert np.array_equal(img, img2)
    s.close()


@pytest.mark.gpu
def test_contracted_kd_frame_across_lanes_vs_oracle(fray, abi, oracle, gpu):
    """boxed at 320 x 240, 12 spp: KD meshes at a size whose batches run on several lanes."""
    s = open_scene(fray, "boxed.fray", 320, 240, gi=1, numPaths=12)
    s.beginRender()
    s.set_option("fp_contract", 1)
    img, st = s.render(seed=42)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42, threads=16)
    check_contracted("boxed 320x240 12 spp", s, img, None, ref, ost)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth,stereo", [(40, 0.0), (40, 1.5), (150, 0.0), (150, 1.5)])
def test_contracted_long_generator_frames(fray, abi, oracle, gpu, depth, stereo):
    """maxTraceDepth >= 20 (per-path generator state): the bounces stay exact and only the shadow kernel is contracted (render_impl.hpp).  A frame of one
    batch launches the shadow kernel once per bounce level and eye -- maxTraceDepth + 2 levels -- and nothing else of the contracted build."""
    s = fray.Scene.parseScene(os.path.join(ROOT, "tests", "scenes", "whitebox.fray"))
    s.settings.maxTraceDepth = depth
    s.camera.stereoSeparation = stereo
    s.beginRender()
    s.set_option("fp_contract", 1)
    eyes = 2 if stereo > 0 else 1
    img, st = s.render(seed=42, stats=True)
    ref, ost = oracle.render(s.desc, abi.MODE_RENDER, seed=42, threads=16)
    assert ref.mean() > 0.05
    check_contracted("whitebox depth %d stereo %g" % (depth, stereo), s, img, st, ref, ost, eyes)
    n_default = s.get_option("contracted_launches")
    assert n_default % (eyes * (depth + 2)) == 0, n_default
    spp = s.samples_per_pixel()
    one, _ = s.render(seed=42, spp_chunk=spp)
    assert s.get_option("contracted_launches") == eyes * (depth + 2)      # shadow launches only: no bounce (depth + 1 more per eye) ran contracted
    assert np.array_equal(one, img)
    s.close()


# ---- part 3: invariances and exclusions ---------------------------------------------------------------------------------------------------------------

def bucket_mask(W, H, first, stride):
    BW, BH = (W - 1) // 48 + 1, (H - 1) // 48 + 1
    m = np.zeros((H, W), bool)
    for b in range(first, BW * BH, stride):
        bx, by = bucket_xy(W, b)
        m[by * 48:(by + 1) * 48, bx * 48:(bx + 1) * 48] = True
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("scene,W,H,over", [("cornell_box.fray", 150, 100, dict(numPaths=8)),
                                            ("boxed.fray", 110, 100, dict(numPaths=6)),
                                            ("cornell_box.fray", 100, 60, dict(numPaths=4, stereoSeparation=12.0))])
def test_contracted_frame_invariances(fray, abi, gpu, scene, W, H, over):
    """spp_chunk, strided bucket subsets and a progressive frame with a callback on every batch each give the blocking contracted frame bit for bit."""
    s = open_scene(fray, scene, W, H, gi=1, **over)
    s.beginRender()
    s.set_option("fp_contract", 1)
    full, _ = s.render(seed=42)
    n_full = s.get_option("contracted_launches")
    assert n_full > 0
    spp = s.samples_per_pixel()
    eyes = 2 if s.camera.stereoSeparation > 0 else 1
    nb = s.settings.maxTraceDepth + 2
    for chunk in (1, 2, spp):
        img, _ = s.render(seed=42, spp_chunk=chunk)
        assert np.array_equal(img, full), (chunk, int((img != full).any(axis=2).sum()))
        # every batch and eye: each bounce but the first, and every level's shadow kernel
        assert s.get_option("contracted_launches") == -(-spp // chunk) * eyes * (2 * nb - 1), chunk
    union = np.zeros_like(full)
    for r in range(3):
        img, _ = s.render(seed=42, bucket_first=r, bucket_stride=3)
        m = bucket_mask(W, H, r, 3)
        assert m.any() and np.array_equal(img[m], full[m]) and not img[~m].any(), r
        union += img
    assert np.array_equal(union, full)
    # progressive, one batch per sample and a callback after every batch: the blocking frame, and the launches of the blocking frame of the same batches
    calls = []
    img, st = s.render(seed=42, spp_chunk=1, progress=lambda info: calls.append((info["batches_done"], info["final"])) and None, preview_ms=0)
    assert len(calls) >= 2 and calls[-1] == (spp, 1) and not st["cancelled"], calls
    assert np.array_equal(img, full)
    assert s.get_option("contracted_launches") == spp * eyes * (2 * nb - 1)
    img, _ = s.render(seed=42, progress=lambda info: None, preview_ms=0)
    assert np.array_equal(img, full) and s.get_option("contracted_launches") == n_full
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["csg_nested", "generated_flavour0", "whitted_cornell", "whitted_boxed", "whitted_generated"])
def test_option_does_nothing_where_the_header_says(fray, abi, gpu, tmp_path, what):
    """Cube / CSG scenes (flag words 2 / 3) have no contracted kernels and Whitted frames never use them: the option renders the exact frame and
    launches nothing of the contracted build."""
    if what == "csg_nested":
        s = fray.Scene.parseScene(os.path.join(ROOT, "tests", "scenes", "csg_nested.fray"))
        s.settings.frameWidth, s.settings.frameHeight, s.settings.gi, s.settings.numPaths = 96, 72, 1, 4
    elif what == "generated_flavour0":
        s = generated(fray, tmp_path, 7, 0, gi=1)
    elif what == "whitted_cornell":
        s = open_scene(fray, "cornell_box.fray", 96, 96, gi=0)
    elif what == "whitted_boxed":
        s = open_scene(fray, "boxed.fray", 96, 72, gi=0, wantAA=0)
    else:
        s = generated(fray, tmp_path, 305, 1, gi=0)
    s.beginRender()
    exact, _ = s.render(seed=3)
    assert exact.max() > 0
    s.set_option("fp_contract", 1)
    for stats in (False, True):
        img, _ = s.render(seed=3, stats=stats)
        assert s.get_option("contracted_launches") == 0, (what, stats)
        assert np.array_equal(img, exact), (what, stats)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,W,H", [("cornell_box.fray", 97, 61), ("boxed.fray", 100, 75), ("smallpt.fray", 80, 60)])
def test_primary_hits_ignore_the_option(fray, abi, gpu, scene, W, H):
    s = open_scene(fray, scene, W, H, wantAA=0, gi=1)
    s.beginRender()
    ids, dist, _ = s.primary_hits()
    s.set_option("fp_contract", 1)
    ids2, dist2, _ = s.primary_hits()
    assert np.array_equal(ids, ids2) and np.array_equal(dist.view(np.int64), dist2.view(np.int64))
    s.close()
