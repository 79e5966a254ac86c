"""Specular feature frames on the GPU (include/frayhip.h "specular feature frames"):
1. sample 0 of a plain Whitted frame pinned bit for bit by a numpy walk of the chain over the ray queries' hit records and the shader table;
2. total internal reflection ends a chain;
3. behind one planar mirror the virtual position is the mirror image of the terminal hit, and the unfolded normal that of its normal;
4. a pixel none of whose samples took a step has frayhip_render_features' row; a scene without Refl / Refr has it everywhere;
5. the contract of frayhip_render_features, for both outputs;
6. render_denoised / render_sequence with specular=K are their pieces."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, open_scene
from test_gpu_denoise import FIGURES

pytestmark = pytest.mark.gpu
F32 = np.float32


# the chain, restated: tests/specular_ref.py; walk_chain here is its walk over the integer-pixel camera rays, fed by the ray queries
from specular_ref import _faceforward, walk_frame as walk_chain


def _assert_pinned(s, ch, K, label):
    feat, plane = s.render_features_specular(K, 1, bounces=True)
    assert np.array_equal(plane, ch["b"].astype(F32)), label
    assert np.array_equal(feat[..., 0:3], ch["pos"].astype(F32)), label
    assert np.array_equal(feat[..., 9], ch["depth"].astype(F32)), label
    assert np.array_equal(feat[..., 3:6], ch["nrm"].astype(F32)), label
    k = ch["alb_known"]
    assert k.mean() > 0.9 and np.array_equal(feat[k][:, 6:9], ch["alb"][k]), label
    return feat, plane


# ---- 1. pinned by the walk -------------------------------------------------------------------------------------------------------------------------
W, H = 160, 120


def _plain(fray, name, **over):
    return open_scene(fray, name, W, H, gi=0, wantAA=0, dof=0, **over)


def _shader_index(desc, kind):
    return next(desc.nodes[i].shader for i in range(desc.n_nodes) if desc.shaders[desc.nodes[i].shader].kind == kind)


CORNELL_LEFT, CORNELL_RIGHT = 4, 3          # cornell_box.fray's nodes in file order: floor, ceiling, backwall, rightwall, leftwall, shortblock, tallblock


def _facing_mirrors(fray):
    """cornell_box with both side walls mirrors, seen from inside the box, looking from the left wall at the right one: the rays near the
    axis bounce between the two until the limit ends them."""
    s = _plain(fray, "cornell_box.fray")
    desc = s.desc
    mirror = _shader_index(desc, 3)
    for i in (CORNELL_LEFT, CORNELL_RIGHT):
        assert desc.shaders[desc.nodes[i].shader].kind == 1
        desc.nodes[i].shader = mirror
    s.camera.pos[0], s.camera.pos[1], s.camera.pos[2] = 500.0, 400.0, 279.0
    s.camera.yaw, s.camera.pitch = 90.0, 0.0
    return s


@pytest.fixture(scope="module")
def cornell(fray, gpu):
    s = _plain(fray, "cornell_box.fray")
    s.beginRender()
    yield s, {K: walk_chain(s, K) for K in (1, 2, 8)}
    s.close()


@pytest.mark.parametrize("K", [1, 2, 8])
def test_cornell_is_pinned(cornell, K):
    s, chains = cornell
    ch = chains[K]
    _assert_pinned(s, ch, K, "cornell K=%d" % K)
    assert (ch["b"] == 1).sum() > 200 and (ch["b"] == 0).sum() > 200
    # the open front: some reflected rays leave the box, and their rows are zero but for the albedo
    gone = (ch["b"] > 0) & (ch["t_id"] == -1)
    assert gone.any() and not ch["pos"][gone].any() and not ch["depth"][gone].any()


@pytest.mark.parametrize("K", [1, 2, 8])
def test_smallpt_is_pinned(fray, gpu, K):
    s = _plain(fray, "smallpt.fray")
    s.beginRender()
    ch = walk_chain(s, K)
    _assert_pinned(s, ch, K, "smallpt K=%d" % K)
    desc = s.desc
    first = s.trace_rays(*s.camera_rays())["hit_id"]
    kinds = {int(i): desc.shaders[desc.nodes[int(i)].shader].kind for i in np.unique(first[first >= 0])}
    refl = np.isin(first, [i for i, k in kinds.items() if k == 3])
    refr = np.isin(first, [i for i, k in kinds.items() if k == 4])
    assert refl.sum() > 50 and refr.sum() > 50
    assert (ch["b"][refl] >= 1).all() and (ch["b"][refr] >= 1).all()
    assert (ch["b"] == K).any() if K <= 2 else True
    if K >= 2:                                           # into the glass sphere and out of it again
        assert (ch["b"][refr] >= 2).mean() > 0.9
    else:                                                # ... or stopped inside it, at the limit, with the glass's own mult as the terminal albedo
        assert ch["limit"][refr].all()
    s.close()


@pytest.mark.parametrize("K", [1, 2, 8])
def test_facing_mirrors_are_pinned_up_to_the_limit(fray, gpu, K):
    s = _facing_mirrors(fray)
    s.beginRender()
    ch = walk_chain(s, K)
    feat, plane = _assert_pinned(s, ch, K, "facing mirrors K=%d" % K)
    at_limit = ch["limit"]
    assert at_limit.sum() > 20 and (ch["b"][at_limit] == K).all() and plane.max() == K
    # a chain the limit ended: the mirror's own row as the virtual hit, the product one mult longer
    mult = np.array(s.desc.shaders[_shader_index(s.desc, 3)].mult[:], F32)
    want = mult.copy()
    for _ in range(K):
        want = want * mult
    assert np.array_equal(feat[at_limit][:, 6:9], np.broadcast_to(want, (at_limit.sum(), 3)))
    assert (feat[at_limit][:, 9] > 0).all()
    if K == 8:
        assert len(np.unique(ch["b"])) >= 4              # and chains of other lengths beside them
    s.close()


# ---- 2. total internal reflection -------------------------------------------------------------------------------------------------------------------
SMALLPT_FLOOR = 2                            # smallpt.fray's nodes in file order: left, right, floor, ceiling, back, reflSphere, glassSphere


def test_total_internal_reflection_ends_the_chain(fray, gpu):
    """smallpt's floor made of glass and seen from under it: past the critical angle (41.8 degrees off the normal at ior 1.5) refract() returns
    the zero vector and the hit is the terminal, with the first-hit rule's row; steeper rays pass into the room."""
    s = _plain(fray, "smallpt.fray")
    desc = s.desc
    desc.nodes[SMALLPT_FLOOR].shader = _shader_index(desc, 4)
    s.camera.pos[0], s.camera.pos[1], s.camera.pos[2] = 50.0, -30.0, 100.0           # under the floor's 128 x 128 extent
    s.camera.yaw, s.camera.pitch = 180.0, 48.0
    s.beginRender()
    ch = walk_chain(s, 4)
    feat, plane = _assert_pinned(s, ch, 4, "glass floor")
    tir = ch["tir"]
    assert tir.sum() > 500 and (ch["b"][tir] == 0).all() and (ch["t_id"][tir] == SMALLPT_FLOOR).all()
    assert (plane > 0).sum() > 500                       # the others went through
    first = s.render_features(1)
    assert np.array_equal(feat[tir], first[tir])
    assert np.array_equal(feat[tir][:, 6:9], np.broadcast_to(np.array(desc.shaders[desc.nodes[SMALLPT_FLOOR].shader].mult[:], F32), (tir.sum(), 3)))
    s.close()


# ---- 3. geometry --------------------------------------------------------------------------------------------------------------------------------------
def test_one_planar_mirror_unfolds_to_the_mirror_image(cornell):
    """b == 1 behind the short block's faces.  With q the first hit, m its normal (unit), and R x = x - 2 ((x - q) . m) m the reflection across
    the face's plane: in exact arithmetic the terminal hit is q + m' 1e-6 + d' t (m' = m face-forwarded: spawn_ray's origin) and the virtual
    position q + d0 t, whose image is q + d' t, so R(virtual) + m' 1e-6 is the terminal ip, and R (without the translation) takes the unfolded
    normal back to the terminal normal.
    The bound: every quantity is a coordinate or a length of the scene, below L = 2^11 (the camera stands 800 in front of a box 560 deep), so one
    FP64 operation errs by at most L 2^-53.  The virtual position takes 4 operations per component, R 12, the kernel's q (o + d dist) and its
    terminal ip 3 each, the reflected direction 9 with its error carried over a length (counted as operations on L already), the face's normal
    is unit within 4 ulps and enters R twice: below 64 operations in all, and 128 L 2^-53 = 2.9e-11 leaves a factor of two.  For the normal
    the same count at unit scale: 128 2^-53."""
    s, chains = cornell
    ch = chains[1]
    one = (ch["b"] == 1) & (ch["t_id"] != -1)
    assert one.sum() > 200
    q, m = ch["m_ip"][one], ch["m_n"][one]
    assert np.abs(np.einsum("ij,ij->i", m, m) - 1).max() <= 2.0 ** -50
    R = lambda x: x - 2 * np.einsum("ij,ij->i", x, m)[:, None] * m
    mf = _faceforward(ch["d0"][one], m)
    image = q + R(ch["pos"][one] - q) + mf * 1e-6
    bound = 128 * 2.0 ** 11 * 2.0 ** -53
    err = np.abs(image - ch["t_ip"][one]).max()
    print("mirror image: max error %.3g, bound %.3g" % (err, bound))
    assert err <= bound
    nerr = np.abs(R(ch["nrm"][one]) - ch["t_n"][one]).max()
    print("unfolded normal: max error %.3g, bound %.3g" % (nerr, 128 * 2.0 ** -53))
    assert nerr <= 128 * 2.0 ** -53
    # and the frame holds those FP64 values rounded once
    feat = s.render_features_specular(1, 1)
    assert np.array_equal(feat[one][:, 0:3], ch["pos"][one].astype(F32))


# ---- 4. parity ------------------------------------------------------------------------------------------------------------------------------------------
def _scene_any(fray, name, **over):
    if name.startswith("tests/"):
        s = fray.Scene.parseScene(os.path.join(ROOT, *name.split("/")))
        s.settings.frameWidth, s.settings.frameHeight = W, H
        for k, v in over.items():
            setattr(s.settings if hasattr(s.settings, k) else s.camera, k, v)
        return s
    return open_scene(fray, name, W, H, **over)


@pytest.mark.parametrize("name", ["cornell_box.fray", "smallpt.fray", "forest.fray", "tests/scenes/csg_nested.fray"])
def test_pixels_without_a_step_have_the_first_hit_row(fray, gpu, name):
    s = _scene_any(fray, name, gi=1, numPaths=8)
    s.beginRender()
    K = 3
    first = s.render_features(4, seed=11)
    feat, plane = s.render_features_specular(K, 4, seed=11, bounces=True)
    same = plane == 0
    desc = s.desc
    own = any(desc.shaders[desc.nodes[i].shader].kind in (3, 4) for i in range(desc.n_nodes))
    assert own or name not in ("cornell_box.fray", "smallpt.fray")
    assert same.sum() > 500 and np.array_equal(feat[same], first[same])
    if own:
        assert (~same).sum() > 50 and not np.array_equal(feat[~same], first[~same])
    else:                                                # Refl / Refr shaders that no node carries itself (layers of Layered shaders at most)
        assert any(desc.shaders[i].kind in (3, 4) for i in range(desc.n_shaders)) and same.all()
    assert plane.min() >= 0 and plane.max() <= K and np.isfinite(feat).all()
    s.close()


def test_a_scene_without_specular_nodes_is_the_first_hit_frame(fray, gpu):
    s = open_scene(fray, "boxed.fray", W, H, gi=1, numPaths=8)
    desc = s.desc
    assert not any(desc.shaders[desc.nodes[i].shader].kind in (3, 4) for i in range(desc.n_nodes))
    s.beginRender()
    out = (np.full((H, W, 10), -3.0, F32), np.full((H, W), -3.0, F32))
    feat, plane = s.render_features_specular(8, 4, seed=3, bounces=True, out=out)
    assert np.array_equal(feat, s.render_features(4, seed=3)) and not plane.any()
    s.close()
    # the fact is looked up per call: cornell with its mirror block painted white by an update, and made a mirror again
    s = open_scene(fray, "cornell_box.fray", W, H, gi=1, numPaths=8)
    s.beginRender()
    block = next(i for i in range(s.desc.n_nodes) if s.desc.shaders[s.desc.nodes[i].shader].kind == 3)
    mirror, white = s.desc.nodes[block].shader, s.desc.nodes[0].shader
    with_mirror = s.render_features_specular(4, 4, seed=3, bounces=True)
    s.desc.nodes[block].shader = white
    s.update()
    feat, plane = s.render_features_specular(4, 4, seed=3, bounces=True)
    assert np.array_equal(feat, s.render_features(4, seed=3)) and not plane.any()
    s.desc.nodes[block].shader = mirror
    s.update()
    again = s.render_features_specular(4, 4, seed=3, bounces=True)
    assert with_mirror[1].any() and all(np.array_equal(a, b) for a, b in zip(with_mirror, again))
    s.close()


# ---- 5. the contract --------------------------------------------------------------------------------------------------------------------------------------
def _raw(fray, abi, s, K, n, seed=42, first=0, stride=1, chunk=0, out=None, flags=0):
    Wd, Hd = s.frame_size
    feat, plane = out if out is not None else (np.zeros((Hd, Wd, 10), F32), np.zeros((Hd, Wd), F32))
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=seed, bucket_first=first, bucket_stride=stride, spp_chunk=chunk, flags=flags)
    rc = fray.lib.frayhip_render_features_specular(s._dev, C.byref(fr), n, K, feat.ctypes.data, plane.ctypes.data if plane is not None else None, None)
    return rc, feat, plane


FRAMES = [("cornell_box.fray", dict(numPaths=8)), ("smallpt.fray", dict(numPaths=8)), ("forest.fray", dict(gi=0, dof=1, numDOFSamples=8))]


@pytest.mark.parametrize("name,over", FRAMES, ids=[f[0] for f in FRAMES])
def test_contract_of_gi_and_dof_frames(fray, abi, gpu, name, over):
    Wd, Hd = 150, 100
    s = open_scene(fray, name, Wd, Hd, **over)
    if name == "forest.fray":
        # no node of it carries its Refl / Refr shaders: its Phong mesh becomes a plain mirror (a KD scene under DOF)
        desc = s.desc
        mirror = next(i for i in range(desc.n_shaders) if desc.shaders[i].kind == 3)
        mesh = next(i for i in range(desc.n_nodes) if desc.geoms[desc.nodes[i].geom].kind == 3 and desc.shaders[desc.nodes[i].shader].kind == 2)
        desc.nodes[mesh].shader = mirror
    s.beginRender()
    img_before, _ = s.render(seed=9)
    before = {k: s.get_option(k) for k in FIGURES}
    a, pa = s.render_features_specular(4, 4, seed=9, bounces=True)
    assert np.isfinite(a).all() and np.any(a[..., 9] > 0) and pa.any() and pa.max() <= 4
    assert {k: s.get_option(k) for k in FIGURES} == before
    same = lambda r: np.array_equal(r[0], a) and np.array_equal(r[1], pa)
    assert same(s.render_features_specular(4, 4, seed=9, bounces=True))
    assert not np.array_equal(a, s.render_features_specular(4, 4, seed=10))            # jittered samples follow the seed
    assert np.array_equal(a, s.render_features_specular(4, 4, seed=9))                 # without the plane
    for opt, v in (("pt_lanes", 1), ("fp_contract", 1), ("pt_lanes", 4), ("fp_contract", 0)):
        s.set_option(opt, v)
        assert same(s.render_features_specular(4, 4, seed=9, bounces=True)), (opt, v)
    for chunk in (1, 3):
        rc, f, p = _raw(fray, abi, s, 4, 4, seed=9, chunk=chunk)
        assert rc == abi.OK and same((f, p))
    # the counting variant
    f, p, st = s.render_features_specular(4, 4, seed=9, bounces=True, stats=True)
    assert same((f, p)) and st["samples"] == Wd * Hd * 4 and st["closest_rays"] > st["samples"] and st["trace_launches"] == 1
    # disjoint bucket sets make up the full call; pixels outside a call's buckets are untouched, in both outputs
    part = (np.full((Hd, Wd, 10), -7.0, F32), np.full((Hd, Wd), -7.0, F32))
    assert _raw(fray, abi, s, 4, 4, seed=9, first=1, stride=3, out=part)[0] == abi.OK
    touched = np.any(part[0] != -7.0, axis=2)
    assert touched.any() and not touched.all() and np.array_equal(touched, part[1] != -7.0)
    for first in (0, 2):
        assert _raw(fray, abi, s, 4, 4, seed=9, first=first, stride=3, out=part)[0] == abi.OK
    assert same(part)
    # the device entry writes the same
    import torch
    t = torch.zeros((Hd, Wd, 10), dtype=torch.float32, device="cuda")
    tb = torch.zeros((Hd, Wd), dtype=torch.float32, device="cuda")
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=9)
    assert fray.lib.frayhip_render_features_specular_device(s._dev, C.byref(fr), 4, 4, t.data_ptr(), tb.data_ptr(), None, None) == abi.OK
    assert same((t.cpu().numpy(), tb.cpu().numpy()))
    t.zero_()
    assert fray.lib.frayhip_render_features_specular_device(s._dev, C.byref(fr), 4, 4, t.data_ptr(), None, None, None) == abi.OK
    assert np.array_equal(t.cpu().numpy(), a)
    # the frame itself is unchanged
    img_after, _ = s.render(seed=9)
    assert np.array_equal(img_before, img_after)
    s.close()


def test_refusals(fray, abi, gpu):
    s = open_scene(fray, "cornell_box.fray", 64, 48, numPaths=4)
    s.beginRender()
    L = fray.lib
    err = lambda: L.frayhip_last_error().decode()
    assert _raw(fray, abi, s, 4, 5)[0] == abi.E_ARG and "n_samples" in err()
    for K in (0, -1, 9):
        assert _raw(fray, abi, s, K, 1)[0] == abi.E_ARG and "max_bounces" in err()
    buf = np.zeros(48 * 64 * 11 + 4, F32)
    fr = abi.Frame(mode=abi.MODE_RENDER, seed=1)
    base = buf.ctypes.data
    for off in (0, 4, 48 * 64 * 40 - 4):
        assert L.frayhip_render_features_specular(s._dev, C.byref(fr), 1, 4, base, base + off, None) == abi.E_ARG and "overlap" in err()
    for off in (48 * 64 * 4 - 4, 4):
        assert L.frayhip_render_features_specular(s._dev, C.byref(fr), 1, 4, base + 48 * 64 * 4, base + 48 * 64 * 4 - off, None) == abi.E_ARG
        assert "overlap" in err()
    assert L.frayhip_render_features_specular(s._dev, C.byref(fr), 1, 4, base, base + 48 * 64 * 40, None) == abi.OK
    import torch
    t = torch.zeros(48 * 64 * 11 + 4, dtype=torch.float32, device="cuda")
    assert L.frayhip_render_features_specular_device(s._dev, C.byref(fr), 1, 4, t.data_ptr(), t.data_ptr() + 48 * 64 * 40 + 2, None, None) == abi.E_ARG
    assert "aligned" in err()
    assert L.frayhip_render_features_specular_device(s._dev, C.byref(fr), 1, 4, t.data_ptr() + 2, None, None, None) == abi.E_ARG and "aligned" in err()
    assert L.frayhip_render_features_specular_device(s._dev, C.byref(fr), 1, 4, t.data_ptr(), t.data_ptr() + 8, None, None) == abi.E_ARG
    assert "overlap" in err()
    s.close()
    s = open_scene(fray, "cornell_box.fray", 64, 48, numPaths=4, maxTraceDepth=20)
    s.beginRender()
    assert _raw(fray, abi, s, 4, 1)[0] == abi.E_UNSUPPORTED and "maxTraceDepth" in err()
    s.close()
    s = open_scene(fray, "cornell_box.fray", 64, 48, numPaths=4, maxTraceDepth=-1)
    s.beginRender()
    rc, f, p = _raw(fray, abi, s, 4, 2, out=(np.full((48, 64, 10), 3.0, F32), np.full((48, 64), 3.0, F32)))
    assert rc == abi.OK and not f.any() and not p.any()
    s.close()
    s = open_scene(fray, "cornell_box.fray", 64, 48, stereoSeparation=12.0)
    s.beginRender()
    assert _raw(fray, abi, s, 4, 1)[0] == abi.E_UNSUPPORTED and "stereo" in err()
    s.close()


def test_the_answer_does_not_depend_on_the_handles_earlier_calls(fray, abi, gpu):
    """One handle: the call first, then after a frame, after a Whitted frame at another size, after an edit and its reversal through update(),
    after a motion call and after a first-hit call; every answer is the fresh handle's, byte for byte (the pattern of tests/call_history.py)."""
    def configure(s):
        s.settings.frameWidth, s.settings.frameHeight, s.settings.gi, s.settings.numPaths = 96, 64, 1, 6
        s.beginFrame()

    def answer(s):
        configure(s)
        f, p, st = s.render_features_specular(4, 4, seed=21, bounces=True, stats=True)
        return f.tobytes(), p.tobytes(), st["closest_rays"], st["samples"]

    s = open_scene(fray, "cornell_box.fray", 96, 64, numPaths=6)
    s.beginRender()
    base = answer(s)
    assert np.frombuffer(base[1], F32).any()

    def frame(s):
        configure(s)
        s.render(seed=5)

    def whitted(s):
        s.settings.frameWidth, s.settings.frameHeight, s.settings.gi = 200, 150, 0
        s.beginFrame()
        s.render(seed=5)

    def edit_and_back(s):
        n = s.desc.nodes[5]
        saved = bytes(n.T)
        fray.Transform(n).translate(30.0, 0.0, 10.0).store(n)
        s.update()
        configure(s)
        moved = s.render_features_specular(4, 4, seed=21)
        assert moved.tobytes() != base[0]
        C.memmove(C.byref(n.T), saved, len(saved))
        s.update()

    def motion(s):
        configure(s)
        s.render_features_motion(s.node_transforms(), 4, seed=21)

    def first_hit(s):
        configure(s)
        s.render_features(4, seed=21, stats=True)

    for before in (frame, whitted, edit_and_back, motion, first_hit, whitted):
        before(s)
        assert answer(s) == base, before.__name__
    s.close()
    s = open_scene(fray, "cornell_box.fray", 96, 64, numPaths=6)          # and on a handle whose first call it is not
    s.beginRender()
    whitted(s)
    assert answer(s) == base
    s.close()


# ---- 6. composition ---------------------------------------------------------------------------------------------------------------------------------------
def test_render_denoised_with_specular_guides_is_its_pieces(fray, gpu):
    s = open_scene(fray, "cornell_box.fray", 100, 70, numPaths=12)
    s.beginRender()
    den, raw, info = s.render_denoised(seed=7, feature_samples=4, specular=4)
    assert np.array_equal(raw, s.render(seed=7)[0])
    guides = s.render_features_specular(4, 4, seed=7)
    assert np.array_equal(info["features_frame"], guides) and not np.array_equal(guides, s.render_features(4, seed=7))
    assert np.array_equal(den, fray.denoise(raw, guides, info["rgb_half"]))
    den0, raw0, info0 = s.render_denoised(seed=7, feature_samples=4, specular=0)
    today = s.render_denoised(seed=7, feature_samples=4)
    assert np.array_equal(den0, today[0]) and np.array_equal(info0["features_frame"], s.render_features(4, seed=7))
    assert not np.array_equal(den, den0)
    dsp, rsp, isp = s.render_denoised_split(seed=7, feature_samples=4, specular=4)
    assert np.array_equal(isp["features_frame"], guides)
    assert np.array_equal(dsp, fray.denoise_signal(isp["direct_rgb"], isp["noise_direct"], guides, demodulate=0)
                          + fray.denoise_signal(isp["indirect_rgb"], isp["noise_indirect"], guides, demodulate=0))
    s.close()


def test_render_sequence_with_specular_guides(fray, abi, gpu):
    from fray_amd.__main__ import orbit
    s = open_scene(fray, "cornell_box.fray", 100, 70, numPaths=8)
    s.beginRender()
    start = abi.Camera.from_buffer_copy(s.camera)
    frames = [(o.cpu().numpy(), r.cpu().numpy(), i) for o, r, i in s.render_sequence(orbit(start, 2, 1.0), seed=7, specular=4)]
    plain = [(o.cpu().numpy(), r.cpu().numpy(), i) for o, r, i in s.render_sequence(orbit(start, 2, 1.0), seed=7, specular=0)]
    today = [(o.cpu().numpy(), r.cpu().numpy(), i) for o, r, i in s.render_sequence(orbit(start, 2, 1.0), seed=7)]
    for (o0, r0, i0), (o1, r1, i1) in zip(plain, today):
        assert np.array_equal(o0, o1) and np.array_equal(r0, r1)
        assert np.array_equal(i0["features_frame"].cpu().numpy(), i1["features_frame"].cpu().numpy())
    # frame 0 of the sequence, from its pieces
    out, raw, info = frames[0]
    guides = s.render_features_specular(4, 4, seed=7)
    assert np.array_equal(info["features_frame"].cpu().numpy(), guides)
    assert np.array_equal(raw, s.render(seed=7)[0])
    hist, signal, var = fray.temporal_accumulate(raw, guides, None, None, film_offset=info["film_offset"])
    assert np.array_equal(info["signal"].cpu().numpy(), signal) and np.array_equal(info["history"].cpu().numpy(), hist)
    assert np.array_equal(out, fray.denoise_signal(signal, var, guides))
    assert not np.array_equal(frames[1][0], plain[1][0])
    assert np.array_equal(frames[1][1], plain[1][1])                     # the frames themselves do not change
    with pytest.raises(ValueError, match="first hits only"):
        next(s.render_sequence(orbit(start, 2, 1.0), seed=7, specular=4, edit=lambda k, sc: None))
    with pytest.raises(ValueError, match="specular"):
        next(s.render_sequence(orbit(start, 2, 1.0), seed=7, specular=9))
    s.close()
