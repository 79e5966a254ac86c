"""The scenes of the specular feature frames' variant tests, built without a GPU: tests/test_specular_ref.py walks them with the CPU oracle and
establishes what tests/test_gpu_features_specular_variants.py relies on; that file uploads the same descriptions.  Not a test module."""
import os

import numpy as np

from conftest import ROOT, open_scene
from specular_ref import restated_shader
from test_fuzz_parity import random_scene

CORNELL_FLOOR = 0                            # cornell_box.fray's nodes in file order: floor, ceiling, backwall, rightwall, leftwall, shortblock, tallblock


def _plain(s, W, H):
    s.settings.frameWidth, s.settings.frameHeight = W, H
    s.settings.gi, s.settings.wantAA = 0, 0
    s.camera.dof, s.camera.stereoSeparation = 0, 0.0
    return s


def shader_of_kind(desc, kind, plain=True):
    """the first shader of this kind (plain: a Refl without gloss)"""
    return next(i for i in range(desc.n_shaders) if desc.shaders[i].kind == kind and not (plain and kind == 3 and desc.shaders[i].glossiness < 1))


def csg_nested(fray, tmp, W, H):
    """as it is: the mirror on node c, a scaled, rotated CsgMinus over a mesh, above the checker floor"""
    return _plain(fray.Scene.parseScene(os.path.join(ROOT, "tests", "scenes", "csg_nested.fray")), W, H)


def forest_mirror(fray, tmp, W, H):
    """forest.fray with its Phong mesh (the wine glass, a KD mesh) given the scene's Refl shader"""
    s = _plain(open_scene(fray, "forest.fray"), W, H)
    desc = s.desc
    mesh = next(i for i in range(desc.n_nodes) if desc.geoms[desc.nodes[i].geom].kind == 3 and desc.shaders[desc.nodes[i].shader].kind == 2)
    phong = desc.nodes[mesh].shader
    desc.nodes[mesh].shader = shader_of_kind(desc, 3)
    # the die: without its bump map (the walk applies none), and the Phong paint for its BitmapTexture'd Lambert, whose albedo the walk does not
    # restate -- every pixel of this frame is one the albedo rule knows
    die = next(i for i in range(desc.n_nodes) if desc.nodes[i].bump_tex >= 0)
    desc.nodes[die].bump_tex = -1
    assert not restated_shader(desc, desc.nodes[die].shader)
    desc.nodes[die].shader = phong
    return s


def forest_bumped(fray, tmp, W, H, bump=True):
    """forest.fray in Const paint for the comparison with the Whitted frame: the teapot (vertex normals and uvs) the plain mirror under the die's bump
    map, every Lambert / Phong record a Const of a colour of its own, Layered and glossy nodes repointed to one of those, no glass on a node."""
    s = _plain(open_scene(fray, "forest.fray"), W, H)
    s.settings.maxTraceDepth = 12
    desc = s.desc
    smooth_uv = lambda i: (lambda g: g.kind == 3 and desc.meshes[g.index].n_normals > 0 and desc.meshes[g.index].n_uvs > 0
                           and not desc.meshes[g.index].faceted)(desc.geoms[desc.nodes[i].geom])
    checkered = lambda i: (lambda sh: sh.kind == 1 and sh.texture >= 0 and desc.textures[sh.texture].kind == 0)(desc.shaders[desc.nodes[i].shader])
    teapot = next(i for i in range(desc.n_nodes) if smooth_uv(i) and checkered(i))           # the only mesh node in checker paint
    paint = [i for i in range(desc.n_shaders) if desc.shaders[i].kind in (1, 2)]
    for k, i in enumerate(paint):
        sh = desc.shaders[i]
        sh.kind, sh.texture = 0, -1
        sh.color[0], sh.color[1], sh.color[2] = 0.15 + 0.11 * k, 0.9 - 0.13 * k, 0.25 + 0.3 * (k % 3)
    assert len({tuple(desc.shaders[i].color[:]) for i in paint}) == len(paint) >= 3
    die_bump = next(desc.nodes[i].bump_tex for i in range(desc.n_nodes) if desc.nodes[i].bump_tex >= 0)
    for i in range(desc.n_nodes):
        sh = desc.shaders[desc.nodes[i].shader]
        if i == teapot:
            desc.nodes[i].shader = shader_of_kind(desc, 3)
            desc.nodes[i].bump_tex = die_bump if bump else -1
        elif sh.kind not in (0, 3) or (sh.kind == 3 and sh.glossiness < 1):
            desc.nodes[i].shader = paint[i % len(paint)]
    assert not any(desc.shaders[desc.nodes[i].shader].kind == 4 for i in range(desc.n_nodes))
    return s, teapot


def cornell_floor_mirror(fray, tmp, W, H):
    """cornell_box with its floor the mirror, seen from inside the box looking down at it: the ceiling's rect light is a terminal behind a chain
    (from the scene's own camera, 800 in front of the box, every ray off the floor reaches the back wall before it has climbed to the ceiling)"""
    s = _plain(open_scene(fray, "cornell_box.fray"), W, H)
    desc = s.desc
    assert desc.shaders[desc.nodes[CORNELL_FLOOR].shader].kind == 1
    desc.nodes[CORNELL_FLOOR].shader = shader_of_kind(desc, 3)
    s.camera.pos[0], s.camera.pos[1], s.camera.pos[2] = 278.0, 450.0, 150.0
    s.camera.pitch = -70.0
    return s


def generated(flavour, seed):
    def build(fray, tmp, W, H):
        """tests/test_fuzz_parity.random_scene, Whitted, no lens, stereo or bump; every node whose shader the walk's albedo rule does not restate
        (painted, coat, wet) or that is glossy (rough) repointed to the scene's grey Lambert.  W, H None: the generated size."""
        s = fray.Scene.parseScene(random_scene(np.random.default_rng(1000 + seed), tmp, 0, flavour=flavour))
        s = _plain(s, W or s.settings.frameWidth, H or s.settings.frameHeight)
        desc = s.desc
        grey = next(i for i in range(desc.n_shaders) if desc.shaders[i].kind == 1 and desc.shaders[i].texture < 0)
        assert [round(c, 3) for c in desc.shaders[grey].color[:]] == [0.6, 0.6, 0.6]
        for i in range(desc.n_nodes):
            desc.nodes[i].bump_tex = -1
            sh = desc.shaders[desc.nodes[i].shader]
            if not restated_shader(desc, desc.nodes[i].shader) or (sh.kind == 3 and sh.glossiness < 1):
                desc.nodes[i].shader = grey
        return s
    return build


# name -> (builder, frame size on the GPU (None: the generated one), the even flag word, the terminals claimed behind a chain)
# random_scene's flavour -> the seeds (of default_rng(1000 + seed)) in whose scenes a `mir` and a `glass` node are both seen by the camera
GENERATED_SEEDS = {0: (4, 11), 1: (4, 6), 2: (5, 11)}
CSG_GI_SIZE, CSG_GI_SEED = (48, 36), 9       # the path-traced csg_nested frame of the sample-loop test
BUMP_SIZE = (96, 72)                         # the bumped forest's frame
CASES = {
    "csg_nested": (csg_nested, (96, 72), 2, ("checker",)),
    "forest_mirror": (forest_mirror, (96, 72), 4, ("environment",)),
    "cornell_floor_mirror": (cornell_floor_mirror, (96, 72), 0, ("light",)),
}
for _flavour, _seeds in GENERATED_SEEDS.items():
    for _seed in _seeds:
        CASES["generated_f%d_s%d" % (_flavour, _seed)] = (generated(_flavour, _seed), None, (2, 4, 8)[_flavour], ("mir", "glass"))


def terminals(desc, ch):
    """which of the claimed terminals occur behind a chain in walk ch (flat or shaped): masks by name; "checker_paint": a terminal in checker paint,
    behind a chain or not"""
    b, t = ch["b"], ch["t_id"]
    node = np.where(t >= 0, t, 0)
    sh = np.array([desc.nodes[i].shader for i in range(desc.n_nodes)])[node]
    checker = np.array([desc.shaders[i].kind in (1, 2) and desc.shaders[i].texture >= 0 and desc.textures[desc.shaders[i].texture].kind == 0
                        for i in range(desc.n_shaders)])[sh]
    return {"checker": (b > 0) & (t >= 0) & checker, "checker_paint": (t >= 0) & checker, "environment": (b > 0) & (t == -1), "light": (b > 0) & (t <= -2)}
