"""The edit cases of frayhip_scene_update's tests (tests/test_scene_update_host.py on the CPU, tests/test_gpu_scene_update.py on the GPU).  Not a test module.

An edit is a list of tokens in the language of tests/native/arena_update_check.cpp ("node 6 translate 30 0 5", ...): the harness applies it in C++
through the C helpers, apply() below applies the same tokens to a fray_amd.Scene through the Python wrappers.  A case also says how the scene FILE
changes -- other scale / rotate / translate lines, shader names, light properties -- so that the CPU test can parse the edited scene afresh."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")


# ---- scene text -----------------------------------------------------------------------------------------------------------------------------
def block_span(text, header):
    """(start of the body, end of the body) of the block whose header line is `header` ("Node tallblock", "RectLight", ...)"""
    m = re.search(r"^%s\s*\{" % re.escape(header).replace(r"\ ", r"\s+"), text, flags=re.M)
    assert m, header
    return m.end(), text.index("}", m.end())


def set_block(text, header, drop=(), add=()):
    """The block's property lines named in `drop` removed and the lines of `add` appended, in order."""
    a, b = block_span(text, header)
    body = [ln for ln in text[a:b].split("\n") if not (ln.split() and ln.split()[0] in drop)]
    return text[:a] + "\n".join(body) + "\n" + "".join("\t%s\n" % ln for ln in add) + text[b:]


def rename_block(text, header, new_header):
    m = re.search(r"^%s(\s*\{)" % re.escape(header).replace(r"\ ", r"\s+"), text, flags=re.M)
    assert m, header
    return text[:m.start()] + new_header + m.group(1) + text[m.end():]


def relocate_files(text, scene_dir, new_dir):
    """`file "x"` properties (relative to the scene file's directory) rewritten for a copy of the text that lies in new_dir."""
    return re.sub(r'^(\s*file\s+)"?([^"\n]+?)"?\s*$',
                  lambda m: '%s"%s"' % (m.group(1), os.path.relpath(os.path.join(scene_dir, m.group(2)), new_dir)), text, flags=re.M)


def strip_comments(text):
    return re.sub(r"//[^\n]*", "", text)


def file_transforms(text):
    """The scene file's own numbers: for every node with a shader (the description's nodes[], in file order) and every light, the edit tokens that
    rebuild its transform from the block's scale / rotate / translate lines, in their order."""
    tokens = []
    node = light = 0
    for m in re.finditer(r"^\s*(\w+)(?:[ \t]+(\w+))?\s*\{([^}]*)\}", strip_comments(text), flags=re.M):
        cls, body = m.group(1), m.group(3)
        props = [ln.split(None, 1) for ln in body.split("\n") if ln.split()]
        if cls == "Node":
            if not any(p[0] == "shader" for p in props):
                continue
            what, i = "node", node
            node += 1
        elif cls in ("RectLight", "PointLight"):
            what, i = "light", light
            light += 1
            if cls == "PointLight":
                continue
        else:
            continue
        tokens += [what, str(i), "reset"]
        for p in props:
            if p[0] in ("scale", "rotate", "translate"):
                tokens += [what, str(i), p[0]] + re.sub(r"[(),]", " ", p[1]).split()[:3]
    return tokens


GLOSSY = """GlobalSettings {
	frameWidth 64
	frameHeight 48
	ambientLight (0.1, 0.1, 0.1)
	maxTraceDepth 3
	wantAA off
}
Camera camera {
	position (0, 6, -18)
	pitch -12
	fov 60
}
PointLight p0 {
	pos (-8, 14, -6)
	color (1, 0.9, 0.8)
	power 600
}
PointLight p1 {
	pos (9, 12, -4)
	color (0.8, 0.9, 1)
	power 400
}
Plane ground {
	y 0
	limit 60
}
Sphere ball {
	O (0, 3, 0)
	R 3
}
Lambert grey {
	color (0.6, 0.6, 0.55)
}
Refl glossy {
	multiplier 0.85
	glossiness 0.75
	numSamples 16
}
Node floorNode {
	geometry ground
	shader glossy
}
Node ballNode {
	geometry ball
	shader grey
}
"""


def write_glossy(path):
    with open(path, "w") as f:
        f.write(GLOSSY)
    return str(path)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
# name -> dict(scene: path under scenes/, tests/scenes/ or "glossy" (generated), text: file text -> edited text, edit / undo: tokens)
def _t(s):
    return s.split()


CASES = {
    # the tall block leaves its place: its gate is no longer the mesh's own box, so no gate is a proof any more
    "cornell-block": dict(scene="cornell_box.fray", text=lambda t: set_block(t, "Node tallblock", add=["translate (30, 0, 5)"]),
                          edit=_t("node 6 reset node 6 translate 30 0 5"), undo=_t("node 6 reset")),
    # a wall moves: it is no longer untransformed, so its planes leave the segment-plane tables
    "cornell-wall": dict(scene="cornell_box.fray", text=lambda t: set_block(t, "Node rightwall", add=["translate (-12, 0, 0)"]),
                         edit=_t("node 3 reset node 3 translate -12 0 0"), undo=_t("node 3 reset")),
    # the only recursive shader goes: shaders[] is white 0, green 1, red 2, mirror 3
    "cornell-shader": dict(scene="cornell_box.fray", text=lambda t: set_block(t, "Node shortblock", drop=["shader"], add=["shader white"]),
                           edit=_t("node 5 shader 0"), undo=_t("node 5 shader 3")),
    "cornell-light": dict(scene="cornell_box.fray",
                          text=lambda t: set_block(t, "RectLight", drop=["scale", "translate", "xSubd", "ySubd"],
                                                   add=["scale (100, 1, 120)", "translate (250, 540, 279.5)", "xSubd 2", "ySubd 2"]),
                          edit=_t("light 0 subd 2 2 light 0 reset light 0 scale 100 1 120 light 0 translate 250 540 279.5"),
                          undo=_t("light 0 subd 4 4 light 0 reset light 0 scale 130 1 105 light 0 translate 278 547.7 279.5")),
    # spheres[]: ball 0, small 1, tiny 2; cubes[]: c0 0, c1 1, box 2; node 1 is `a` (CsgMinus hollow = (box & ball) - small)
    "csg-nested": dict(scene="../tests/scenes/csg_nested.fray",
                       text=lambda t: set_block(set_block(set_block(t, "Node a", drop=["translate", "rotate"], add=["translate (-5, 3, 1)", "rotate (40, 10, 0)"]),
                                                          "Sphere small", drop=["R"], add=["R 1.9"]), "Cube box", drop=["halfSide"], add=["halfSide 2.5"]),
                       edit=_t("node 1 reset node 1 translate -5 3 1 node 1 rotate 40 10 0 sphere 1 R 1.9 cube 2 half 2.5"),
                       undo=_t("node 1 reset node 1 translate -6 2.5 0 node 1 rotate 30 20 0 sphere 1 R 1.6 cube 2 half 2")),
    # textures[]: diceBump 0, checker 1, diceTexture 2; node 6 is zarche (the bumped dice), node 7 teapotNode (a KD mesh)
    "boxed-textured": dict(scene="boxed.fray",
                           text=lambda t: set_block(set_block(set_block(t, "CheckerTexture checker", drop=["color1", "color2", "scaling"],
                                                                        add=["color1 (0.25, 0.5, 0.75)", "color2 (0.5, 0.125, 0.25)", "scaling 1.5"]),
                                                              "Node zarche", drop=["bump"]),
                                                    "Node teapotNode", drop=["rotate"], add=["rotate (45, 10, 0)"]),
                           edit=_t("tex 1 color1 0.25 0.5 0.75 tex 1 color2 0.5 0.125 0.25 tex 1 scaling 1.5 node 6 bump -1 "
                                   "node 7 reset node 7 translate 0 16 0 node 7 scale 7.5 7.5 7.5 node 7 rotate 45 10 0"),
                           undo=None),
    # one glossy Refl under point lights only: its fan of 16 may be drawn ahead, a fan of 4 may not
    "glossy-fan": dict(scene="glossy", text=lambda t: set_block(t, "Refl glossy", drop=["numSamples", "glossiness"], add=["glossiness 0.5", "numSamples 4"]),
                       edit=_t("shader 1 numSamples 4 shader 1 glossiness 0.5"), undo=_t("shader 1 numSamples 16 shader 1 glossiness 0.75")),
    # a point light becomes a rect light: now a light draws random numbers
    "glossy-rect": dict(scene="glossy",
                        text=lambda t: set_block(rename_block(t, "PointLight p1", "RectLight p1"), "RectLight p1", drop=["pos"],
                                                 add=["translate (9, 12, -4)", "scale (3, 1, 3)", "xSubd 2", "ySubd 2"]),
                        edit=_t("light 1 kind 1 light 1 pos 0 0 0 light 1 subd 2 2 light 1 reset light 1 translate 9 12 -4 light 1 scale 3 1 3"),
                        undo=_t("light 1 kind 0 light 1 pos 9 12 -4 light 1 subd 1 1 light 1 reset")),
}


def scene_path(case, tmp_dir):
    """The case's original scene file (the generated one is written into tmp_dir)."""
    if case["scene"] == "glossy":
        return write_glossy(os.path.join(str(tmp_dir), "glossy.fray"))
    return os.path.normpath(os.path.join(SCENES, case["scene"]))


def edited_text(case, original_path, new_dir):
    """The case's scene as edited text, to be written into new_dir."""
    with open(original_path) as f:
        text = f.read()
    return relocate_files(case["text"](text), os.path.dirname(original_path), str(new_dir))


# ---- the same tokens on a fray_amd.Scene ------------------------------------------------------------------------------------------------------
def apply(fray, s, tokens):
    """Applies edit tokens to s.desc through Scene's table views, fray_amd.Transform and the begin_frame wrappers (no update())."""
    p = list(tokens)
    num = lambda: float(p.pop(0))
    while p:
        what, i, op = p.pop(0), int(p.pop(0)), p.pop(0)
        if what in ("node", "light"):
            rec = (s.nodes if what == "node" else s.lights)[i]
            if op == "reset":
                fray.Transform().store(rec)
            elif op in ("scale", "rotate", "translate"):
                getattr(fray.Transform(rec), op)(num(), num(), num()).store(rec)
            elif op == "shader":
                rec.shader = int(num())
            elif op == "bump":
                rec.bump_tex = int(num())
            elif op == "geom":
                rec.geom = int(num())
            elif op == "subd":
                rec.xSubd, rec.ySubd = int(num()), int(num())
            elif op == "kind":
                rec.kind = int(num())
            elif op == "pos":
                rec.pos[0], rec.pos[1], rec.pos[2] = num(), num(), num()
            else:
                raise ValueError(op)
        elif what == "sphere" and op == "R":
            s.spheres[i].R = num()
        elif what == "cube" and op == "half":
            s.cubes[i].halfSide = num()
        elif what == "tex" and op in ("color1", "color2"):
            c = getattr(s.textures[i], op)
            c[0], c[1], c[2] = num(), num(), num()
        elif what == "tex" and op == "scaling":
            s.textures[i].scaling = num()
        elif what == "shader" and op == "numSamples":
            s.shaders[i].numSamples = int(num())
        elif what == "shader" and op == "glossiness":
            s.shaders[i].glossiness = num()
        else:
            raise ValueError("%s %s" % (what, op))
    for L in s.lights:
        fray.light_begin_frame(L)
    for sh in s.shaders:
        fray.shader_begin_frame(sh)
    return s
