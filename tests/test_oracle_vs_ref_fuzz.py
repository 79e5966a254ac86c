"""Scenes nobody hand-picked, through the reference's object code: tests/test_fuzz_parity.py's random scenes (every geometry kind under random transforms,
KD and tree-less meshes, CsgOps three levels deep, all shaders, bitmap / bump / Fresnel textures, thin lens, stereo) are written to a scratch folder,
rendered and probed by oracle/_ref -- the reference's OWN parser, OBJ / BMP loaders, KD builder, geometry, lights, camera, shaders -- and by the oracle, which
is fed by the PRODUCT's parser and KD builder.  Probe records and pictures must be equal bit for bit, for both integrators on every scene.  (The fixed
fixtures of tests/test_oracle_vs_ref.py are scenes somebody chose; eight of these generated ones are committed as ref_fuzz*.npz for the GPU suite.)
The reference's probe records and pictures of the seeds below are stored in tests/golden/generated/ (each with a digest of the scene files it was
made from), so the comparison runs wherever the repository does; `python tests/test_oracle_vs_ref_fuzz.py` writes them again from oracle/_ref.
FRAY_REF_FUZZ_SEEDS=50 runs the long form: the seeds beyond the stored ones go through oracle/_ref live and are skipped where it is not built."""
import hashlib
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_fuzz_parity import random_scene

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libfray_ref.so")
STORED = os.path.join(ROOT, "tests", "golden", "generated")
SEEDS, FAN_SEEDS = range(3000, 3012), (3200, 3201, 3202)          # the stored ones
N = int(os.environ.get("FRAY_REF_FUZZ_SEEDS", str(len(SEEDS))))


def scene_digest(folder):
    """SHA-1 over the names and bytes of the files random_scene wrote: ties a stored fixture to the scene it was made from."""
    h = hashlib.sha1()
    for f in sorted(os.listdir(str(folder))):
        h.update(f.encode())
        h.update(open(os.path.join(str(folder), f), "rb").read())
    return h.hexdigest()


def ref_fixture(scene_path, name, W, H, over, outdir, digest):
    """The reference's probe records and picture of a generated scene: stored for the seeds above, else made now by oracle/_ref."""
    stored = os.path.join(STORED, name + ".npz")
    if os.path.exists(stored):
        z = np.load(stored)
        assert str(z["scene_sha1"]) == digest, "%s was made from another scene: random_scene changed (regenerate the stored fixtures)" % stored
        return z
    if not os.path.exists(REF_SO):
        pytest.skip("no stored fixture for %s, and oracle/_ref is only built where the reference tree is mounted" % name)
    return ref_fixture_now(scene_path, name, W, H, over, outdir)


def ref_fixture_now(scene_path, name, W, H, over, outdir):
    env = dict(os.environ, GOLDEN_OUT=str(outdir))
    env.pop("FRAY_REF_FACES_DIR", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "make_golden.py"), name, scene_path, str(W), str(H), over, "3", "120"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(os.path.join(outdir, "ref_%s.npz" % name))


def compare(fray, abi, oracle, z, scene_path, gi):
    s = fray.Scene.parseScene(scene_path)
    s.settings.gi = gi
    assert (s.settings.frameWidth, s.settings.frameHeight) == (int(z["W"]), int(z["H"]))
    S, D = z["ray_start"], z["ray_dir"]
    for i in range(len(S)):
        out = np.zeros(9)
        a, b = np.ascontiguousarray(S[i]), np.ascontiguousarray(D[i])
        hid = oracle.lib.fray_oracle_probe(s.desc, a.ctypes.data, b.ctypes.data, out.ctypes.data)
        assert hid == z["hit_id"][i], (i, hid, z["hit_id"][i])
        want = z["hit_rec"][i]
        if hid == -1:
            assert out[0] == want[0] == 1e99
        elif hid <= -2:
            assert np.array_equal(out[:7], want[:7])
        else:
            assert np.array_equal(out, want), (i, out, want)
    img, _ = oracle.render(s.desc, abi.MODE_RENDER, seed=42, threads=4)
    ref = z["image"]
    assert ref.shape == img.shape and np.isfinite(ref).all()
    assert np.array_equal(img, ref), "gi %d: max abs diff %g over %d pixels" % (gi, np.abs(img - ref).max(), int((img != ref).any(axis=2).sum()))
    s.close()


@pytest.mark.parametrize("seed", range(3000, 3000 + N))
def test_generated_scene_through_reference_object_code_and_oracle(fray, abi, oracle, tmp_path, seed):
    rng = np.random.default_rng(seed)
    gi = seed % 2
    scene = random_scene(rng, pathlib.Path(tmp_path), gi, flavour=seed % 3, bump_on=("blob",))      # bump maps on meshes only: elsewhere the reference reads uninitialised memory
    digest = scene_digest(tmp_path)
    s = fray.Scene.parseScene(scene)
    W, H = s.settings.frameWidth, s.settings.frameHeight
    s.close()
    for g in (gi, 1 - gi):
        z = ref_fixture(scene, "fz%d_%d" % (seed, g), W, H, "gi=%d" % g, tmp_path, digest)
        compare(fray, abi, oracle, z, scene, g)


@pytest.mark.parametrize("seed", FAN_SEEDS)
def test_generated_glossy_fan_scene_through_reference_object_code_and_oracle(fray, abi, oracle, tmp_path, seed):
    """The scenes the device's speculative glossy fans apply to (point lights only, fans of 8-13 samples: tests/test_fuzz_parity.py): here the oracle they
    are compared with is itself compared with the reference's object code."""
    rng = np.random.default_rng(seed)
    scene = random_scene(rng, pathlib.Path(tmp_path), 0, flavour=seed % 3, bump_on=("blob",), fans=True)
    digest = scene_digest(tmp_path)
    s = fray.Scene.parseScene(scene)
    W, H = s.settings.frameWidth, s.settings.frameHeight
    s.close()
    z = ref_fixture(scene, "fans%d" % seed, W, H, "gi=0", tmp_path, digest)
    compare(fray, abi, oracle, z, scene, 0)


def write_stored_fixtures():
    """Makes tests/golden/generated/ again from oracle/_ref (`make ref`): the scenes of SEEDS and FAN_SEEDS as the tests above generate them."""
    import tempfile
    sys.path.insert(0, ROOT)
    os.environ.setdefault("FRAYHIP_NO_TORCH", "1")
    import fray_amd
    assert os.path.exists(REF_SO), "oracle/_ref is not built"
    os.makedirs(STORED, exist_ok=True)
    jobs = [(seed, seed % 2, False, (seed % 2, 1 - seed % 2)) for seed in SEEDS] + [(seed, 0, True, (0,)) for seed in FAN_SEEDS]
    for seed, gi, fans, gis in jobs:
        with tempfile.TemporaryDirectory() as tmp:
            folder = pathlib.Path(tmp) / "scene"
            folder.mkdir()
            scene = random_scene(np.random.default_rng(seed), folder, gi, flavour=seed % 3, bump_on=("blob",), fans=fans)
            digest = scene_digest(folder)
            s = fray_amd.Scene.parseScene(scene)
            W, H = s.settings.frameWidth, s.settings.frameHeight
            s.close()
            for g in gis:
                name = "fans%d" % seed if fans else "fz%d_%d" % (seed, g)
                z = dict(ref_fixture_now(scene, name, W, H, "gi=%d" % g, tmp))
                del z["scene"]                       # a scratch path
                np.savez_compressed(os.path.join(STORED, name + ".npz"), scene_sha1=digest, **z)
                print(name, W, H, "rays", len(z["ray_start"]), flush=True)


if __name__ == "__main__":
    write_stored_fixtures()
