"""fray_amd/csrc/dev_gatecert.hpp on the host: the certificate that lets the path tracer's producers test a gated mesh by the box of its own triangles
(frayhip_scene_tight_gates) -- no triangle of the mesh accepts a certified ray, as the reference's arithmetic and the fp_contract copy compute it."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(__file__), "..")
SRC = os.path.join(ROOT, "tests", "native", "gatecert_check.cpp")
INC = "-I" + os.path.join(ROOT, "fray_amd", "csrc")
MODES = 9
NONFINITE = 7          # the mode of the rays with a NaN or an infinity: never certified


def _per_mode(out, title):
    words = out.split(title)[1].split("\n")[0].split()
    return [int(words[2 * k + 1].split("/")[0]) for k in range(MODES)]


def test_a_certified_ray_has_no_triangle_of_the_mesh_accepted(tmp_path):
    """tests/native/gatecert_check.cpp runs the certificate against the mesh loop and the triangle test restated from the reference, and against the
    fp_contract copy of the device code: the two Cornell blocks, rotated and scaled boxes, an L-shaped prism, a box around the origin; random rays, rays
    aimed at edges and corners at distances around the margin, directions 1e-13 .. 1e-2 off parallel to a face (both sides of the guard threshold), far
    starts, starts on the faces, axis-parallel directions, unnormalised segments, the Cornell situation, NaN and infinity.  No certified ray has a
    triangle accepted; a mesh with a sliver, with seven normal directions, with a NaN, with a wrong stored normal or at 1e8 gets no record; every kind of
    ray is certified sometimes and the guard does send rays back; built without the margins and the guard the same harness finds contradictions, some
    of them among the nearly parallel rays."""
    exe = str(tmp_path / "gatecert_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "6000000"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "contradictions 0" in r.stdout, r.stdout + r.stderr
    assert "refused wrongly 0, admitted wrongly 0, non-finite rays certified 0" in r.stdout, r.stdout
    cases = int(r.stdout.split("cases")[1].split(",")[0])
    certified = int(r.stdout.split("certified")[1].split()[0])
    assert cases > 5000000 and certified > 0.2 * cases, r.stdout
    counts = _per_mode(r.stdout, "certified per mode:")
    assert all(c > 0 for k, c in enumerate(counts) if k != NONFINITE) and counts[NONFINITE] == 0, r.stdout
    sent_back = int(r.stdout.split("the guard sent back")[1].split(";")[0])
    assert sent_back > 1000, r.stdout
    exe0 = str(tmp_path / "gatecert_check0")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DFRAY_GATECERT_SCALE=0", "-DFRAY_MISSCERT_SCALE=0", INC, SRC, "-o", exe0], check=True)
    r0 = subprocess.run([exe0, "1000000"], capture_output=True, text=True, timeout=600)
    print(r0.stdout)
    words = r0.stdout.split("contradictions per mode:")[1].split("\n")[0].split()
    bad = [int(words[2 * k + 1]) for k in range(MODES)]
    assert r0.returncode == 1 and sum(bad) > 100 and bad[2] > 0, r0.stdout          # mode 2: the nearly parallel rays


def test_the_harness_is_clean_under_the_sanitizers(tmp_path):
    """the same program built with AddressSanitizer and UndefinedBehaviorSanitizer, a shorter run"""
    exe = str(tmp_path / "gatecert_check_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "300000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "contradictions 0" in r.stdout, r.stdout + r.stderr
