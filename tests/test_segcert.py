"""fray_amd/csrc/dev_segcert.hpp on the host: the certificate that lets k_pt_shadow skip a small untransformed mesh whose triangles' planes a next-event
segment does not cross (option "segment_planes")."""
import os
import subprocess


def test_a_certified_segment_is_never_occluded_by_its_triangle(tmp_path):
    """tests/native/segcert_check.cpp runs the certificate against visible() restated from the reference for one triangle (the segment's ray, the second
    normalisation of Node::intersect, Triangle::intersectFast, the hit point, `info.dist < maxDist`) and against the fp_contract copy of the device code
    (fused products, the ray parameter as the distance): random segments, ends at offsets around the margin on either side of the plane, segments nearly
    parallel to it (|Dcr| 1e-20 .. 1e-6), coplanar disjoint triangles, segments ending just short of and just beyond the triangle, coordinates scaled by
    1e-3, 1 and 1e4, directions with exact zeros, degenerate lengths.  No certified segment is ever reported occluded; a substantial share of the cases
    is certified; built with the margin set to zero the same harness finds contradictions, so it does see them."""
    root = os.path.join(os.path.dirname(__file__), "..")
    src, inc = os.path.join(root, "tests", "native", "segcert_check.cpp"), "-I" + os.path.join(root, "fray_amd", "csrc")
    exe = str(tmp_path / "segcert_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", inc, src, "-o", exe], check=True)
    r = subprocess.run([exe, "6000000"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "contradictions 0" in r.stdout, r.stdout + r.stderr
    cases = int(r.stdout.split("cases")[1].split(",")[0])
    certified = int(r.stdout.split("certified")[1].split()[0])
    assert cases > 5000000 and certified > 0.3 * cases, r.stdout          # the harness must actually certify: a third of what it runs
    per_mode = r.stdout.split("certified per mode:")[1].split("\n")[0].split()
    counts = [int(per_mode[2 * k + 1].split("/")[0]) for k in range(9)]
    assert all(c > 0 for c in counts), r.stdout                           # ... in every kind of segment (even "just beyond": chords that end beside the triangle)
    exe0 = str(tmp_path / "segcert_check0")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DFRAY_SEGCERT_SCALE=0", inc, src, "-o", exe0], check=True)
    r0 = subprocess.run([exe0, "1000000"], capture_output=True, text=True, timeout=600)
    print(r0.stdout)
    assert r0.returncode == 1 and int(r0.stdout.split("contradictions")[1].split()[0]) > 100, r0.stdout
