"""fray_amd/csrc/budget_search.hpp on the host: the 16-way search that frayhip_sample_map_budget's kernels replay from their control block -- the
stage of a budget, the candidates of a launch and the narrowing of the next -- against brute force, under AddressSanitizer and
UndefinedBehaviorSanitizer (a stand-alone program, tests/native/budget_search_check.cpp)."""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(__file__), "..")
SRC = os.path.join(ROOT, "tests", "native", "budget_search_check.cpp")
INC = "-I" + os.path.join(ROOT, "fray_amd", "csrc")


def _figures(out):
    line = [l for l in out.splitlines() if l.startswith("cases ")][-1]
    words = line.replace(",", " ").replace("(", " ").replace(")", " ").replace(":", " ").split()
    return {"cases": int(words[1]), "stage1": int(words[4]), "stage2": int(words[7]), "start": int(words[9]), "bad": int(words[11]),
            "launches": int(words[14]), "of": int(words[16])}


def test_the_fixed_launch_count_closes_every_interval(tmp_path):
    """Random non-increasing step functions over intervals of width 1, 2, K-1, K, K+1, K+2, 17^2, 17^2 + 1, 4096, 2^24 and 2^31 - 1, steps at both
    ends, capped sums of random planes for the cap, and the budgets that never reach the search: the replayed protocol ends at width 1 on the brute
    force's answer within eight launches, and the widest interval needs all eight."""
    exe = str(tmp_path / "budget_search_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    f = _figures(r.stdout)
    assert f["bad"] == 0 and f["stage1"] > 50000 and f["stage2"] > 20000 and f["start"] > 5000, r.stdout
    assert f["launches"] == f["of"] == 8, r.stdout


def test_seven_launches_would_not_be_enough(tmp_path):
    """the same harness with one launch fewer finds intervals left open: the check can fail, and eight is not slack"""
    exe = str(tmp_path / "budget_search_check7")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DFRAY_BUDGET_LAUNCHES=7", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, "50"], capture_output=True, text=True, timeout=600)
    f = _figures(r.stdout)
    assert r.returncode == 1 and f["bad"] > 100 and f["of"] == 7, r.stdout
