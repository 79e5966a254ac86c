"""bench.py --dump-outputs: what the last timed step computed, written as .npy files so that two builds can be compared output for output."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, run_in_clean_child

import bench


def test_dump_keeps_small_outputs_whole_and_as_float(tmp_path):
    ids = np.arange(6 * 8, dtype=np.int32).reshape(6, 8) - 3
    dist = np.linspace(0, 1, 48).reshape(6, 8)
    rgb = np.random.default_rng(1).random((6, 8, 3), dtype=np.float32)
    assert bench.dump_outputs(str(tmp_path), {"hit_id": ids, "hit_dist": dist, "frame": rgb}) == ["frame", "hit_dist", "hit_id"]
    got = {k: np.load(str(tmp_path / (k + ".npy"))) for k in ("hit_id", "hit_dist", "frame")}
    assert got["hit_id"].dtype == np.float64 and np.array_equal(got["hit_id"], ids)
    assert got["hit_dist"].dtype == np.float64 and np.array_equal(got["hit_dist"], dist)
    assert got["frame"].dtype == np.float32 and np.array_equal(got["frame"], rgb)


def test_dump_of_a_large_output_is_the_same_seeded_sample_under_the_limit(tmp_path):
    rgb = np.random.default_rng(2).random((300, 400, 3), dtype=np.float32)
    limit = 200000
    for run in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / run), {"frame": rgb}, limit=limit) == ["frame", "pixel_index"]
        assert sum(os.path.getsize(str(tmp_path / run / f)) for f in ("frame.npy", "pixel_index.npy")) <= limit
    a, b = np.load(str(tmp_path / "a" / "frame.npy")), np.load(str(tmp_path / "b" / "frame.npy"))
    idx = np.load(str(tmp_path / "a" / "pixel_index.npy"))
    assert np.array_equal(a, b) and np.array_equal(idx, np.load(str(tmp_path / "b" / "pixel_index.npy")))
    assert idx.dtype == np.float64 and len(idx) > 1000 and np.all(np.diff(idx) > 0)
    assert a.dtype == np.float32 and np.array_equal(a, rgb.reshape(-1, 3)[idx.astype(np.int64)])


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["boxed_primary", "csg_nested_pt16"])
def test_bench_dumps_the_last_timed_step(fray, gpu, tmp_path, workload):
    """The files hold the timed path's own result: the hit records / the exact-arithmetic frame, not the contracted frame bench.py renders
    into the same buffer afterwards."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "0", "--full", "--no-cpu-baseline", "--no-serial-pass",
           "--workload", workload, "--dump-outputs", str(tmp_path / "out")]
    out = run_in_clean_child(cmd, str(tmp_path / "bench.log"), timeout=600)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and "[exit code 0]" in out, out[-3000:]
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["ms_per_step"] > 0
    name, W, H, over, _ = bench.WORKLOADS[workload]
    s = bench.open_scene(fray, name, W, H, over)
    s.beginRender()
    if workload.endswith("_primary"):
        ids, dist, _ = s.primary_hits()
        assert sorted(os.listdir(str(tmp_path / "out"))) == ["hit_dist.npy", "hit_id.npy"]
        assert np.array_equal(np.load(str(tmp_path / "out" / "hit_id.npy")), ids)
        assert np.array_equal(np.load(str(tmp_path / "out" / "hit_dist.npy")), dist)
    else:
        assert "contracted" in r
        img, _ = s.render(seed=42)
        assert sorted(os.listdir(str(tmp_path / "out"))) == ["frame.npy"]
        assert np.array_equal(np.load(str(tmp_path / "out" / "frame.npy")), img)
    s.close()
