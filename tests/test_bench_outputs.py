"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files so that two builds can
be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_samples_are_fixed():
    assert bench.dump_sample(100, 100, 0) is None
    a, b = bench.dump_sample(10_000, 500, 1), bench.dump_sample(10_000, 500, 1)
    assert np.array_equal(a, b) and len(np.unique(a)) == 500 and np.all(np.diff(a) > 0) and a.max() < 10_000
    assert not np.array_equal(a, bench.dump_sample(10_000, 500, 2))
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d" and bench.parse_args([]).dump_outputs is None


def test_dumped_maps_are_finite_and_keep_where_they_had_no_value():
    a = np.array([[1.5, -np.inf], [np.nan, -0.25]], dtype=np.float32)
    v, ok = bench.dump_finite(a)
    assert v.dtype == np.float32 and ok.dtype == np.float32 and np.isfinite(v).all()
    assert np.array_equal(ok, [[1, 0], [0, 1]]) and np.array_equal(v, [[1.5, 0], [0, -0.25]])


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--no-cpu-baseline",
                        "--no-extra-legs", "--preroll-seconds", "0", "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and abs(res["value"] * res["ms_per_step"] * 1e-3 - 1.0) < 1e-3
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    maps = ("raycast_depth", "raycast_depth4", "raycast_normals", "raycast_colors")
    assert set(got) == set(maps) | {m + "_valid" for m in maps} | {"scene_counts", "scene_block_positions", "scene_voxel_block_positions",
                                                                  "scene_voxel_sdf", "scene_voxel_weight", "scene_voxel_color"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64_000_000
    # cfg2: 640x480, every map whole; frame 4 rendered from pose 3 sees the spheres, and the background holds no value
    assert got["raycast_depth"].shape == (480, 640) and got["raycast_colors"].shape == (480, 640, 4)
    for m in maps:
        ok = got[m + "_valid"]
        assert ok.shape == got[m].shape and set(np.unique(ok)) <= {0.0, 1.0} and not got[m][ok == 0].any()
    hit = got["raycast_depth_valid"] == 1
    assert 1000 < hit.sum() < hit.size and np.all(got["raycast_depth"][hit] > 0)
    n = int(got["scene_counts"][0])
    pos = got["scene_block_positions"]
    assert n > 100 and pos.shape == (n, 3) and np.all(np.lexsort(pos.T[::-1]) == np.arange(n))
    k = min(n, bench.DUMP_VOXEL_BLOCKS)
    assert got["scene_voxel_block_positions"].shape == (k, 3) and got["scene_voxel_sdf"].shape == (k, 512)
    assert got["scene_voxel_color"].shape == (k, 512, 3) and got["scene_voxel_weight"].max() > 0
