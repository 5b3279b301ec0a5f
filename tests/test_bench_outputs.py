"""`bench.py --dump-outputs DIR`: the last timed step's outputs as DIR/<name>.npy, identical from run to run with the same arguments,
at most 64 MB in all (a fixed seeded sample of rows above that); a plain run prints the headline fields only, `--full` adds the rest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _arrays(n):
    rng = np.random.default_rng(3)
    return {"obs": rng.standard_normal((n, 29)).astype(np.float32), "reward": rng.standard_normal(n).astype(np.float32)}


def _read(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_array_whole_under_the_limit(tmp_path):
    a = _arrays(1000)
    bench.dump_outputs(a, str(tmp_path))
    got = _read(str(tmp_path))
    assert sorted(got) == ["obs.npy", "reward.npy"]
    assert all(np.array_equal(got[k + ".npy"], v) and got[k + ".npy"].dtype == np.float32 for k, v in a.items())


def test_dump_samples_the_same_rows_above_the_limit(tmp_path):
    a, limit = _arrays(50_000), 1 << 20
    bench.dump_outputs(a, str(tmp_path / "1"), limit_bytes=limit)
    bench.dump_outputs(a, str(tmp_path / "2"), limit_bytes=limit)
    one, two = _read(str(tmp_path / "1")), _read(str(tmp_path / "2"))
    assert sorted(one) == ["obs.npy", "obs_rows.npy", "reward.npy", "reward_rows.npy"]
    assert sum(os.path.getsize(os.path.join(tmp_path, "1", f)) for f in one) <= limit
    assert all(np.array_equal(one[f], two[f]) for f in one)
    for k, v in a.items():
        rows = one[k + "_rows.npy"]
        assert rows.dtype == np.float64 and len(rows) > 0 and np.all(np.diff(rows) > 0)
        assert np.array_equal(one[k + ".npy"], v[rows.astype(np.int64)])


def test_step_outputs_are_float32_host_copies_with_final_observation_only_where_done():
    import torch

    n = 6
    done = torch.tensor([0, 1, 0, 2, 0, 3], dtype=torch.uint8)
    final = torch.full((n, 3), float("nan"))
    final[done != 0] = 7.0
    info = torch.arange(n * 4, dtype=torch.float32).reshape(n, 4)
    result = (torch.ones((n, 3)), torch.zeros(n), done, {"position": info[:, :2], "goal_index": torch.arange(n, dtype=torch.int32),
                                                        "final_observation": final})
    got = bench.step_outputs(result)
    assert sorted(got) == ["done", "final_observation", "goal_index", "obs", "position", "reward"]
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["done"], [0, 1, 0, 2, 0, 3]) and np.array_equal(got["position"], info[:, :2].numpy())
    want = np.zeros((n, 3), np.float32)
    want[(done != 0).numpy()] = 7.0  # the NaN rows (done == 0) hold nothing the caller may read
    assert np.array_equal(got["final_observation"], want)


def _run(*extra):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MZ_BENCH_SINGLE_GPU"):
        e.pop(k, None)
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "6", "--warmup", "2", "--settle", "10", "--envs", "512", *extra],
                         capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    lines = [_run("--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for d in lines:
        assert d["steps"] == 6 and d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
        assert d["unit"] == "env-steps/s" and d["dtype"] == "f32" and d["metric"].endswith("AntUMaze-v0, 512 envs/GPU")
        assert not {"roofline", "roofline_valu", "sustained", "cpu_baseline", "without_allgather"} & set(d)
    a, b = _read(str(tmp_path / "a")), _read(str(tmp_path / "b"))
    assert {"obs.npy", "reward.npy", "done.npy", "final_observation.npy"} <= set(a) and sorted(a) == sorted(b)
    assert a["obs.npy"].shape[0] == 512 and all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[f], b[f]) for f in a)
    assert np.isfinite(a["obs.npy"]).all()


@pytest.mark.gpu
def test_full_run_adds_the_other_figures_and_computes_the_same_outputs(tmp_path):
    plain = _run("--dump-outputs", str(tmp_path / "plain"))
    full = _run("--full", "--no-cpu-baseline", "--no-live-pmc", "--sustained", "4", "--dump-outputs", str(tmp_path / "full"))
    assert full["roofline"]["kernel_ms"] > 0 and full["sustained"]["steps"] == 4
    assert {k: plain[k] for k in ("metric", "unit", "dtype", "steps")} == {k: full[k] for k in ("metric", "unit", "dtype", "steps")}
    a, b = _read(str(tmp_path / "plain")), _read(str(tmp_path / "full"))  # the HIP event pairs of --full do not change what is computed
    assert sorted(a) == sorted(b) and all(np.array_equal(a[f], b[f]) for f in a)
