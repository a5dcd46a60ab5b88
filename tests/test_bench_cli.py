"""CPU: the launcher logic of bench.py that needs no GPU -- `--gpus N` without a launcher must either spawn N ranks
or refuse loudly; it used to be parsed and ignored.  (The 2-rank run itself is tests/test_gpu_bench_multirank.py.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(env_extra, *flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=300)


def test_gpus_n_refuses_a_node_without_n_gpus():
    import torch

    if torch.cuda.device_count() >= 2:
        return   # (a multi-GPU node: the command would really run; covered by the GPU suite)
    r = _run({}, "--gpus", "2", "--steps", "2")
    assert r.returncode != 0 and "--gpus 2" in (r.stderr + r.stdout) and "GPU(s)" in (r.stderr + r.stdout), (r.returncode, r.stderr[-400:])


def test_world_size_must_match_gpus():
    r = _run({"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, "--gpus", "4", "--steps", "2")
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout), (r.returncode, r.stderr[-400:])
    r = _run({}, "--gpus", "0")
    assert r.returncode != 0 and ">= 1" in (r.stderr + r.stdout)


def test_steps_must_be_positive():
    r = _run({}, "--steps", "0")
    assert r.returncode != 0 and "--steps must be >= 1" in (r.stderr + r.stdout), (r.returncode, r.stderr[-400:])


def test_dump_outputs_formats_and_budget(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 arrays only; over the byte budget of the whole job, the batch-major arrays become the
    same seeded sample of rows in every run (indices stored beside them), the others are written whole, and the files of all
    ranks together stay within the budget; a row that cannot fit is an error, not an empty file."""
    import numpy as np
    import pytest
    import torch

    import bench

    small = {"h": torch.arange(6, dtype=torch.bfloat16).view(2, 3), "d": torch.ones(2, dtype=torch.float64)}
    assert bench.dump_outputs(str(tmp_path / "small"), small) == {"h": [2, 3], "d": [2]}
    assert sorted(os.listdir(tmp_path / "small")) == ["d.npy", "h.npy"]
    h, d = np.load(tmp_path / "small" / "h.npy"), np.load(tmp_path / "small" / "d.npy")
    assert h.dtype == np.float32 and np.array_equal(h, np.arange(6).reshape(2, 3)) and d.dtype == np.float64

    budget = 40000
    monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    y, g, k = torch.randn(10, 1000), torch.randn(10, 100, dtype=torch.float64), torch.randn(50)
    out = {"y": y, "grad_a": g, "grad_room_kernel": k}
    for run in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / run), out) == {"y": [8, 1000], "grad_a": [8, 100], "grad_room_kernel": [50],
                                                               "rows": [8]}
        files = sorted(os.listdir(tmp_path / run))
        assert files == ["grad_a.npy", "grad_room_kernel.npy", "rows.npy", "y.npy"]
        assert sum(os.path.getsize(tmp_path / run / f) for f in files) <= budget
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))
    idx = rows.astype(np.int64)
    assert np.array_equal(idx, np.unique(idx)) and idx.min() >= 0 and idx.max() < 10
    assert np.array_equal(np.load(tmp_path / "a" / "y.npy"), y.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "grad_a.npy"), g.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "grad_room_kernel.npy"), k.numpy())

    # N ranks share the one budget: every rank writes its shard under its own names
    world = 2
    for r in range(world):
        written = bench.dump_outputs(str(tmp_path / "ranks"), {"y": y, "grad_a": g}, rank=r, world=world)
        assert written == {f"y_rank{r}": [4, 1000], f"grad_a_rank{r}": [4, 100], f"rows_rank{r}": [4]}, written
    files = os.listdir(tmp_path / "ranks")
    assert len(files) == 3 * world and sum(os.path.getsize(tmp_path / "ranks" / f) for f in files) <= budget

    with pytest.raises(ValueError, match="not one batch row"):
        bench.dump_outputs(str(tmp_path / "big"), {"y": torch.zeros(2, budget)})
    assert not os.path.exists(tmp_path / "big")
