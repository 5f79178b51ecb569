"""bench.py host logic that needs no GPU: the PMC `traffic` figure is only reported while the kernel sources it was
measured on are unchanged."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _fake_tree(tmp_path):
    csrc = tmp_path / "parrot_amd" / "csrc"
    csrc.mkdir(parents=True)
    for name in ("skinny.hip", "skinny.h", "plans.hip", "plans_common.h", "att_fwd_body.h"):
        (csrc / name).write_text("// " + name + "\n")
    (tmp_path / "profiles").mkdir()
    return str(tmp_path)


def test_traffic_figure_fresh_stale_absent(tmp_path):
    import bench
    root = _fake_tree(tmp_path)
    assert bench.pmc_traffic_figure(root) == (None, None)  # nothing measured: null, no note
    blob = {"hbm_bytes_per_launch": 12345678, "session": "unit test", "source_digest": bench.kernel_source_digest(root)}
    path = os.path.join(root, "profiles", "r06_pmc_traffic.json")
    json.dump(blob, open(path, "w"))
    value, note = bench.pmc_traffic_figure(root)
    assert value == 12345678 and "unit test" in note and "r06_pmc_traffic.json" in note
    # a kernel source changes -> the figure is refused and the note says why
    with open(os.path.join(root, "parrot_amd", "csrc", "plans.hip"), "a") as f:
        f.write("// edited\n")
    value, note = bench.pmc_traffic_figure(root)
    assert value is None and "stale" in note
    # an unreadable file never yields a number
    open(path, "w").write("{not json")
    value, note = bench.pmc_traffic_figure(root)
    assert value is None and "unreadable" in note


def test_repo_has_no_stale_traffic_figure():
    """Whatever profiles/ holds for this tree: bench.py either reports a figure whose digest matches, or null."""
    import bench
    value, note = bench.pmc_traffic_figure()
    if value is not None:
        import re
        name = re.search(r"profiles/(\S+\.json)", note).group(1)  # the file the note says the figure comes from
        blob = json.load(open(os.path.join(ROOT, "profiles", name)))
        assert blob["source_digest"] == bench.kernel_source_digest()
    else:
        assert note is None or "stale" in note or "unreadable" in note


def test_dump_outputs_budget_and_fixed_sample(tmp_path):
    """--dump-outputs: every array of the last step as float32 / float64 .npy, below 64 MB in all; an array over its share
    is a sample at the same sorted distinct indices on every run, a small one is written whole in its own shape."""
    import types

    import numpy as np
    import torch
    import bench
    B, H, L = 4, 8, 2
    n = 16_000_000  # 64 MB of float32 parameters (exact integers below 2**24): over budget on their own
    model = types.SimpleNamespace(
        flat_parameters=torch.arange(n, dtype=torch.float32), flat_gradients=torch.full((1000,), 0.5),
        _carry={B: dict(h=[torch.randn(B, H) for _ in range(L)], c=[torch.randn(B, H) for _ in range(L)],
                        w=torch.randn(B, 3), k=torch.randn(B, 5))})
    cost = torch.tensor(1.25)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), cost, model, B)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["cost.npy", "parameters.npy", "gradients.npy", "state_w.npy", "state_k.npy"] +
                           [f"state_{s}{l}.npy" for s in "hc" for l in range(1, L + 1)])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64_000_000
    out = {f: np.load(tmp_path / "a" / f) for f in names}
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert out["cost.npy"].dtype == np.float64 and out["cost.npy"].tolist() == [1.25]
    p = out["parameters.npy"]
    assert 0 < p.size < n and np.all(np.diff(p) > 0)  # the values are their indices: sorted and distinct
    assert np.array_equal(p, np.load(tmp_path / "b" / "parameters.npy"))
    assert np.array_equal(out["gradients.npy"], model.flat_gradients.numpy())
    assert np.array_equal(out["state_h2.npy"], model._carry[B]['h'][1].numpy())
    assert np.array_equal(out["state_k.npy"], model._carry[B]['k'].numpy())


def test_bench_gpus2_starts_its_own_ranks():
    """`python bench.py --gpus 2` outside torchrun launches two ranks itself: the collective spans
    both (`ranks_seen` = all-reduce of ones) and the line says n_gpus 2.  CPU/gloo, no GPU step (--plumbing-only)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["PARROT_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--plumbing-only"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks_seen"] == 2 and out["allreduce_ms"] > 0


def test_bench_refuses_a_world_that_is_not_gpus():
    """--gpus 2 inside a 1-rank environment must fail, not silently report one GPU."""
    import subprocess
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plumbing-only"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
