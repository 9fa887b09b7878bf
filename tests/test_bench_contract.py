"""Driver-contract tests for bench.py.

The round driver runs `python bench.py --gpus N --steps K --warmup W` (N=1
directly; N>1 via `python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 ... bench.py ...`) and parses ONE
JSON line from rank 0.  These tests execute those exact invocations on CPU
(gloo fallback) and validate the contract fields, so a schema or rendezvous
regression is caught here rather than at round end on the GPU box."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}


def _json_line(out: str) -> dict:
    for line in out.splitlines():
        line = line.strip()
        if line.startswith("{") and '"metric"' in line:
            return json.loads(line)
    raise AssertionError(f"no bench JSON line in output:\n{out[-2000:]}")


def _check(rec: dict, n: int):
    assert REQUIRED <= set(rec), f"missing fields: {REQUIRED - set(rec)}"
    assert rec["metric"] == "images/sec (whole node) VGG16/CIFAR10 cut=7"
    assert rec["n_gpus"] == n
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "weak"
    assert rec["dtype"] == "fp32"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    cfg = rec["config"]
    assert cfg["model"] == "VGG16_CIFAR10"
    assert cfg["cut_layer"] == 7
    assert cfg["global_batch"] == 32 * max(n // 2, 1)
    assert f"dp{max(n // 2, 1)}" in cfg["parallelism"]


@pytest.mark.timeout(600)
def test_bench_n1_cpu_contract():
    p = subprocess.run([sys.executable, "bench.py", "--steps", "2",
                        "--warmup", "1"],
                       capture_output=True, text=True, cwd=REPO, timeout=550)
    assert p.returncode == 0, p.stderr[-2000:]
    _check(_json_line(p.stdout), 1)


DUMP_STEPS, DUMP_WARMUP = 2, 1


def _run_dump(out_dir, *extra, env=None):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps",
                        str(DUMP_STEPS), "--warmup", str(DUMP_WARMUP),
                        "--dump-outputs", str(out_dir), *extra],
                       capture_output=True, text=True, cwd=REPO, timeout=550,
                       env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = _json_line(p.stdout)
    _check(rec, 1)
    assert rec["steps"] == DUMP_STEPS
    return {f[:-4]: np.load(os.path.join(out_dir, f))
            for f in sorted(os.listdir(out_dir)) if f.endswith(".npy")}


@pytest.mark.timeout(600)
def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's results as float .npy
    files within the 64 MB budget, from identical inputs run to run (same
    names, shapes and sample positions); --full keeps the plain result line.

    Two runs with the same arguments must write the same outputs up to
    rounding: 1e-4 of each array's scale, 1e-3 on the loss.  The training
    step is chaotic (a 1e-7 input perturbation grows ~10x per step), so this
    only holds because every split-K / ci-split accumulation on this path
    reduces per-split slabs in a fixed order instead of using float atomics,
    and the graph-capture warm steps run on a real batch."""
    a = _run_dump(tmp_path / "a")
    b = _run_dump(tmp_path / "b", "--full")
    assert a["logits"].shape == (32, 10) and a["loss"].shape == ()
    assert any(k.startswith("stage1.") for k in a)
    assert any(k.startswith("stage2.") for k in a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    assert set(a) == set(b)
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64), k
        assert np.isfinite(v).all(), k
        assert v.shape == b[k].shape, k
    # Identical seeded weights and batches, a handful of SGD steps.  The CPU
    # path is deterministic, so there the two runs agree to the bit.  The
    # bound for any device is "rounding": fp32 sums of K <= 4608 terms taken
    # in another order differ by ~sqrt(K) * 2^-24 ~ 4e-6 relative, so 1e-4 of
    # an array's scale (1e-3 on a loss of ~2.3) leaves a wide margin.
    # --steps really sets the number of steps run: every BatchNorm counts its
    # training forwards (stage 1 runs two per step, the no_grad forward and
    # the recompute), and the GPU path adds 3 graph-capture warm steps
    n_steps = DUMP_WARMUP + DUMP_STEPS + (3 if torch.cuda.is_available() else 0)
    assert float(a["stage2.layer9.num_batches_tracked"]) == n_steps
    assert float(a["stage1.layer2.num_batches_tracked"]) == 2 * n_steps
    worst = max((float(np.abs(v - b[k]).max()) / max(1.0, float(np.abs(v).max())), k)
                for k, v in a.items() if v.size)
    d_loss = abs(float(a["loss"]) - float(b["loss"]))
    print(f"run-to-run: |dloss|={d_loss:.3e} worst scaled diff {worst[0]:.3e} ({worst[1]})")
    if not torch.cuda.is_available():
        for k, v in a.items():
            assert np.array_equal(v, b[k]), k
    assert d_loss < 1e-3
    assert worst[0] < 1e-4, worst


def test_bench_dump_matches_recomputed_last_step(tmp_path):
    """The dump is the LAST timed step's result: recompute warmup + steps with
    plain torch autograd and torch.optim.SGD from the same seeds, outside the
    pipeline classes, and compare logits, loss and weights.  Both sides run
    the deterministic CPU path (the bench process gets the GPUs hidden)."""
    sys.path.insert(0, REPO)
    try:
        import bench
    finally:
        sys.path.remove(REPO)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    dump = _run_dump(tmp_path / "d", env=env)
    assert float(dump["stage2.layer9.num_batches_tracked"]) == DUMP_WARMUP + DUMP_STEPS
    cpu = torch.device("cpu")
    s1, _ = bench.build_stage([0, bench.CUT], cpu)
    s2, _ = bench.build_stage([bench.CUT, -1], cpu)
    o1 = torch.optim.SGD(s1.parameters(), lr=bench.LR, momentum=bench.MOMENTUM)
    o2 = torch.optim.SGD(s2.parameters(), lr=bench.LR, momentum=bench.MOMENTUM)
    for seed, n in ((1, DUMP_WARMUP), (2, DUMP_STEPS)):   # run() bumps the seed
        xs, ys = bench.make_batches(cpu, n, seed=seed)
        for i in range(n):
            with torch.no_grad():
                act = s1(xs[i])
            act.requires_grad_(True)
            logits = s2(act)
            loss = torch.nn.functional.cross_entropy(logits, ys[i])
            o2.zero_grad()
            loss.backward()
            o2.step()
            o1.zero_grad()
            s1(xs[i]).backward(gradient=act.grad)
            o1.step()
    # same math, possibly another summation order inside the optimizer:
    # a few fp32 ulps of O(1) values
    np.testing.assert_allclose(dump["logits"], logits.detach().numpy(),
                               rtol=0, atol=1e-5)
    assert abs(float(dump["loss"]) - float(loss.detach())) < 1e-5
    for prefix, m in (("stage1", s1), ("stage2", s2)):
        for k, v in m.state_dict().items():
            d = dump[f"{prefix}.{k}"]
            if v.numel() <= bench.DUMP_SAMPLE_ELEMS:     # sampled ones: see above
                np.testing.assert_allclose(d, v.double().numpy() if d.dtype == np.float64
                                           else v.numpy(), rtol=0, atol=1e-5,
                                           err_msg=k)


def test_bench_inputs_identical_run_to_run():
    """Same arguments -> same batches, labels and initial weights."""
    sys.path.insert(0, REPO)
    try:
        import bench
    finally:
        sys.path.remove(REPO)
    cpu = torch.device("cpu")
    x1, y1 = bench.make_batches(cpu, 3, seed=5)
    x2, y2 = bench.make_batches(cpu, 3, seed=5)
    assert torch.equal(x1, x2) and torch.equal(y1, y2)
    assert x1.shape == (3, 32, 3, 32, 32) and y1.shape == (3, 32)
    x3, _ = bench.make_batches(cpu, 3, seed=6)
    assert not torch.equal(x1, x3)
    m1, _ = bench.build_stage([0, bench.CUT], cpu)
    m2, _ = bench.build_stage([0, bench.CUT], cpu)
    for (k, v1), v2 in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(v1, v2), k


def _rank_env(n):
    """These launches exercise the rendezvous and the result line, on gloo
    when the node has fewer than n GPUs: hide the devices from the ranks then,
    instead of letting rank >= device_count fail on a missing ordinal."""
    env = dict(os.environ)
    if torch.cuda.is_available() and torch.cuda.device_count() < n:
        env["HIP_VISIBLE_DEVICES"] = "-1"
        env["CUDA_VISIBLE_DEVICES"] = "-1"
    return env


@pytest.mark.timeout(900)
def test_bench_n2_torchrun_cpu_contract():
    """The driver's exact N=2 launch shape (gloo fallback on CPU).  On a node
    with a GPU but fewer than 2, the ranks are run with the devices hidden, so
    there this covers gloo only and never the nccl path."""
    p = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29417", "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, cwd=REPO, timeout=850, env=_rank_env(2))
    assert p.returncode == 0, p.stderr[-2000:]
    _check(_json_line(p.stdout), 2)


@pytest.mark.timeout(900)
def test_bench_n4_torchrun_cpu_contract():
    """4-rank rendezvous shape (2 pipelines) on gloo: the same launch the
    driver uses for the SCALE curve, so a multi-pipeline regression (rank
    mapping, eager comm warmup ordering, poison-drain) is caught on CPU.  On a
    node with a GPU but fewer than 4, the ranks are run with the devices
    hidden, so there this covers gloo only and never the nccl path."""
    p = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
         "--master-port", "29423", "bench.py", "--gpus", "4",
         "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, cwd=REPO, timeout=850, env=_rank_env(4))
    assert p.returncode == 0, p.stderr[-2000:]
    _check(_json_line(p.stdout), 4)
