"""Two data-parallel ranks through the HIP path on ONE device (exchange over gloo: RCCL refuses two
ranks per GPU) — the multi-rank code path of bench.py / FlatAdamW end to end: rank-0 broadcast,
bucketed backward-overlapped all-reduce of the flat gradient, per-rank BatchNorm statistics.
Expected values: the CPU oracle run as two shards with averaged gradients (fixture G5 semantics)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_two_shards(steps=2):
    from oracle import ref_models as R
    R.seed_all(42)
    model = R.RefECGMultimodal().train()
    opt = R.make_adamw(model, 1e-4, 1e-4)
    x, xd, y = R.synthetic_batch(16, 1000, 5, demo=True)
    losses = []
    for _ in range(steps):
        # per-shard forward/backward on the SAME weights (per-rank BN statistics), gradients averaged;
        # running statistics: each rank keeps its own — rank 0's are the ones compared below
        grads, shard_losses, bufs0 = None, [], None
        start = {k: v.clone() for k, v in model.state_dict().items()}
        for r in range(2):
            model.load_state_dict(start)
            opt.zero_grad()
            sl = slice(8 * r, 8 * r + 8)
            logits = model(x[sl], xd[sl])
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y[sl])
            loss.backward()
            shard_losses.append(float(loss.detach()))
            g = [p.grad.clone() for p in model.parameters()]
            grads = g if grads is None else [a + b for a, b in zip(grads, g)]
            if r == 0:
                bufs0 = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
        model.load_state_dict(start)
        for p, g in zip(model.parameters(), grads):
            p.grad = g / 2
        opt.step()
        sd = model.state_dict()
        sd.update(bufs0)
        model.load_state_dict(sd)
        losses.append(shard_losses)
    return model.state_dict(), np.array(losses)


@pytest.mark.parametrize("overlap", [True, False, "wrap"])
def test_two_ranks_share_one_gpu(tmp_path, overlap):
    env = dict(os.environ, ECG_HIP_REHEARSE_ON_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "ddp_gpu_worker.py"), str(tmp_path),
           "wrap" if overlap == "wrap" else ("1" if overlap else "0")]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    r0, r1 = (dict(np.load(tmp_path / f"rank{r}.npz")) for r in range(2))
    want, want_losses = _oracle_two_shards()
    lr = 1e-4
    for k, w in want.items():
        w = w.numpy()
        if "running" in k or "num_batches" in k:
            # BatchNorm buffers are rank-local (no SyncBN in the reference); rank 0 = shard 0
            if "num_batches" in k:
                assert r0[k] == w == 2 and r1[k] == 2
            else:
                np.testing.assert_allclose(r0[k], w, rtol=1e-4, atol=1e-5, err_msg=k)
            continue
        assert np.array_equal(r0[k], r1[k]), f"{k}: replicas diverged after the exchange"
        # AdamW moves noise-level gradients by up to lr per step whatever the implementation
        assert np.abs(r0[k] - w).max() <= 2.02 * lr * 2, k
        assert np.mean(np.abs(r0[k] - w) > 0.3 * lr * 2) <= 0.03 or r0[k].size < 70, k
    np.testing.assert_allclose(r0["losses"], want_losses[:, 0], atol=2e-4)
    np.testing.assert_allclose(r1["losses"], want_losses[:, 1], atol=2e-4)


@pytest.mark.parametrize("launcher", ["self", "torchrun"])
def test_bench_two_rank_line(tmp_path, launcher):
    """bench.py for N > 1 in both launch forms — the plain `python bench.py --gpus 2` (bench starts its own
    rank processes before touching the GPU) and the driver's torch.distributed.run form — rehearsed with both
    ranks on one device (gloo): one JSON line from rank 0 with the contract's fields and the exchange checks."""
    import json
    env = dict(os.environ, ECG_HIP_REHEARSE_ON_ONE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    detail = tmp_path / "detail.json"
    tail = [os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "4", "--warmup", "2", "--priming", "2",
            "--priming-seconds", "0.2", "--batch", "32", "--n1-value", "1000", "--detail", str(detail)]
    if launcher == "self":
        cmd = [sys.executable] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + tail
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    assert len(lines[0]) < 4000, len(lines[0])          # the driver keeps 8000 characters of stdout (round 2: 32 KB, unparsed)
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "step_ms", "frac_by_block", "rccl", "efficiency_vs_n1",
                "detail"):
        assert key in d, key
    assert "layers" not in d and d["dtype"] == "f32"
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak" and d["unit"] == "windows/s"
    assert d["config"]["global_batch"] == 64 and d["config"]["parallelism"] == "dp2"
    assert "cpu_baseline" not in d                      # rank 0 at N = 1 only
    assert abs(d["value"] - 64 * 4 / (d["ms_per_step"] * 4 * 1e-3)) / d["value"] < 1e-3
    assert d["step_ms"]["n"] == 4 and d["step_ms"]["p10"] <= d["step_ms"]["median"] <= d["step_ms"]["p90"]
    r = d["rccl"]
    assert r["ranks_seen_by_allreduce"] == 2 and r["rel_diff"] < 1e-6 and r["flat_gradient_bytes"] == 719397 * 4
    assert r["exchange_exposed_ms_per_step"]["n"] == 5
    for fr in d["frac_by_block"].values():
        assert len(fr) == 4
    assert d["frac_by_block"]["dgrad"][0] is None         # block 0 has no input gradient
    assert r["exchange"]["mode"] in ("overlapped", "single") and set(r["exchange"]["calibration_ms_per_step"]) == {"overlapped", "single"}
    assert [a["value"] > 0 for a in d["also"]] == [True]          # N > 1: the multimodal leg only
    assert d["also"][0]["exchange_mode"] in ("overlapped", "single")
    full = json.loads(detail.read_text())               # the per-entry-point tables live in the side file
    layers = full["primary"]["layers"]
    assert {row["op"] for row in layers} == {"fwd", "dgrad", "wgrad"} and len(layers) == 11
    assert len(full["also"][0]["layers"]) == 11 and full["rccl"]["grad_checksum_sum_of_ranks"] != 0


def test_one_rank_rccl_exchange():
    """The exchange code on RCCL itself: a one-rank `nccl` group (the most RCCL a one-GPU box can run) through the
    hooked two-bucket all-reduce, the single all-reduce, FlatGradDDP + stock AdamW and no_sync() accumulation — each
    bit-identical to the step without an exchange (tools/rccl_selftest.py)."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ECG_HIP_REHEARSE_ON_ONE_GPU"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_selftest.py"), "--steps", "10", "--port",
                          str(_free_port())], env=env, capture_output=True, text=True, timeout=400)
    assert res.returncode == 0, res.stderr[-3000:]
    d = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["ok"] and d["backend"] == "nccl" and d["world"] == 1 and d["ranks_seen_by_allreduce"] == 1
    assert d["flat_adamw_hooked_exchange"] == {"overlap_hooks_active": True, "bit_identical_to_unexchanged_step": True}
    for k in ("flat_adamw_single_allreduce", "flat_grad_ddp_stock_adamw", "no_sync_accumulation"):
        assert d[k]["bit_identical_to_unexchanged_step"], k
    assert d["allreduce_two_buckets_ms"]["floats"] == 719397
    # the one-launch BatchNorm backward is chosen per call from what the parameters' owner declared: OFF while hooks issue
    # all-reduces under backward, ON for the single all-reduce / FlatGradDDP (their exchange starts after the last backward
    # kernel) and for undeclared parameters of a single-rank process; set_overlap() moves an optimizer between the two
    assert d["bn_backward_one_launch"] == {"undeclared_single_rank": True, "hooked_exchange": False,
                                           "single_allreduce": True, "hooked_then_set_overlap_false": True,
                                           "flat_grad_ddp": True}
