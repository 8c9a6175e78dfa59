"""Host-side logic of bench.py (no GPU): how an instrumented pass is priced against the roofs, which entry point is
reported as dominant, where counter traffic comes from and when it is refused, the N > 1 self-launch environment."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_layer_table_prices_entry_points_against_their_roofs(monkeypatch):
    monkeypatch.setattr(bench, "_PMC", {"_meta": {"csrc_digest": bench.csrc_digest(), "commit": "abc", "source": "x"},
                                        "entries": {"cnn5_f32_1000|ecg_conv1d_fwd[256, 128, 256, 125, 15, 7]": 65_000_000,
                                                    # the same signature in another leg: must not be picked up
                                                    "mm_f32_1000|ecg_conv1d_fwd[256, 128, 256, 125, 15, 7]": 1}})
    timings = {
        ("ecg_conv1d_fwd", (256, 128, 256, 125, 15, 7)): [0.25, 0.25],                       # ms per call
        ("ecg_conv1d_bwd_weight_bias_ld", (128, 256, 128, 256, 125, 15, 7)): [0.27],         # heaviest: dominant
        ("ecg_conv1d_fwd_bf16_yh", (1, 632, 632, 256, 128, 256, 625, 15, 7)): [0.18],
        ("ecg_conv1d_bwd_data_bf16hh", (640, 632, 256, 128, 256, 625, 15, 7)): [0.16],
        ("ecg_bn_stats_relu_pool_fwd", (1024, 256000, 256, 32, 1000, 0)): [0.014],
    }
    rows, other_ms = bench.layer_table(timings, bench.leg_tag("cnn", 5, "f32", 1000))
    assert bench.leg_tag("multimodal", 5, "f32", 1000) == "mm_f32_1000" and bench.leg_tag("cnn", 1, "bf16", 5000) == "cnn1_bf16_5000"
    assert abs(other_ms - 0.014) < 1e-12 and len(rows) == 4
    by = {r["entry"].split("[")[0]: r for r in rows}
    f = by["ecg_conv1d_fwd"]
    flops = 2.0 * 256 * 256 * 128 * 15 * 125
    assert f["algorithmic_flops"] == flops and f["calls"] == 2 and f["operands"] == "f32"
    assert abs(f["tflops"] - flops / 0.25e-3 / 1e12) < 0.01 and abs(f["frac"] - f["tflops"] / 157.3) < 1e-3
    assert f["algorithmic_bytes"] == 4.0 * 256 * 125 * (128 + 256) + 4.0 * 256 * 128 * 15
    # the fast-FIR kernels issue 23 of the 30 multiplies per output pair: the matrix-pipe share is reported beside the algorithmic rate
    assert f["multiplies_per_output_pair"] == 23 and abs(f["pipe_frac"] - f["frac"] * 23 / 30) < 1e-3
    assert by["ecg_conv1d_fwd_bf16_yh"]["multiplies_per_output_pair"] == 30
    assert bench.frac_by_block(rows, "pipe_frac")["fwd"][-1] in (f["pipe_frac"], by["ecg_conv1d_fwd_bf16_yh"]["pipe_frac"])
    assert f["traffic_bytes_from_profile"] == 65_000_000 and f["traffic_over_algorithmic"] == round(65e6 / f["algorithmic_bytes"], 3)
    # bf16 activation storage: two bytes per activation element on both sides, priced against the bf16 peak
    h = by["ecg_conv1d_fwd_bf16_yh"]
    assert h["operands"] == "bf16" and h["peak"] == 2500.0
    assert h["algorithmic_bytes"] == 256.0 * (2 * 625 * 128 + 2 * 625 * 256) + 4.0 * 256 * 128 * 15
    assert h["traffic_bytes_from_profile"] is None and h["traffic_source"] == "not collected"
    assert by["ecg_conv1d_bwd_data_bf16hh"]["algorithmic_bytes"] == h["algorithmic_bytes"]
    # the dominant entry point is the one with the largest TOTAL time, multi-launch entry points included
    roof = bench.roofline_of(rows)
    assert roof["kernel"].startswith("ecg_conv1d_fwd[") and roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s"
    timings[("ecg_conv1d_bwd_weight_bias_ld", (128, 256, 128, 256, 125, 15, 7))] = [0.27, 0.27]
    roof = bench.roofline_of(bench.layer_table(timings)[0])
    assert roof["kernel"].startswith("ecg_conv1d_bwd_weight_bias_ld[") and roof["op"] == "wgrad"
    assert bench.roofline_of([]) is None


def test_counter_traffic_is_refused_for_other_kernel_sources(monkeypatch):
    key = "cnn5_f32_1000|ecg_conv1d_fwd[256, 12, 32, 1000, 15, 7]"
    monkeypatch.setattr(bench, "_PMC", {"_meta": {"csrc_digest": "0" * 16, "commit": "old", "source": "s"}, "entries": {key: 1}})
    tr, why = bench.pmc_traffic(key)
    assert tr is None and why.startswith("stale: collected for csrc 0000000000000000 at old")
    monkeypatch.setattr(bench, "_PMC", {})
    assert bench.pmc_traffic(key) == (None, "not collected")


def test_committed_counter_traffic_matches_the_committed_kernels():
    """profiles/pmc_traffic.json must have been collected for the kernel sources in the tree (bench.py prints null
    otherwise), and must cover every conv entry point of the headline step."""
    meta = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    assert meta["_meta"]["csrc_digest"] == bench.csrc_digest()
    keys = set(meta["entries"])
    for ci, co, L in ((12, 32, 1000), (32, 64, 500), (64, 128, 250), (128, 256, 125)):
        assert f"cnn5_f32_1000|ecg_conv1d_fwd[256, {ci}, {co}, {L}, 15, 7]" in keys
        assert f"mm_f32_1000|ecg_conv1d_fwd[256, {ci}, {co}, {L}, 15, 7]" in keys        # keyed by leg: no collisions


def test_percentiles_and_flop_counts():
    p = bench.percentiles([1.0, 2.0, 3.0, 4.0, 5.0])
    assert p["median"] == 3.0 and p["min"] == 1.0 and p["max"] == 5.0 and p["n"] == 5 and p["p10"] <= p["median"] <= p["p90"]
    fwd, step = bench.conv_flops_per_window(1000)
    per = [2 * co * ci * 15 * L for ci, co, L in ((12, 32, 1000), (32, 64, 500), (64, 128, 250), (128, 256, 125))]
    assert fwd == sum(per) and step == 3 * sum(per) - per[0]            # block 0 has no input gradient


def test_flat_adamw_exchange_switches_are_noops_without_a_process_group():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "ptbxl-multimodal_amd"))
    from ecg_hip.optim import FlatAdamW
    lin = torch.nn.Linear(4, 3)
    opt = FlatAdamW(lin.parameters(), lr=1e-3)
    assert opt.set_overlap(True) is False
    assert opt.calibrate_overlap(lambda n: pytest.fail("nothing to calibrate on one rank")) == {"mode": "single", "ms_per_step": {}}


def _fake_leg(name, short, n_rows=11, world=1, exchange=False):
    rows = []
    for i in range(n_rows):
        ci, co = bench.CONV_GEOM[i % 4]
        rows.append({"entry": f"ecg_conv1d_bwd_weight_bias_ld[128, 256, {ci}, {co}, 125, 15, 7]", "op": ("fwd", "dgrad", "wgrad")[i % 3],
                     "operands": "f32", "c_in": ci, "c_out": co, "L": 125, "calls": 5, "avg_us": 264.51 - i, "tflops": 118.93,
                     "peak": 157.3, "frac": 0.7561, "algorithmic_flops": 31457280000.0, "algorithmic_bytes": 51118080.0,
                     "traffic_bytes_from_profile": 132812345, "traffic_over_algorithmic": 2.598,
                     "traffic_source": "profiles/pmc_traffic.json (profiles/r02_pmc_summary.txt, commit b5d3eb7)" * 2,
                     "traffic_source_short": "pmc@b5d3eb7"})
    leg = {"workload": name, "workload_short": short, "value": 156103.4, "unit": "windows/s", "ms_per_step": 1.6399,
           "step_ms": {"median": 1.6391, "p10": 1.6312, "p90": 1.6533, "min": 1.62, "max": 1.71, "n": 20},
           "value_at_median_step": 156183.3, "dtype": "f32 " * 40, "dtype_short": "f32", "optimizer": "FlatAdamW",
           "loop": "train_one_epoch", "final_loss": 0.693147, "step_conv_tflops": 104.31, "step_frac_of_mfma_peak": 0.6631,
           "roofline": bench.roofline_of(rows), "frac_by_block": bench.frac_by_block(rows), "layers": rows,
           "instrumented_ms_per_step": {"conv_entry_points": 1.4412, "everything_else": 0.2011}}
    if exchange:
        leg["exchange_exposed_ms_per_step"] = {"median": 0.0712, "p10": 0.0601, "p90": 0.0899, "min": 0.05, "max": 0.2, "n": 5}
        leg["exchange"] = {"mode": "overlapped", "calibration_ms_per_step": {"overlapped": 1.7012, "single": 1.7144}}
    return leg


@pytest.mark.parametrize("world", [1, 8])
def test_printed_line_fits_the_driver_and_keeps_what_is_graded(world):
    """Round 2's line was 32 KB (per-entry-point tables of five legs) and the driver, which keeps 8000 characters of
    stdout, could parse nothing.  The line now stays under LINE_BUDGET whatever the legs carry; the tables go to the
    side file."""
    long_name = "ECGCNN(5) train step fwd+BCE+bwd+AdamW, 12x1000, fp32, batch 256/GPU, global batch 2048"
    primary = _fake_leg(long_name, "ECGCNN(5) 12x1000 f32 B=256", world=world, exchange=world > 1)
    also = [_fake_leg(long_name.replace("ECGCNN(5)", "ECGMultimodal (FiLM)"), f"leg {i} 12x5000 bf16 B=256 stockAdamW",
                      exchange=world > 1) for i in range(1 if world > 1 else 4)]
    cpu = None
    if world == 1:
        cpu = {"value": 1098.5, "unit": "windows/s", "cores": 16, "kind": "port", "threads": 16, "sample": "s" * 180,
               "thread_sweep": {str(t): 1000.0 + t for t in (8, 16, 32, 128)},
               "batch256": {"value": 1302.2, "median_ms": 196.6, "steps": 5}, "cpu_model": "AMD EPYC 9575F 64-Core Processor",
               "physical_cores": 128, "logical_cpus": 256, "torch_threads": 128, "torch": "2.10.0+rocm7.0"}
    rccl = None if world == 1 else {"backend": "nccl", "ranks_seen_by_allreduce": world, "rel_diff": 1.2e-9,
                                    "grad_checksum_sum_of_ranks": -0.123456789, "grad_checksum_after_allreduce": -0.123456789,
                                    "flat_gradient_bytes": 2877588}
    line, detail = bench.build_line(primary, also, cpu, rccl, n_gpus=world, steps=20, warmup=5, batch=256, length=1000,
                                    priming=30, priming_seconds=1.5, n1_value=150000.0 if world > 1 else None)
    line["detail"] = "gpurun_out/bench_detail_n8.json"
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < bench.LINE_BUDGET, len(text)
    back = json.loads(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "step_ms"):
        assert key in back, key
    assert back["dtype"] == "f32" and back["vs_baseline"] is None and back["config"]["global_batch"] == 256 * world
    assert "model" not in back["config"] and back["config"]["workload"] == long_name
    for key in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_flops", "algorithmic_bytes"):
        assert key in back["roofline"], key
    assert "layers" not in back and all("layers" not in leg for leg in back.get("also", []))
    assert len(detail["primary"]["layers"]) == 11 and len(detail["also"]) == len(also)      # the tables survive in the side file
    if world == 1:
        for key in ("value", "unit", "cores", "kind", "sample", "cpu_model", "physical_cores"):
            assert key in back["cpu_baseline"], key
        assert "rccl" not in back
    else:
        assert "cpu_baseline" not in back
        assert back["rccl"]["ranks_seen_by_allreduce"] == world and back["rccl"]["exchange"]["mode"] == "overlapped"
        assert back["rccl"]["exchange_exposed_ms_per_step"]["median"] == 0.0712
        assert back["efficiency_vs_n1"] == round(156103.4 / (world * 150000.0), 4)
        assert back["also"][0]["exchange_mode"] == "overlapped"


def test_line_sheds_optional_blocks_before_it_outgrows_the_budget():
    primary = _fake_leg("w" * 300, "p")
    also = [_fake_leg("x", "y" * 120) for _ in range(40)]
    line, _ = bench.build_line(primary, also, None, None, n_gpus=1, steps=20, warmup=5, batch=256, length=1000, priming=30,
                               priming_seconds=1.5)
    assert len(json.dumps(line, separators=(",", ":"))) < bench.LINE_BUDGET
    assert "roofline" in line and "value" in line and "also" not in line


def test_self_launch_reports_the_failing_rank_and_does_not_wait_for_a_timeout(capfd):
    """A rank that dies (here: every rank — there is no GPU in the CPU test run, or an unknown flag on a GPU box)
    must end the launch with its exit code and the tail of ITS stderr, not after a collective timeout."""
    import time
    t0 = time.time()
    rc = bench.self_launch(2, argv=["--gpus", "2", "--no-such-flag"], grace_s=2.0)
    assert rc != 0 and time.time() - t0 < 120
    err = capfd.readouterr().err
    assert "rank exit codes" in err and "last lines of stderr" in err and "no-such-flag" in err


def test_rank_env_explains_itself():
    env = bench.rank_env(3, 8, 1234, base={"PATH": "/bin"})
    assert env["RANK"] == env["LOCAL_RANK"] == "3" and env["WORLD_SIZE"] == "8" and env["MASTER_ADDR"] == "127.0.0.1"
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and "dmabuf" in bench.rank_env.__doc__
    assert bench.rank_env(0, 2, 1, base={"HSA_ENABLE_IPC_MODE_LEGACY": "1"})["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"


def test_plain_line_carries_the_headline_and_nothing_from_the_extra_passes():
    """A plain run (no --full) measures the timed steps only: its primary record has the headline figures, and the line
    holds them with the configuration, without the blocks that the per-step, instrumented and other-leg passes fill."""
    full = _fake_leg("ECGCNN(5) train step", "ECGCNN(5) 12x1000 f32 B=256")
    lean = {k: full[k] for k in ("workload", "workload_short", "value", "unit", "ms_per_step", "dtype", "dtype_short",
                                 "optimizer", "loop", "final_loss", "step_conv_tflops", "step_frac_of_mfma_peak")}
    line, _ = bench.build_line(lean, [], None, None, n_gpus=1, steps=20, warmup=5, batch=256, length=1000, priming=30,
                               priming_seconds=1.5)
    back = json.loads(json.dumps(line, separators=(",", ":")))
    assert back["value"] == 156103.4 and back["ms_per_step"] == 1.6399 and back["unit"] == "windows/s"
    assert back["higher_is_better"] is True and back["dtype"] == "f32" and back["steps"] == 20 and back["warmup"] == 5
    assert back["config"]["global_batch"] == 256 and back["config"]["final_loss"] == 0.693147
    for key in ("step_ms", "roofline", "frac_by_block", "instrumented_ms_per_step", "also", "cpu_baseline", "rccl",
                "ref_batch_sizes"):
        assert key not in back, key


def test_output_arrays_are_what_the_loop_leaves_after_its_last_step(tmp_path):
    """--dump-outputs: the loop's mean loss, every parameter and buffer, and the last step's gradients, as float32 /
    float64 .npy files (here on CPU tensors, which the loop API runs through stock torch)."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "ptbxl-multimodal_amd"))
    from ecg_hip.optim import FlatAdamW
    from src.models.ecg_cnn import ECGCNN
    from src.training.loop import train_one_epoch
    from src.utils.seed import set_seed
    set_seed(42)
    model = ECGCNN(num_labels=5)
    opt = FlatAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    g = torch.Generator().manual_seed(1234)
    batch = (torch.randn(4, 12, 1000, generator=g), (torch.rand(4, 5, generator=g) < 0.3).float())
    loss = train_one_epoch(model, bench.ListLoader(batch, 3), opt, "cpu")
    arrays = bench.output_arrays(model, loss)
    bench.write_outputs(str(tmp_path / "out"), arrays)
    back = {p.name[:-len(".npy")]: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(back) == set(arrays)
    assert back["loss"].dtype == np.float64 and float(back["loss"]) == loss
    sd = model.state_dict()
    assert {k for k in back if k.startswith("state.")} == {f"state.{k}" for k in sd}
    assert {k for k in back if k.startswith("grad.")} == {f"grad.{k}" for k, _ in model.named_parameters()}
    for k, v in sd.items():
        a = back[f"state.{k}"]
        if k.endswith("num_batches_tracked"):
            assert a.dtype == np.float64 and float(a) == 3.0            # exactly the steps the loop took
        else:
            assert a.dtype == np.float32 and np.array_equal(a, v.numpy())
    for k, p in model.named_parameters():
        assert back[f"grad.{k}"].dtype == np.float32 and np.array_equal(back[f"grad.{k}"], p.grad.numpy())
    assert sum(a.nbytes for a in back.values()) < 64 << 20
