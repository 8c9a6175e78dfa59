"""Scoring a continuous recording: the sliding input step against the copy-then-cut path it replaces, and
score_recording end to end.

    python tools/bench_recording.py [--hours 1] [--rounds 7] [--iters 20] [--out profiles/recording_bench.json]

Workloads: one 12-lead recording of --hours at 500 Hz (window 5000) and at 100 Hz (window 1000), hop = window / 2.
  (a) sliding   ecg_wfdb16_windows on the recording in place
  (b) gather    what the entry points for pre-cut windows allow: a torch index-gather of the overlapping slices into
                [W][T][leads], then wfdb16_to_windows
  (c) score     score_recording in fp32 and under inference_precision("bf16"), without CAMs and with CAMs for all classes
(a) and (b) alternate in one process, --rounds times; each round times --iters calls between device events.  The bytes
are counted from the shapes; "frac_of_hbm" is bytes / time over the 6.3 TB/s the project uses as achievable bandwidth.
Fails when no GPU is visible: no number here means anything on a CPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ptbxl-multimodal_amd")]
HBM_BYTES_PER_S = 6.3e12
LEADS = 12


def timed(fn, iters):
    """ms per call: `iters` calls between two device events, synchronised."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def prime(fn, seconds=0.5):
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end:
        fn()
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recording_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_recording: no GPU visible")
    from ecg_hip import _lib
    from ecg_hip import functional as F
    from ecg_hip.recording import score_recording, window_plan
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    _lib.call("ecg_check_device")
    res = []
    for fs, window in ((500, 5000), (100, 1000)):
        Ttot, hop = int(a.hours * 3600 * fs), window // 2
        rng = np.random.default_rng(fs)
        d = torch.from_numpy(rng.integers(-3000, 3000, size=(1, Ttot, LEADS)).astype(np.int16)).cuda()
        gain = torch.full((1, LEADS), 1000.0, dtype=torch.float64).cuda()
        base = torch.zeros(1, LEADS, dtype=torch.int32).cuda()
        plan = window_plan(Ttot, window, hop)
        W = plan[2]
        starts = torch.tensor(plan[4], device="cuda")
        gW, bW = gain.expand(W, LEADS).contiguous(), base.expand(W, LEADS).contiguous()
        idx = starts[:, None] + torch.arange(window, device="cuda")[None, :]            # [W][T] sample indices

        def sliding():
            return F.wfdb16_to_windows_sliding(d, gain, base, window, hop)[0]

        def gather():
            return F.wfdb16_to_windows(d[0][idx], gW, bW)

        assert torch.equal(sliding()[0], gather())
        prime(sliding), prime(gather)
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(timed(sliding, a.iters))
            tb.append(timed(gather, a.iters))
        n = W * window * LEADS                           # window samples
        bytes_a, bytes_b = n * (2 + 4), n * (2 + 2 + 2 + 4)
        ma, mb = float(np.median(ta)), float(np.median(tb))
        line = {"metric": "recording_input_step_ms", "value": round(ma, 4), "unit": "ms",
                "config": {"workload": f"{a.hours:g} h, {LEADS} leads at {fs} Hz (Ttot {Ttot}), window {window}, hop {hop}, "
                                       f"{W} windows, int16 -> z-scored fp32"},
                "sliding_ms": [round(t, 4) for t in ta], "gather_ms": [round(t, 4) for t in tb],
                "sliding_median_ms": round(ma, 4), "gather_median_ms": round(mb, 4),
                "gather_spread_ms": round(max(tb) - min(tb), 4), "gather_over_sliding": round(mb / ma, 3),
                "sliding_within_gather_spread": bool(ma <= mb + (max(tb) - min(tb))),
                "sliding_bytes": bytes_a, "gather_bytes": bytes_b,
                "sliding_frac_of_hbm": round(bytes_a / (ma * 1e-3) / HBM_BYTES_PER_S, 4),
                "gather_frac_of_hbm": round(bytes_b / (mb * 1e-3) / HBM_BYTES_PER_S, 4),
                "windows_per_s": round(W / (ma * 1e-3), 1)}
        print(json.dumps(line), flush=True)
        res.append(line)

        set_seed(42)
        model = ECGCNN(num_labels=5).cuda().eval()
        x = sliding()[0, :a.batch].contiguous()
        for prec in ("fp32", "bf16"):
            with F.inference_precision(prec):
                def forward():
                    with torch.no_grad():
                        return F.sigmoid(model(x))
                prime(forward)
                eval_ms = timed(forward, a.iters)                # tools/bench_eval.py's step on this window shape
                for cams in (None, [0, 1, 2, 3, 4]):
                    def score():
                        return score_recording(model, d, gain, base, window=window, hop=hop, batch_size=a.batch,
                                               cam_classes=cams)
                    prime(score)
                    ms = float(np.median([timed(score, max(1, a.iters // 4)) for _ in range(a.rounds)]))
                    line = {"metric": "score_recording_windows_per_s", "value": round(W / (ms * 1e-3), 1), "unit": "windows/s",
                            "config": {"workload": f"ECGCNN(5) score_recording, {a.hours:g} h at {fs} Hz, window {window}, hop {hop}, "
                                                   f"{W} windows in chunks of {a.batch}, {prec}, "
                                                   f"{'CAMs for 5 classes' if cams else 'no CAMs'}"},
                            "ms_per_recording": round(ms, 3), "recording_seconds_per_s": round(Ttot / fs / (ms * 1e-3), 1),
                            "eval_forward_windows_per_s": round(a.batch / (eval_ms * 1e-3), 1),
                            "orchestration_cost": round((a.batch / eval_ms) / (W / ms), 3)}
                    print(json.dumps(line), flush=True)
                    res.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
