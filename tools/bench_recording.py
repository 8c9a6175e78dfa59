"""Scoring a continuous recording: the sliding input step against the copy-then-cut path it replaces, and
score_recording end to end.

    python tools/bench_recording.py [--hours 1] [--rounds 7] [--iters 20] [--out profiles/recording_bench.json]
                                    [--legs recording,resample,filter,decode,quality,beats,template]
                                    [--resample-out profiles/resample_bench.json]

Workloads: one 12-lead recording of --hours at 500 Hz (window 5000) and at 100 Hz (window 1000), hop = window / 2.
  (a) sliding   ecg_wfdb16_windows on the recording in place
  (b) gather    what the entry points for pre-cut windows allow: a torch index-gather of the overlapping slices into
                [W][T][leads], then wfdb16_to_windows
  (c) score     score_recording in fp32 and under inference_precision("bf16"), without CAMs and with CAMs for all classes
(a) and (b) alternate in one process, --rounds times; each round times --iters calls between device events.  The bytes
are counted from the shapes; "frac_of_hbm" is bytes / time over the 6.3 TB/s the project uses as achievable bandwidth.

Leg "resample": the same one-hour 12-lead recording at 500 Hz scored by the 12x1000 model at 100 Hz (hop = window / 2).
  (d) resampled  ecg_wfdb16_windows_resampled on the recording in place
  (e) stock      wfdb16_to_windows(normalize=False) on the whole recording, a strided torch.nn.functional.conv1d with the
                 same taps (edge-padded), a torch index-gather of the windows, then ecg_zscore_rows
alternating in one process like (a) and (b), together with the streaming plan spelled out (the resampling launch, then
ecg_zscore_rows in place) against the plan the entry point picks; the resampling launch alone (normalize=False) is also rated against the bytes it must
move, 2*down/up B in + 4 B out per output sample.  Written to --resample-out.

Leg "filter" (not in the default --legs): the zero-phase FIR conditioning step, ecg_fir_windows.
  (f) fir_windows on --batch windows of 12x1000 with the default 100 Hz high-pass (half 363), and of 12x5000 with the
      500 Hz high-pass + 50 Hz notch (half 2720): int16 -> physical fp32 (wfdb16_to_windows(normalize=False)) -> fir_windows
  (g) score_recording(filter=...) on the one-hour recording at both rates, fp32, no CAMs
each against (a) the unfiltered path on the same plan (wfdb16_to_windows / score_recording without filter: what the
feature adds) and (b) what a user would otherwise run on the device: torch.nn.functional.conv1d with the same taps over
the replicate-padded fp32 recording, then cutting and zscore_per_lead.  The three alternate in one process, --rounds
times; the calls per round are cut down where one call is long, so that a round stays near a third of a second.
Written into --out under "filter" (the other entries of that file are kept).

Leg "decode" (not in the default --legs): the step before all of them, ecg_wfdb_decode16 — the bytes of a .dat file -> the
int16 stream.  The one-hour 12-lead 500 Hz recording stored as format 212, and 12 of the 15 signals (by name, reordered) of a
one-hour format-16 file at 1000 Hz.
  (h) kernel   functional.wfdb_decode16 on the uploaded bytes
  (i) torch    the same decode in torch tensor ops on the device (view(-1, 3), shifts and masks, stack; a column gather for
               the format-16 file): the stock alternative, several passes over widened temporaries
  (j) numpy    the decode on the host and an upload of the int16 result
alternating in one process like the others.  The kernel is also rated against the bytes it must move (1.5 B in + 2 B out
per sample for 212; 2 B + 2 B per selected sample for the selection), and its share of score_wfdb_record end to end (header,
file read, upload, decode, checksum, scoring; host clock around a synchronise) is reported.  Written into --out under
"decode".

Leg "quality" (not in the default --legs): the signal-quality stage, ecg_wfdb16_quality, on the one-hour 12-lead recording at
100 Hz (window 1000, hop 500) and at 500 Hz (window 5000, hop 2500).
  (k) kernel   functional.wfdb16_quality on the recording in place: one launch, rated against the R*W*Tq*leads*2 bytes it
               must read
  (l) torch    the same table in torch tensor ops on the device: unfold plus masked reductions, run lengths through a
               cummax of the positions where the value changes (checked equal to the kernel's table)
  (m) score    score_recording with quality=True against the same call without it (fp32, no CAMs): what the gate adds
alternating in one process like the others.  Written into --out under "quality".

Leg "beats" (not in the default --legs): beat detection and the rhythm table on the one-hour 12-lead recording at 100 Hz
(window 1000, hop 500) and at 500 Hz (window 5000, hop 2500): R-like pulses every 0.7-0.9 s in noise, BeatSpec() defaults.
  (n) kernel   functional.wfdb16_beats + functional.beats_rhythm (five launches); "detect" is wfdb16_beats alone
  (o) torch    the same detector in torch tensor ops on the device: cumsum for g, max_pool1d for the windowed maxima,
               nonzero for the list (checked equal to the kernel's list; no table)
  (p) score    score_recording with beats=True against the same call without it (fp32, no CAMs): what the stage adds
alternating in one process like the others.  Written into --out under "beats".

Leg "template" (not in the default --legs): beat morphology on the same one-hour recordings and their device-made beat
lists, TemplateSpec() defaults.
  (q) kernels  functional.beats_sum over the display range, functional.beats_match over the match range against the centred
               mean template, functional.beats_series_mean of five fp32 series on the recording's own axis; beats_sum is
               also rated against the bytes it must read (the whole segments, 2 B a sample, and the list)
  (r) torch    the same sums in torch tensor ops on the device: an index tensor [beats][Lseg], a gather of the segments
               and a masked sum (the integer sums checked equal to the kernel's; the fp32 mean adds in another order)
  (s) score    score_recording with beats=True, template=True against beats=True alone (fp32, no CAMs)
alternating in one process like the others.  Written into --out under "template".
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


def resample_leg(a):
    """500 Hz recording -> 12x1000 windows at 100 Hz: the resampled entry point against stock torch on the same GPU."""
    from ecg_hip import functional as F
    from ecg_hip.recording import window_plan
    from ecg_hip.resample import device_taps, rational_ratio, resampled_length
    fs, model_fs, window = 500, 100, 1000
    hop = window // 2
    up, down = rational_ratio(fs, model_fs)
    Ttot = int(a.hours * 3600 * fs)
    Tout = resampled_length(Ttot, up, down)
    rng = np.random.default_rng(fs)
    d = torch.from_numpy(rng.integers(-3000, 3000, size=(1, Ttot, LEADS)).astype(np.int16)).cuda()
    gain = torch.full((1, LEADS), 1000.0, dtype=torch.float64).cuda()
    base = torch.zeros(1, LEADS, dtype=torch.int32).cuda()
    first, hop, W, last, starts = window_plan(Tout, window, hop)
    taps, ntap, half = device_taps(up, down, d.device)
    # stock form of the same filter: y[n] = sum_i g[phi][i] * p[k0 - i]; for up == 1 that is a correlation of the edge-padded
    # signal with the reversed taps at stride `down` (this leg's ratio; a general up would need one conv per phase)
    assert up == 1
    w = taps[0].flip(0).reshape(1, 1, ntap).expand(LEADS, 1, ntap).contiguous()
    lpad = ntap - 1 - half // up
    rpad = max(0, ((Tout - 1) * down + half) // up - (Ttot - 1))
    idx = torch.tensor(starts, device="cuda")[:, None] + torch.arange(window, device="cuda")[None, :]      # [W][T]

    def resampled():
        return F.wfdb16_windows_resampled(d, gain, base, window, first, hop, W, last, up, down)

    def kernel_only():
        return F.wfdb16_windows_resampled(d, gain, base, window, first, hop, W, last, up, down, normalize=False)

    def streaming():                # the streaming plan spelled out: the resampling launch, then ecg_zscore_rows in place
        p = kernel_only()
        return F.zscore_per_lead(p, out=p)

    def stock():
        p = F.wfdb16_to_windows(d, gain, base, normalize=False)                          # [1][leads][Ttot]
        p = torch.nn.functional.pad(p, (lpad, rpad), mode="replicate")
        y = torch.nn.functional.conv1d(p, w, stride=down, groups=LEADS)[..., :Tout]      # [1][leads][Tout]
        x = y[0][:, idx].permute(1, 0, 2).contiguous()                                   # [W][leads][T]
        return F.zscore_per_lead(x, out=x)

    # same filter, another summation order and fused multiply-adds: close, not bit-identical
    diff = float((resampled()[0] - stock()).abs().max())
    assert diff <= 1e-3, diff
    assert torch.equal(resampled(), streaming())
    prime(resampled), prime(stock), prime(kernel_only), prime(streaming)
    ta, tb, tk, ts = [], [], [], []
    for _ in range(a.rounds):
        ta.append(timed(resampled, a.iters))
        tb.append(timed(stock, a.iters))
        tk.append(timed(kernel_only, a.iters))
        ts.append(timed(streaming, a.iters))
    n = W * window * LEADS                                                               # output samples
    must = n * (2.0 * down / up + 4.0)
    ma, mb, mk = float(np.median(ta)), float(np.median(tb)), float(np.median(tk))
    line = {"metric": "resampled_input_step_ms", "value": round(ma, 4), "unit": "ms",
            "config": {"workload": f"{a.hours:g} h, {LEADS} leads at {fs} Hz (Ttot {Ttot}) -> {model_fs} Hz (up/down {up}/{down}, "
                                   f"{ntap} taps, Tout {Tout}), window {window}, hop {hop}, {W} windows, int16 -> z-scored fp32"},
            "resampled_ms": [round(t, 4) for t in ta], "stock_ms": [round(t, 4) for t in tb],
            "kernel_only_ms": [round(t, 4) for t in tk], "streaming_plan_ms": [round(t, 4) for t in ts],
            "streaming_plan_median_ms": round(float(np.median(ts)), 4),
            "streaming_over_resampled": round(float(np.median(ts)) / ma, 3),
            "resampled_median_ms": round(ma, 4), "stock_median_ms": round(mb, 4), "kernel_only_median_ms": round(mk, 4),
            "stock_spread_ms": round(max(tb) - min(tb), 4), "resampled_spread_ms": round(max(ta) - min(ta), 4),
            "stock_over_resampled": round(mb / ma, 3), "max_abs_diff_resampled_vs_stock": diff,
            "kernel_bytes_it_must_move": int(must), "kernel_GBps_of_those_bytes": round(must / (mk * 1e-3) / 1e9, 1),
            "kernel_frac_of_hbm": round(must / (mk * 1e-3) / HBM_BYTES_PER_S, 4),
            "kernel_fp32_madds_per_s": round(n * ntap / (mk * 1e-3), 1),
            "windows_per_s": round(W / (ma * 1e-3), 1)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.resample_out)), exist_ok=True)
    with open(a.resample_out, "w") as f:
        json.dump([line], f, indent=1)


def _rounds(fns, a):
    """{name: [ms per call, ...]}: the functions alternate, a.rounds times; calls per round from one timed call each."""
    iters = {}
    for k, fn in fns.items():
        prime(fn, 0.3)
        iters[k] = max(1, min(a.iters, int(300.0 / max(timed(fn, 1), 1e-3))))
    ms = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters[k]))
    return ms, iters


def _report(metric, workload, ms, iters, extra):
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {"metric": metric, "value": round(med["filtered"], 4), "unit": "ms", "config": {"workload": workload},
            **{f"{k}_ms": [round(t, 4) for t in v] for k, v in ms.items()},
            **{f"{k}_median_ms": round(m, 4) for k, m in med.items()},
            **{f"{k}_spread_ms": round(max(v) - min(v), 4) for k, v in ms.items()},
            "calls_per_round": iters,
            "filtered_over_unfiltered": round(med["filtered"] / med["unfiltered"], 3),
            "added_ms": round(med["filtered"] - med["unfiltered"], 4), **extra}
    if "stock" in med:
        line["stock_over_filtered"] = round(med["stock"] / med["filtered"], 3)
    print(json.dumps(line), flush=True)
    return line


def filter_leg(a):
    """ecg_fir_windows and score_recording(filter=) against the unfiltered path and against stock torch conv1d."""
    from ecg_hip import functional as F
    from ecg_hip.filter import FilterSpec, one_sided
    from ecg_hip.recording import plan_chunks, score_recording, window_plan
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    conv1d, pad = torch.nn.functional.conv1d, torch.nn.functional.pad
    res = []
    for fs, window, spec in ((100, 1000, FilterSpec()), (500, 5000, FilterSpec(notch=50))):
        h = spec.taps(fs)
        c = one_sided(h)
        half = len(c) - 1
        w = torch.from_numpy(h.astype(np.float32)).cuda().reshape(1, 1, -1).expand(LEADS, 1, -1).contiguous()
        rng = np.random.default_rng(fs + 1)
        # (f) a batch of pre-cut windows
        B = a.batch
        d = torch.from_numpy(rng.integers(-3000, 3000, size=(B, window, LEADS)).astype(np.int16)).cuda()
        gain = torch.full((B, LEADS), 1000.0, dtype=torch.float64).cuda()
        base = torch.zeros(B, LEADS, dtype=torch.int32).cuda()

        def filtered():
            return F.fir_windows(F.wfdb16_to_windows(d, gain, base, normalize=False), c, window, 0, 1, 1)[:, 0]

        def kernel_only(p=F.wfdb16_to_windows(d, gain, base, normalize=False)):
            return F.fir_windows(p, c, window, 0, 1, 1, normalize=False)

        def unfiltered():
            return F.wfdb16_to_windows(d, gain, base)

        def stock():
            p = pad(F.wfdb16_to_windows(d, gain, base, normalize=False), (half, half), mode="replicate")
            y = conv1d(p, w, groups=LEADS)
            return F.zscore_per_lead(y, out=y)

        print(f"filter leg: {fs} Hz, half {half}: windows", file=sys.stderr, flush=True)
        # same filter, another summation order and fused multiply-adds: close, not bit-identical
        diff = float((filtered() - stock()).abs().max())
        assert diff <= 1e-3, diff
        ms, iters = _rounds({"filtered": filtered, "unfiltered": unfiltered, "stock": stock, "kernel_only": kernel_only}, a)
        n = B * window * LEADS
        mk = float(np.median(ms["kernel_only"]))
        res.append(_report("fir_windows_ms", f"{B} windows of {LEADS}x{window} at {fs} Hz, {spec!r} (half {half}), "
                           "int16 -> physical -> filtered -> z-scored fp32", ms, iters,
                           {"max_abs_diff_filtered_vs_stock": diff, "half": half,
                            "kernel_fp32_ops_per_s": round(n * (3.0 * half + 1) / (mk * 1e-3), 1),
                            "kernel_tap_pairs_per_s": round(n * float(half) / (mk * 1e-3), 1)}))
        # (g) the one-hour recording
        Ttot, hop = int(a.hours * 3600 * fs), window // 2
        d1 = torch.from_numpy(rng.integers(-3000, 3000, size=(1, Ttot, LEADS)).astype(np.int16)).cuda()
        g1, b1 = gain[:1].contiguous(), base[:1].contiguous()
        plan = window_plan(Ttot, window, hop)
        W, starts = plan[2], torch.tensor(plan[4], device="cuda")
        set_seed(42)
        model = ECGCNN(num_labels=5).cuda().eval()

        def score(flt):
            return score_recording(model, d1, g1, b1, window=window, hop=hop, batch_size=a.batch, fs=fs, filter=flt).logits

        def stock_score():
            p = pad(F.wfdb16_to_windows(d1, g1, b1, normalize=False), (half, half), mode="replicate")
            y = conv1d(p, w, groups=LEADS)[0]                                           # [leads][Ttot]
            out = []
            for _, _, w0, _, Wc, _ in plan_chunks(1, plan, a.batch):
                idx = starts[w0:w0 + Wc, None] + torch.arange(window, device="cuda")[None, :]
                x = y[:, idx].permute(1, 0, 2).contiguous()
                with torch.no_grad():
                    out.append(model(F.zscore_per_lead(x, out=x)))
            return torch.cat(out)

        print(f"filter leg: {fs} Hz, half {half}: score_recording", file=sys.stderr, flush=True)
        fns = {"filtered": lambda: score(c), "unfiltered": lambda: score(None)}
        extra = {"windows": W, "half": half}
        try:
            extra["max_abs_logit_diff_filtered_vs_stock"] = float((score(c)[0] - stock_score()).abs().max())
            fns["stock"] = stock_score
        except RuntimeError as e:           # stock torch may have no plan for a filter this long on a signal this long
            extra["stock_error"] = str(e).splitlines()[0][:200]
        ms, iters = _rounds(fns, a)
        extra["windows_per_s"] = round(W / (float(np.median(ms["filtered"])) * 1e-3), 1)
        res.append(_report("score_recording_filtered_ms", f"ECGCNN(5) score_recording, {a.hours:g} h at {fs} Hz, window "
                           f"{window}, hop {hop}, {W} windows in chunks of {a.batch}, fp32, no CAMs, {spec!r}", ms, iters,
                           extra))
    return res


def decode_leg(a):
    """ecg_wfdb_decode16 against the same decode in torch ops on the device and in numpy on the host."""
    import tempfile
    from ecg_hip import functional as F
    from ecg_hip import wfdbraw
    from ecg_hip.recording import score_wfdb_record
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    res = []
    a = argparse.Namespace(**{**vars(a), "iters": max(a.iters, 2000)})     # a call is tens of microseconds: _rounds caps a round at 0.3 s
    tmp = tempfile.mkdtemp(prefix="bench_decode_")
    rng = np.random.default_rng(212)
    names = list(wfdbraw.PTBXL_LEADS) + ["vx", "vy", "vz"]
    order = rng.permutation(15)
    for fmt, fs, n_sig, window in ((212, 500, LEADS, 5000), (16, 1000, 15, 5000)):
        Ttot = int(a.hours * 3600 * fs)
        lim = 2047 if fmt == 212 else 3000
        d = rng.integers(-lim, lim, size=(Ttot, n_sig)).astype(np.int16)
        path = os.path.join(tmp, f"rec{fmt}")
        sig_names = list(wfdbraw.PTBXL_LEADS) if n_sig == LEADS else [names[i] for i in order]
        wfdbraw.write_raw_record(path, d, fs, np.full(n_sig, 1000.0), np.zeros(n_sig, np.int32), fmt=fmt, sig_names=sig_names)
        rec = wfdbraw.read_raw_record(path)
        leads = None if n_sig == LEADS else wfdbraw.PTBXL_LEADS
        cols = list(range(n_sig)) if leads is None else wfdbraw.select_leads(rec, leads)
        raw_host = rec.files[0]
        raw = torch.from_numpy(raw_host).cuda()
        idx = torch.tensor(cols, device="cuda")

        def kernel():
            return F.wfdb_decode16([raw], rec.signals, Ttot, cols)

        def decode_ops(b, xp):                      # the same statements for torch (device) and numpy (host)
            if fmt == 16:
                return b.view(xp.int16).reshape(Ttot, n_sig)
            b = b[:3 * (Ttot * n_sig // 2)].reshape(-1, 3).astype(np.int32) if xp is np else \
                b[:3 * (Ttot * n_sig // 2)].view(-1, 3).to(torch.int32)
            even = b[:, 0] | ((b[:, 1] & 0x0F) << 8)
            odd = b[:, 2] | ((b[:, 1] & 0xF0) << 4)
            v = xp.stack([even, odd], 1).reshape(-1)
            v = (v ^ 0x800) - 0x800
            v = xp.where(v == -2048, -32768, v)
            return (v.astype(np.int16) if xp is np else v.to(torch.int16)).reshape(Ttot, n_sig)

        def stock():
            v = decode_ops(raw, torch)
            return v if leads is None else v.index_select(1, idx)

        def host_numpy():
            v = decode_ops(raw_host, np)
            return torch.from_numpy(np.ascontiguousarray(v if leads is None else v[:, cols])).cuda()

        want = d if leads is None else d[:, cols]
        assert Ttot * n_sig % 2 == 0
        for fn in (kernel, stock, host_numpy):
            assert np.array_equal(fn().cpu().numpy(), want), fn.__name__
        print(f"decode leg: format {fmt}, {Ttot} x {n_sig}", file=sys.stderr, flush=True)
        ms, iters = _rounds({"kernel": kernel, "torch": stock, "numpy": host_numpy}, a)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        n_out = Ttot * len(cols)
        must = n_out * (3.5 if fmt == 212 else 4.0)
        # end to end: header, file read, upload, decode, checksum, scoring
        set_seed(42)
        model = ECGCNN(num_labels=5).cuda().eval()

        def e2e():
            t0 = time.perf_counter()
            score_wfdb_record(path, model, leads=leads, window=window, batch_size=a.batch)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        e2e()
        e2e_ms = [e2e() for _ in range(max(3, a.rounds // 2))]
        line = {"metric": "wfdb_decode16_ms", "value": round(med["kernel"], 4), "unit": "ms",
                "config": {"workload": f"{a.hours:g} h at {fs} Hz, format {fmt}, {n_sig} signals in the file, {len(cols)} decoded"
                                       f"{'' if leads is None else ' (picked by name, reordered)'}: {raw_host.size} bytes -> "
                                       f"int16 [{Ttot}][{len(cols)}]"},
                **{f"{k}_ms": [round(t, 4) for t in v] for k, v in ms.items()},
                **{f"{k}_median_ms": round(m, 4) for k, m in med.items()},
                **{f"{k}_spread_ms": round(max(v) - min(v), 4) for k, v in ms.items()},
                "calls_per_round": iters, "torch_over_kernel": round(med["torch"] / med["kernel"], 3),
                "numpy_over_kernel": round(med["numpy"] / med["kernel"], 3),
                "kernel_bytes_it_must_move": int(must), "kernel_GBps_of_those_bytes": round(must / (med["kernel"] * 1e-3) / 1e9, 1),
                "kernel_frac_of_hbm": round(must / (med["kernel"] * 1e-3) / HBM_BYTES_PER_S, 4),
                "score_wfdb_record_ms": [round(t, 2) for t in e2e_ms],
                "score_wfdb_record_median_ms": round(float(np.median(e2e_ms)), 2),
                "kernel_share_of_score_wfdb_record": round(med["kernel"] / float(np.median(e2e_ms)), 5)}
        print(json.dumps(line), flush=True)
        res.append(line)
        for ext in (".hea", ".dat"):
            os.remove(path + ext)
    os.rmdir(tmp)
    return res


def quality_table_torch(d, window, hop, lo=-32767, hi=32767):
    """The table of ecg_wfdb16_quality for one recording d int16 [Ttot, leads] in torch tensor ops (regular windows only)."""
    v16 = d.unfold(0, window, hop)                                      # [W][leads][T], a view
    v = v16.to(torch.int32)
    valid = v16 != -32768
    zero = torch.zeros((), dtype=torch.int32, device=d.device)
    vv = torch.where(valid, v, zero)
    t = torch.arange(window, device=d.device, dtype=torch.int32)
    change = torch.ones_like(valid)
    change[..., 1:] = v16[..., 1:] != v16[..., :-1]
    run_start = torch.where(change, t, zero).cummax(-1).values          # where the run a sample belongs to began
    pair = valid[..., 1:] & valid[..., :-1]
    step = torch.where(pair, (v[..., 1:] - v[..., :-1]).abs(), zero)
    i64 = torch.int64
    return torch.stack([(~valid).sum(-1), torch.where(valid, v, zero + 32767).amin(-1).to(i64),
                        torch.where(valid, v, zero - 32768).amax(-1).to(i64), vv.sum(-1, dtype=i64),
                        (vv.to(i64) * vv).sum(-1), (t - run_start + 1).amax(-1).to(i64),
                        (valid & ((v <= lo) | (v >= hi))).sum(-1), pair.sum(-1), step.sum(-1, dtype=i64),
                        step.amax(-1).to(i64) if window > 1 else torch.zeros_like(pair.sum(-1))], -1)[None]


def quality_leg(a):
    """ecg_wfdb16_quality against the same table in torch ops, and what quality= adds to score_recording."""
    from ecg_hip import functional as F
    from ecg_hip.recording import score_recording, window_plan
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    res = []
    for fs, window in ((100, 1000), (500, 5000)):
        Ttot, hop = int(a.hours * 3600 * fs), window // 2
        rng = np.random.default_rng(fs + 2)
        h = rng.integers(-3000, 3000, size=(1, Ttot, LEADS)).astype(np.int16)
        for _ in range(200):                            # flat stretches, rails and invalid samples, so that no field is trivial
            t, c, n = int(rng.integers(0, Ttot - 400)), int(rng.integers(LEADS)), int(rng.integers(2, 400))
            h[0, t:t + n, c] = rng.choice([0, 32767, -32767, -32768, int(rng.integers(-3000, 3000))])
        d = torch.from_numpy(h).cuda()
        gain = torch.full((1, LEADS), 1000.0, dtype=torch.float64).cuda()
        base = torch.zeros(1, LEADS, dtype=torch.int32).cuda()
        first, hop, W, last, _ = window_plan(Ttot, window, hop)
        assert last == -1                               # the torch form below cuts regular windows only
        set_seed(42)
        model = ECGCNN(num_labels=5).cuda().eval()

        def kernel():
            return F.wfdb16_quality(d, window, first, hop, W, last)

        def stock():
            return quality_table_torch(d[0], window, hop)

        def score(q):
            return score_recording(model, d, gain, base, window=window, hop=hop, batch_size=a.batch, fs=fs, quality=q).prob_max

        assert torch.equal(kernel(), stock())
        print(f"quality leg: {fs} Hz, {W} windows of {LEADS}x{window}", file=sys.stderr, flush=True)
        big = argparse.Namespace(**{**vars(a), "iters": max(a.iters, 2000)})       # a launch is microseconds
        ms, iters = _rounds({"kernel": kernel, "torch": stock}, big)
        ms2, iters2 = _rounds({"gated": lambda: score(True), "ungated": lambda: score(None)}, a)
        ms.update(ms2), iters.update(iters2)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        must = W * window * LEADS * 2
        line = {"metric": "wfdb16_quality_ms", "value": round(med["kernel"], 4), "unit": "ms",
                "config": {"workload": f"{a.hours:g} h, {LEADS} leads at {fs} Hz (Ttot {Ttot}), window {window}, hop {hop}, "
                                       f"{W} windows: int16 in place -> int64 [1][{W}][{LEADS}][10]; score_recording: "
                                       f"ECGCNN(5), chunks of {a.batch}, fp32, no CAMs"},
                **{f"{k}_ms": [round(t, 4) for t in v] for k, v in ms.items()},
                **{f"{k}_median_ms": round(m, 4) for k, m in med.items()},
                **{f"{k}_spread_ms": round(max(v) - min(v), 4) for k, v in ms.items()},
                "calls_per_round": iters, "torch_over_kernel": round(med["torch"] / med["kernel"], 3),
                "kernel_bytes_it_must_read": int(must), "kernel_GBps_of_those_bytes": round(must / (med["kernel"] * 1e-3) / 1e9, 1),
                "kernel_frac_of_hbm": round(must / (med["kernel"] * 1e-3) / HBM_BYTES_PER_S, 4),
                "gated_over_ungated": round(med["gated"] / med["ungated"], 4),
                "added_ms": round(med["gated"] - med["ungated"], 4),
                "kernel_share_of_gated_score_recording": round(med["kernel"] / med["gated"], 5)}
        print(json.dumps(line), flush=True)
        res.append(line)
    return res


def beats_torch(d, s, h, ref, blk, num, den, g_min):
    """The beat list of ecg_wfdb16_beats for one recording d int16 [Ttot, leads] in torch tensor ops on d's device: cumsum
    for g, a sort of five shifted copies for the block medians, max_pool1d (float64: g < 2^29 is exact) for the windowed
    maxima, nonzero for the list."""
    Ttot, i64 = d.shape[0], torch.int64
    v, valid = d.to(torch.int32), d != -32768
    f = torch.zeros(Ttot, dtype=i64, device=d.device)
    if Ttot > 2 * s:
        both = valid[2 * s:] & valid[:Ttot - 2 * s]
        f[s:Ttot - s] = torch.where(both, (v[2 * s:] - v[:Ttot - 2 * s]).abs(), torch.zeros_like(v[2 * s:])).sum(1, dtype=i64)
    c = torch.cat([f.new_zeros(1), f.cumsum(0)])
    n = torch.arange(Ttot, device=d.device)
    g = c[(n + h).clamp(max=Ttot - 1) + 1] - c[(n - h).clamp(min=0)]
    nblk = -(-Ttot // blk)
    M = torch.cat([g, g.new_zeros(nblk * blk - Ttot)]).view(nblk, blk).amax(1)
    big = torch.iinfo(i64).max
    five = torch.cat([M.new_full((2,), big), M, M.new_full((2,), big)]).unfold(0, 5, 1).sort(-1).values
    k = (five != big).sum(-1)                                           # the neighbours inside [0, nblk)
    med = five.gather(1, ((k - 1) // 2)[:, None])[:, 0]
    thr = torch.clamp((num * med) // den, min=int(g_min))
    edge = g.new_full((ref,), -1)
    wmax = torch.nn.functional.max_pool1d(torch.cat([edge, g, edge]).double()[None, None], ref, 1)[0, 0]
    left, right, gd = wmax[:Ttot], wmax[ref + 1:ref + 1 + Ttot], g.double()
    return torch.nonzero((g >= thr[n // blk]) & (gd > left) & (gd >= right))[:, 0]


def _pulse_recording(a, fs):
    """-> (d int16 [1, Ttot, LEADS], gain, baseline) on the device: R-like pulses (sigma 12 ms, 0.3-1.5 mV, a sign per lead)
    every 0.7-0.9 s in 0.02 mV of noise, 1000 counts per mV."""
    Ttot = int(a.hours * 3600 * fs)
    rng = np.random.default_rng(fs + 3)
    at = np.cumsum(rng.uniform(0.7, 0.9, size=int(a.hours * 3600 / 0.7)) * fs).astype(np.int64)
    train = np.zeros(Ttot)
    train[at[at < Ttot - fs]] = 1.0
    k = np.arange(-int(0.06 * fs), int(0.06 * fs) + 1)
    shape = np.convolve(train, np.exp(-0.5 * (k / (0.012 * fs)) ** 2), mode="same")
    amp = rng.choice([-1.0, 1.0], size=LEADS) * rng.uniform(300, 1500, size=LEADS)
    x = shape[:, None] * amp[None, :] + 20.0 * rng.standard_normal((Ttot, LEADS))
    d = torch.from_numpy(np.round(x).astype(np.int16)[None]).cuda()
    return d, torch.full((1, LEADS), 1000.0, dtype=torch.float64).cuda(), torch.zeros(1, LEADS, dtype=torch.int32).cuda()


def beats_leg(a):
    """ecg_wfdb16_beats + ecg_beats_rhythm against the same detector in torch ops, and what beats= adds to score_recording."""
    from ecg_hip import functional as F
    from ecg_hip.beats import BeatSpec
    from ecg_hip.recording import score_recording, window_plan
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    res = []
    for fs, window in ((100, 1000), (500, 5000)):
        Ttot, hop = int(a.hours * 3600 * fs), window // 2
        d, gain, base = _pulse_recording(a, fs)
        p = BeatSpec().params(fs, gain)
        g_min = p["g_min"].cuda()
        first, hop, W, last, _ = window_plan(Ttot, window, hop)
        set_seed(42)
        model = ECGCNN(num_labels=5).cuda().eval()

        def detect():
            return F.wfdb16_beats(d, p["s"], p["h"], p["ref"], p["blk"], p["num"], p["den"], g_min)

        def kernel():
            b, n = detect()
            return F.beats_rhythm(b, n, Ttot, window, first, hop, W, last, 1, 1, p["nn_delta"])

        def stock():
            return beats_torch(d[0], p["s"], p["h"], p["ref"], p["blk"], p["num"], p["den"], int(g_min[0]))

        def score(b):
            return score_recording(model, d, gain, base, window=window, hop=hop, batch_size=a.batch, fs=fs, beats=b).prob_max

        b, n = detect()
        want = stock()
        assert int(n[0]) == want.numel() and torch.equal(b[0, :int(n[0])].long(), want)
        print(f"beats leg: {fs} Hz, Ttot {Ttot}, {int(n[0])} beats, {W} windows", file=sys.stderr, flush=True)
        big = argparse.Namespace(**{**vars(a), "iters": max(a.iters, 500)})
        ms, iters = _rounds({"kernel": kernel, "detect": detect, "torch": stock}, big)
        ms2, iters2 = _rounds({"with_beats": lambda: score(True), "without": lambda: score(None)}, a)
        ms.update(ms2), iters.update(iters2)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        must = Ttot * LEADS * 2
        line = {"metric": "wfdb16_beats_rhythm_ms", "value": round(med["kernel"], 4), "unit": "ms",
                "config": {"workload": f"{a.hours:g} h, {LEADS} leads at {fs} Hz (Ttot {Ttot}), BeatSpec() defaults "
                                       f"(s {p['s']}, h {p['h']}, ref {p['ref']}, blk {p['blk']}), {int(n[0])} beats; table over "
                                       f"{W} windows of {window}, hop {hop}; kernel: wfdb16_beats + beats_rhythm, detect: "
                                       f"wfdb16_beats alone, torch: the list in tensor ops (no table); score_recording: ECGCNN(5), "
                                       f"chunks of {a.batch}, fp32, no CAMs"},
                **{f"{k}_ms": [round(t, 4) for t in v] for k, v in ms.items()},
                **{f"{k}_median_ms": round(m, 4) for k, m in med.items()},
                **{f"{k}_spread_ms": round(max(v) - min(v), 4) for k, v in ms.items()},
                "calls_per_round": iters, "torch_over_kernel": round(med["torch"] / med["kernel"], 3),
                "stream_bytes": int(must), "detect_GBps_of_the_stream": round(must / (med["detect"] * 1e-3) / 1e9, 1),
                "with_over_without": round(med["with_beats"] / med["without"], 4),
                "added_ms": round(med["with_beats"] - med["without"], 4)}
        print(json.dumps(line), flush=True)
        res.append(line)
    return res


def template_leg(a):
    """ecg_beats_sum / ecg_beats_match / ecg_beats_series_mean, the sums in torch ops, and what template= adds to
    score_recording with beats=True."""
    from ecg_hip import functional as F
    from ecg_hip import template as T
    from ecg_hip.beats import BeatSpec
    from ecg_hip.recording import score_recording
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    res, K = [], 5
    for fs, window in ((100, 1000), (500, 5000)):
        Ttot, hop = int(a.hours * 3600 * fs), window // 2
        d, gain, base = _pulse_recording(a, fs)
        bp = BeatSpec().params(fs, gain)
        b, n = F.wfdb16_beats(d, bp["s"], bp["h"], bp["ref"], bp["blk"], bp["num"], bp["den"], bp["g_min"].cuda())
        p = T.TemplateSpec().params(fs)
        pre, post, L = p["pre"], p["post"], p["pre"] + p["post"] + 1
        tm = T.mean_template(*F.beats_sum(d, b, n, p["match_pre"], p["match_post"]), centre=True)
        series = torch.randn(1, K, Ttot, device="cuda")
        set_seed(42)
        model = ECGCNN(num_labels=5).cuda().eval()
        cap = b.shape[1]
        x = b[0].long()
        whole = (torch.arange(cap, device="cuda") < n[0]) & (x - pre >= 0) & (x + post < Ttot)
        t = torch.arange(L, device="cuda")

        def sums():
            return F.beats_sum(d, b, n, pre, post)

        def match():
            return F.beats_match(d, b, n, tm, p["match_pre"], p["match_post"], p["J"])

        def mean():
            return F.beats_series_mean(series, b, n, Ttot, pre, post)

        def sums_torch():
            idx = (x[:, None] - pre + t[None, :]).clamp(0, Ttot - 1)            # the index tensor [beats][Lseg]
            seg = d[0][idx]                                                     # [beats][Lseg][leads]
            valid = (seg != -32768) & whole[:, None, None]
            return torch.where(valid, seg, torch.zeros_like(seg)).sum(0, dtype=torch.int64), valid.sum(0, dtype=torch.int32)

        def mean_torch():
            idx = (x[:, None] - pre + t[None, :]).clamp(0, Ttot - 1)
            seg = series[0][:, idx] * whole[None, :, None]                      # [K][beats][Lseg]
            return seg.sum(1) / whole.sum()

        def score(tp):
            return score_recording(model, d, gain, base, window=window, hop=hop, batch_size=a.batch, fs=fs, beats=True,
                                   template=tp).prob_max

        (s1, c1), (s2, c2) = sums(), sums_torch()
        assert torch.equal(s1[0], s2) and torch.equal(c1[0], c2)
        assert torch.allclose(mean()[0][0], mean_torch(), rtol=1e-3, atol=1e-3)
        taking = int(whole.sum())
        print(f"template leg: {fs} Hz, Ttot {Ttot}, {int(n[0])} beats, Lseg {L}, J {p['J']}", file=sys.stderr, flush=True)
        big = argparse.Namespace(**{**vars(a), "iters": max(a.iters, 500)})
        ms, iters = _rounds({"sum": sums, "match": match, "series_mean": mean, "sum_torch": sums_torch,
                             "series_mean_torch": mean_torch}, big)
        ms2, iters2 = _rounds({"with_template": lambda: score(True), "beats_only": lambda: score(None)}, a)
        ms.update(ms2), iters.update(iters2)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        must = taking * L * LEADS * 2 + cap * 4
        line = {"metric": "beats_sum_ms", "value": round(med["sum"], 4), "unit": "ms",
                "config": {"workload": f"{a.hours:g} h, {LEADS} leads at {fs} Hz (Ttot {Ttot}), {int(n[0])} beats ({taking} with a "
                                       f"whole segment), TemplateSpec() defaults: display Lseg {L}, match Lseg "
                                       f"{p['match_pre'] + p['match_post'] + 1}, J {p['J']}; series_mean: {K} fp32 series at ratio 1/1; "
                                       f"torch: index tensor + gather + masked sum; score_recording: ECGCNN(5), chunks of "
                                       f"{a.batch}, fp32, no CAMs, beats=True with and without template=True"},
                **{f"{k}_ms": [round(v_, 4) for v_ in v] for k, v in ms.items()},
                **{f"{k}_median_ms": round(m, 4) for k, m in med.items()},
                **{f"{k}_spread_ms": round(max(v) - min(v), 4) for k, v in ms.items()},
                "calls_per_round": iters, "sum_torch_over_kernel": round(med["sum_torch"] / med["sum"], 3),
                "series_mean_torch_over_kernel": round(med["series_mean_torch"] / med["series_mean"], 3),
                "sum_bytes_it_must_read": int(must), "sum_GBps_of_those_bytes": round(must / (med["sum"] * 1e-3) / 1e9, 1),
                "sum_frac_of_hbm": round(must / (med["sum"] * 1e-3) / HBM_BYTES_PER_S, 4),
                "with_over_beats_only": round(med["with_template"] / med["beats_only"], 4),
                "added_ms": round(med["with_template"] - med["beats_only"], 4)}
        print(json.dumps(line), flush=True)
        res.append(line)
    return res


_SECTIONS = ("filter", "decode", "quality", "beats", "template")


def _write(path, lines=None, **sections):
    """profiles/recording_bench.json: the recording leg's lines, then {"filter": [...]}, {"decode": [...]},
    {"quality": [...]}, {"beats": [...]} and {"template": [...]}; a leg replaces its own part."""
    old = []
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    kept = {k: e for e in old if isinstance(e, dict) for k in _SECTIONS if k in e}
    old_lines = [e for e in old if not (isinstance(e, dict) and any(k in e for k in _SECTIONS))]
    for k, v in sections.items():
        kept[k] = {k: v}
    out = (old_lines if lines is None else lines) + [kept[k] for k in _SECTIONS if k in kept]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recording_bench.json"))
    ap.add_argument("--legs", default="recording,resample")
    ap.add_argument("--resample-out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_recording: no GPU visible")
    from ecg_hip import _lib
    from ecg_hip import functional as F
    from ecg_hip.recording import score_recording, window_plan
    from src.models.ecg_cnn import ECGCNN
    from src.utils.seed import set_seed
    _lib.call("ecg_check_device")
    if "resample" in a.legs.split(","):
        resample_leg(a)
    if "filter" in a.legs.split(","):
        _write(a.out, filter=filter_leg(a))
    if "decode" in a.legs.split(","):
        _write(a.out, decode=decode_leg(a))
    if "quality" in a.legs.split(","):
        _write(a.out, quality=quality_leg(a))
    if "beats" in a.legs.split(","):
        _write(a.out, beats=beats_leg(a))
    if "template" in a.legs.split(","):
        _write(a.out, template=template_leg(a))
    if "recording" not in a.legs.split(","):
        return
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
    _write(a.out, lines=res)


if __name__ == "__main__":
    main()
