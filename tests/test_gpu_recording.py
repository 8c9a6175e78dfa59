"""GPU checks of the continuous-recording path: the sliding input step is BIT-IDENTICAL to the pre-cut one on copied
slices (and to the oracle, and to the reference's committed demo windows), the overlap mean equals its numpy fp32
definition bit for bit, and score_recording equals a manual loop over the same chunks."""
import numpy as np
import pytest
import torch

from input_util import _model, dev, hip, host  # noqa: F401
from util import golden

from oracle import input_oracle as io_ref
from test_recording_host import overlap_mean_ref

pytestmark = pytest.mark.gpu


def recording(R, Ttot, leads, seed):
    """The generator of test_wfdb16_to_windows_vs_oracle_exact: random int16, extreme samples, mixed gains, baselines."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-4000, 4000, size=(R, Ttot, leads)).astype(np.int16)
    d[0, 0, 0], d[-1, -1, -1] = 32767, -32767
    gain = rng.choice([200.0, 1000.0, 1000.5, 3.3333e3], size=(R, leads))
    base = rng.integers(-50, 50, size=(R, leads)).astype(np.int32)
    return d, gain, base


def cut(d, gain, base, starts, T):
    """The copy a user makes today: every window's slice, [R*W][T][leads], with its recording's calibration."""
    R = d.shape[0]
    ds = np.stack([d[r, s:s + T] for r in range(R) for s in starts])
    return ds, np.repeat(gain, len(starts), axis=0), np.repeat(base, len(starts), axis=0)


CASES = [(2, 700, 12, 256, 100, "shift"),       # shifted tail
         (1, 3000, 12, 1000, 333, "drop"),      # odd starts, fused path
         (1, 4100, 12, 1345, 451, "shift"),     # streaming path, T % 4 == 1
         (1, 12000, 12, 5000, 2500, "drop"),    # long window
         (3, 200, 1, 63, 7, "shift"),           # one lead
         (1, 130, 16, 128, 1, "drop"),          # 16 leads, hop 1
         (2, 1000, 12, 1000, 1000, "drop"),     # W = 1
         (1, 900, 3, 100, 250, "drop")]         # gaps, hop > T


@pytest.mark.parametrize("case", CASES)
def test_sliding_windows_bit_identical_to_cut_windows(hip, case):
    R, Ttot, leads, T, hop, tail = case
    d, gain, base = recording(R, Ttot, leads, R * 7 + Ttot + leads)
    dd, dg, db = dev(d), dev(gain), dev(base)
    x, stats, plan = hip.wfdb16_to_windows_sliding(dd, dg, db, T, hop, tail, return_stats=True)
    starts = plan[4]
    W = len(starts)
    assert tuple(x.shape) == (R, W, leads, T) and tuple(stats.shape) == (R * W * leads, 2)
    # the device slices through the pre-cut entry point
    ds = torch.stack([dd[r, s:s + T] for r in range(R) for s in starts])
    rep = lambda t: t.repeat_interleave(W, dim=0)                                        # noqa: E731
    want, want_stats = hip.wfdb16_to_windows(ds, rep(dg), rep(db), return_stats=True)
    assert np.array_equal(host(x).reshape(R * W, leads, T), host(want))
    assert np.array_equal(host(stats), host(want_stats))
    phys, plan2 = hip.wfdb16_to_windows_sliding(dd, dg, db, T, hop, tail, normalize=False)
    assert plan2 == plan
    assert np.array_equal(host(phys).reshape(R * W, leads, T), host(hip.wfdb16_to_windows(ds, rep(dg), rep(db), normalize=False)))
    # ... and the oracle on the same slices
    hs, hg, hb = cut(d, gain, base, starts, T)
    assert np.array_equal(host(phys).reshape(R * W, leads, T),
                          np.stack([np.ascontiguousarray(io_ref.load_ecg(hs[i], hg[i], hb[i])) for i in range(R * W)]))
    if leads > 1:
        assert np.array_equal(host(x).reshape(R * W, leads, T), io_ref.windows_from_wfdb16(hs, hg, hb))
    if W == 1 and Ttot == T:
        whole, whole_stats = hip.wfdb16_to_windows(dd, dg, db, return_stats=True)
        assert np.array_equal(host(x)[:, 0], host(whole)) and np.array_equal(host(stats), host(whole_stats))


def test_reference_windows_out_of_one_concatenated_recording(hip):
    g = golden("g8_input_pipeline")
    gain, base = g["gain"], g["baseline"].astype(np.int32)
    assert (gain == gain[0]).all() and (base == base[0]).all()          # one calibration: the three records concatenate
    d = dev(g["d"].reshape(1, 15000, 12))
    for hop, pick in ((5000, [0, 1, 2]), (2500, [0, 2, 4])):
        x, plan = hip.wfdb16_to_windows_sliding(d, dev(gain[:1]), dev(base[:1]), 5000, hop)
        assert plan[4] == tuple(range(0, 10001, hop))
        assert np.array_equal(host(x)[0, pick], g["x"])


def test_invalid_sample_poisons_exactly_the_windows_over_it(hip):
    d, gain, base = recording(1, 700, 12, 5)
    args = (dev(gain), dev(base), 256, 100)
    clean, plan = hip.wfdb16_to_windows_sliding(dev(d), *args)
    assert plan[4] == (0, 100, 200, 300, 400, 444)
    d[0, 250, 3] = -32768                                    # inside windows 0, 1, 2 (their overlap), before window 3
    x = host(hip.wfdb16_to_windows_sliding(dev(d), *args)[0])[0]
    clean = host(clean)[0]
    for w in range(6):
        if w <= 2:
            assert np.isnan(x[w, 3]).all()
            assert np.array_equal(np.delete(x[w], 3, axis=0), np.delete(clean[w], 3, axis=0))
        else:
            assert np.array_equal(x[w], clean[w])


# (R, W, K, T, Ttot, hop, tail)
@pytest.mark.parametrize("case", [(2, 6, 5, 256, 700, 100, "shift"), (1, 4, 1, 100, 900, 250, "drop"),
                                  (1, 3, 2, 63, 77, 7, "shift"), (1, 3, 8, 128, 130, 1, "shift")])
def test_overlap_mean_equals_the_numpy_definition(hip, case):
    from ecg_hip.recording import window_plan
    R, W, K, T, Ttot, hop, tail = case
    plan = window_plan(Ttot, T, hop, tail)
    assert plan[2] == W
    v = np.random.default_rng(Ttot).standard_normal((R, W, K, T)).astype(np.float32)
    want, want_cover = overlap_mean_ref(v, plan[4], Ttot)
    out, cover = hip.overlap_mean(dev(v), plan, Ttot, return_cover=True)
    assert np.array_equal(host(out), want) and np.array_equal(host(cover), want_cover)
    if hop > T:
        assert (want_cover == 0).any() and (host(out)[:, :, want_cover == 0] == 0).all()
    again = hip.overlap_mean(dev(v), plan, Ttot)
    assert torch.equal(again, out)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cnn", "multimodal"])
def test_score_recording_equals_a_manual_loop(hip, name):
    import ecg_hip
    from ecg_hip.recording import score_recording
    model = _model(name)
    R, Ttot, window, hop, K = 2, 3000, 1000, 500, [0, 3]
    rng = np.random.default_rng(21)
    d = rng.integers(-3000, 3000, size=(R, Ttot, 12)).astype(np.int16)
    gain, base = np.full((R, 12), 1000.0), rng.integers(-9, 9, size=(R, 12)).astype(np.int32)
    xd = torch.rand(R, 5, generator=torch.Generator().manual_seed(3)).cuda() if name == "multimodal" else None
    dd, dg, db = dev(d), dev(gain), dev(base)
    x, plan = hip.wfdb16_to_windows_sliding(dd, dg, db, window, hop)
    W = plan[2]
    assert W == 5

    def manual(chunks, cams):
        """chunks: (r0, r1, w0, w1) in the order score_recording walks them."""
        logits, cam = torch.empty(R, W, 5, device="cuda"), torch.empty(R, W, len(K), window, device="cuda")
        with torch.no_grad():
            for r0, r1, w0, w1 in chunks:
                xc = x[r0:r1, w0:w1].reshape(-1, 12, window)
                dc = None if xd is None else xd[r0:r1].repeat_interleave(w1 - w0, dim=0)
                if cams:
                    c, lg = ecg_hip.grad_cam(model, xc, dc, class_idx=K, signal_length=window, normalize=None,
                                             return_logits=True)
                    cam[r0:r1, w0:w1] = c.view(r1 - r0, w1 - w0, len(K), window)
                else:
                    lg = model(xc) if dc is None else model(xc, dc)
                logits[r0:r1, w0:w1] = lg.view(r1 - r0, w1 - w0, 5)
        return logits, cam

    # batch_size 4 < W: one recording per call, chunked over w;  batch_size 16: both recordings in one call
    for bs, chunks in ((4, [(0, 1, 0, 4), (0, 1, 4, 5), (1, 2, 0, 4), (1, 2, 4, 5)]), (16, [(0, 2, 0, 5)])):
        s = score_recording(model, dd, dg, db, window=window, hop=hop, batch_size=bs, x_demo=xd)
        want, _ = manual(chunks, False)
        assert s.starts == plan[4] and s.cam is None and s.cover is None
        assert torch.equal(s.logits, want) and torch.equal(s.prob, hip.sigmoid(want))
        assert bool(s.finite.all())
        assert torch.equal(s.prob_max, s.prob.amax(1)) and torch.equal(s.prob_mean, s.prob.mean(1))
        sc = score_recording(model, dd, dg, db, window=window, hop=hop, batch_size=bs, x_demo=xd, cam_classes=K)
        want, wcam = manual(chunks, True)
        assert torch.equal(sc.logits, want)
        assert torch.equal(sc.cam, hip.overlap_mean(wcam, plan, Ttot))
        ref_cam, ref_cover = overlap_mean_ref(host(wcam), plan[4], Ttot)
        assert np.array_equal(host(sc.cam), ref_cam) and np.array_equal(host(sc.cover), ref_cover)
        assert tuple(sc.cam.shape) == (R, len(K), Ttot)
    # per-record normalisation: min-max over the covered samples (all of them with tail="shift")
    sn = score_recording(model, dd, dg, db, window=window, hop=hop, batch_size=16, x_demo=xd, cam_classes=K,
                         cam_normalize="record")
    raw = host(sc.cam)
    lo, hi = raw.min(-1, keepdims=True), raw.max(-1, keepdims=True)
    live = (hi - lo)[..., 0] > 0
    assert live.any()
    # (one correctly rounded fp32 subtraction and division per sample on either side: 2 ulp covers a differing last bit)
    np.testing.assert_allclose(host(sn.cam)[live], ((raw - lo) / np.where(hi - lo > 0, hi - lo, 1))[live], rtol=2.4e-7, atol=0)
    assert host(sn.cam)[live].min() == 0 and host(sn.cam)[live].max() == 1
    # a 2-D recording is one recording
    s1 = score_recording(model, dd[0], dg[0], db[0], window=window, hop=hop, batch_size=16,
                         x_demo=None if xd is None else xd[:1])
    assert tuple(s1.logits.shape) == (1, W, 5) and torch.equal(s1.logits[0], s.logits[0])


@pytest.mark.parametrize("R,batch", [(1, 2), (3, 16)])
def test_score_recording_launches_what_the_plan_says(hip, monkeypatch, R, batch):
    """The input-step launches of one score_recording call, in order, are what plan_chunks says: without filter= one
    normalising ecg_wfdb16_windows[_resampled] per chunk; with filter= one whole-recording launch of it (W = 1, stats NULL)
    per distinct (r0, r1) group and one ecg_fir_windows per chunk; ecg_wfdb16_quality once and first when quality is set;
    ecg_windows_overlap_mean once and last when CAMs are asked for; nothing else of the input step.  The results of a launch
    made once per chunk instead of once per group are bit-identical, so only the launch list can tell.
    (1, 2): 6 windows in 3 chunks of one group; (3, 16): groups of two recordings, 2 chunks."""
    import sys

    from ecg_hip import _lib
    from ecg_hip.recording import plan_chunks, score_recording, window_plan
    model = _model("cnn")
    window, taps = 200, np.array([0.25, 0.5, 0.25])
    stats_at = {"ecg_wfdb16_windows": 4, "ecg_wfdb16_windows_resampled": 5, "ecg_fir_windows": 3}     # (W follows 7 later)
    others = ("ecg_wfdb16_quality", "ecg_windows_overlap_mean", "ecg_wfdb16_physical", "ecg_wfdb16_zscore", "ecg_zscore_rows",
              "ecg_wfdb_decode16")
    seen, raw = [], _lib.call

    def spy(name, *args):
        if name in stats_at:
            seen.append((name, args[stats_at[name]] is not None, args[stats_at[name] + 7]))
        elif name in others:
            seen.append((name, None, None))
        raw(name, *args)

    plan = window_plan(700, window, window // 2)
    chunks = plan_chunks(R, plan, batch)
    groups = {(c[0], c[1]) for c in chunks}
    assert plan[2] == 6 and (len(chunks), len(groups)) == {1: (3, 1), 3: (2, 2)}[R]
    rate = dict(fs=250, model_fs=100)
    for kw in (dict(), rate, dict(filter=taps), dict(filter=taps, quality=True, cam_classes=[0, 1], **rate)):
        Ttot = 1750 if "fs" in kw else 700          # 1750 samples at 250 Hz are 700 on the model's axis
        d, gain, base = recording(R, Ttot, 12, 50 + R)
        dd, dg, db = dev(d), dev(gain), dev(base)
        del seen[:]
        with monkeypatch.context() as m:            # every name the package's modules hold the ABI call under
            for mod in [v for k, v in sys.modules.items() if k == "ecg_hip" or k.startswith("ecg_hip.")]:
                for attr, val in list(vars(mod).items()):
                    if val is raw:
                        m.setattr(mod, attr, spy)
            s = score_recording(model, dd, dg, db, window=window, batch_size=batch, **kw)
        assert s.starts == plan[4]
        cut = "ecg_wfdb16_windows_resampled" if "fs" in kw else "ecg_wfdb16_windows"
        want, group = [("ecg_wfdb16_quality", None, None)] if kw.get("quality") else [], None
        for r0, r1, _, _, Wc, _ in chunks:
            if "filter" in kw:
                if group != (r0, r1):
                    want.append((cut, False, 1))
                    group = (r0, r1)
                want.append(("ecg_fir_windows", True, Wc))
            else:
                want.append((cut, True, Wc))
        if "cam_classes" in kw:
            want.append(("ecg_windows_overlap_mean", None, None))
        assert seen == want, (kw.keys(), seen)
        names = [n for n, _, _ in seen]
        assert names.count(cut) == (len(groups) if "filter" in kw else len(chunks))
        assert names.count("ecg_fir_windows") == (len(chunks) if "filter" in kw else 0)
        assert names.count("ecg_wfdb16_quality") == (1 if kw.get("quality") else 0)
        assert names.count("ecg_windows_overlap_mean") == (1 if "cam_classes" in kw else 0)


def test_invalid_windows_are_flagged_and_left_out(hip):
    from ecg_hip.recording import score_recording
    model = _model("cnn")
    rng = np.random.default_rng(22)
    d = rng.integers(-3000, 3000, size=(2, 3000, 12)).astype(np.int16)
    d[0, 1700, 2] = -32768                                   # windows 2 (1000..1999) and 3 (1500..2499) of recording 0
    gain, base = dev(np.full((2, 12), 1000.0)), dev(np.zeros((2, 12), np.int32))
    s = score_recording(model, dev(d), gain, base, window=1000, hop=500, batch_size=4)
    want = torch.ones(2, 5, dtype=torch.bool)
    want[0, 2] = want[0, 3] = False
    assert torch.equal(s.finite.cpu(), want)
    assert torch.isnan(s.logits[0, 2]).all()                 # the NaN lead comes out as NaN logits, as stock torch gives
    keep = s.prob[0][[0, 1, 4]]
    assert torch.equal(s.prob_max[0], keep.amax(0)) and torch.equal(s.prob_mean[0], keep.mean(0))
    assert torch.equal(s.prob_max[1], s.prob[1].amax(0)) and torch.equal(s.prob_mean[1], s.prob[1].mean(0))
    # no finite window at all: NaN, the other recording untouched
    one = score_recording(model, dev(d[:, 1000:2000]), gain, base, window=1000, batch_size=4)
    assert one.starts == (0,) and not bool(one.finite[0, 0]) and bool(one.finite[1, 0])
    assert bool(torch.isnan(one.prob_max[0]).all()) and bool(torch.isnan(one.prob_mean[0]).all())
    assert torch.equal(one.prob_max[1], one.prob[1, 0])


def test_score_recording_refuses_cpu_tensors_and_training_mode(hip):
    from ecg_hip import EcgHipError, score_recording
    model = _model("cnn")
    d = torch.zeros(3000, 12, dtype=torch.int16)
    gain, base = torch.full((12,), 1000.0, dtype=torch.float64), torch.zeros(12, dtype=torch.int32)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        score_recording(model, d, gain, base, window=1000)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.wfdb16_to_windows_sliding(d[None], gain[None], base[None], 1000, 500)
    with pytest.raises(ValueError, match="eval"):
        score_recording(model.train(), d.cuda(), gain, base, window=1000)
    with pytest.raises(ValueError, match="fewer than one window"):
        score_recording(model.eval(), d.cuda(), gain, base, window=5000)


def test_score_wfdb_record_reads_a_long_record(hip, tmp_path):
    from ecg_hip import wfdb16
    from ecg_hip.recording import score_recording, score_wfdb_record
    model = _model("cnn")
    rng = np.random.default_rng(23)
    d = rng.integers(-3000, 3000, size=(2750, 12)).astype(np.int16)
    gain, base = np.full(12, 1000.0), rng.integers(-9, 9, size=12).astype(np.int32)
    wfdb16.write_record(str(tmp_path / "strip"), d, 100, gain, base)
    a = score_wfdb_record(str(tmp_path / "strip"), model, window=1000, cam_classes=[1])
    b = score_recording(model, dev(d), dev(gain), dev(base), window=1000, cam_classes=[1])
    assert a.starts == (0, 500, 1000, 1500, 1750)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.cam, b.cam) and tuple(a.cam.shape) == (1, 1, 2750)
