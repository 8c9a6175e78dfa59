"""GPU checks of the on-device zero-phase FIR (ecg_fir_windows): the filtered physical windows, the z-scored windows and
their statistics are BIT-IDENTICAL to the numpy restatement (tests/fir_ref.py + oracle/input_oracle.py), a filtered sample
does not depend on the window that asks for it, invalid samples poison exactly what the restatement says, bad arguments
are refused before any launch, and score_recording conditions a drifting recording end to end.

Every fp32 recording is a slice out of the middle of a larger tensor filled with 12345.0 (at an odd element offset, so
rows are 4-byte aligned only): a read outside the recording changes a value and faults nothing."""
import functools

import numpy as np
import pytest
import torch

import fir_ref as fr
from input_util import _model, _score, dev, guarded, hip, host, plan_on, unchanged  # noqa: F401

pytestmark = pytest.mark.gpu


# (half, leads, T, first).  half = 0: taps [1.0], the output is the unfiltered physical windows; 363 and 2720: the real
# 100 Hz high-pass and the 500 Hz high-pass + 50 Hz notch; (363, 5, 37, 3): half > Ttot, both clamps in one sum;
# T = 1500 with half = 2720: two tiles per window, a filter longer than any tile; 4096: the ABI limit; 1 and 7: the tap
# loop's remainder without and with nothing before it.
CASES = [(0, 12, 37, 0), (1, 1, 37, 3), (7, 5, 256, 0), (363, 12, 1000, 0), (363, 5, 37, 3), (2720, 12, 1500, 3),
         (4096, 1, 256, 0)]
IDS = [f"h{h}-l{l}-T{T}-f{f}" for h, l, T, f in CASES]


def case_taps(half):
    """-> (what the test hands to fir_windows, the one-sided fp32 taps).  Designs go in as one_sided's result, the others
    as the full symmetric array."""
    from ecg_hip.filter import FilterSpec, one_sided
    if half == 363:
        c = one_sided(FilterSpec().taps(100))
    elif half == 2720:
        c = one_sided(FilterSpec(notch=50).taps(500))
    elif half == 0:
        return np.ones(1, np.float32), np.ones(1, np.float32)
    else:
        c = np.random.default_rng(half).uniform(-1, 1, size=half + 1).astype(np.float32)
        return np.concatenate([c[:0:-1], c]), c
    assert len(c) == half + 1
    return c, np.asarray(c)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """One case's recordings (R = 2, own gain and baseline each), plan and restatement, computed once."""
    half, leads, T, first = case
    R = 2
    Ttot = 2 * T + T // 2 + 7
    rng = np.random.default_rng(half * 1000 + leads + T)
    d = rng.integers(-4000, 4000, size=(R, Ttot, leads)).astype(np.int16)
    d[0, 0, 0], d[-1, -1, -1] = 32767, -32767
    gain = rng.choice([200.0, 1000.0, 1000.5, 3.3333e3], size=(R, leads))
    base = rng.integers(-50, 50, size=(R, leads)).astype(np.int32)
    p = [fr.physical(d[r], gain[r], base[r]) for r in range(R)]            # [Ttot, leads] each
    plan = plan_on(Ttot, T, T // 2 + 1, first)
    assert plan[3] == Ttot - T and plan[4][0] == first      # the left edge in window 0, the right one in the shifted tail
    taps, c = case_taps(half)
    y = [fr.fir(p[r], c) for r in range(R)]
    x = np.stack([np.ascontiguousarray(p[r].T) for r in range(R)])          # [R, leads, Ttot]
    dx, big = guarded(x)
    assert dx.data_ptr() % 8 == 4
    return dict(x=x, p=p, y=y, plan=plan, Ttot=Ttot, taps=taps, c=c, dx=dx, big=big)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filtered_windows_equal_the_restatement(hip, case):
    half, leads, T, _ = case
    c = case_data(case)
    first, hop, W, last, starts = c["plan"]
    phys = host(hip.fir_windows(c["dx"], c["taps"], T, first, hop, W, last, normalize=False))
    assert phys.shape == (2, W, leads, T)
    for r in range(2):
        assert np.array_equal(phys[r], fr.windows(c["y"][r], starts, T))
        if half == 0:
            assert np.array_equal(phys[r], fr.windows(c["p"][r], starts, T))
    assert unchanged(c)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zscored_windows_and_stats_equal_the_oracle_on_the_restatement(hip, case):
    half, leads, T, _ = case
    c = case_data(case)
    first, hop, W, last, starts = c["plan"]
    x, stats = hip.fir_windows(c["dx"], c["taps"], T, first, hop, W, last, return_stats=True)
    assert tuple(x.shape) == (2, W, leads, T) and tuple(stats.shape) == (2 * W * leads, 2)
    x, stats = host(x), host(stats).reshape(2, W * leads, 2)
    for r in range(2):
        want, want_stats = fr.zscored(c["y"][r], starts, T)
        assert np.array_equal(x[r], want)
        assert np.array_equal(stats[r], want_stats)
    assert np.array_equal(host(hip.fir_windows(c["dx"], c["taps"], T, first, hop, W, last)), x)
    # the plan spelled out: the filter launch (all a call without statistics runs), then ecg_zscore_rows in place
    phys = hip.fir_windows(c["dx"], c["taps"], T, first, hop, W, last, normalize=False)
    streamed, streamed_stats = hip.zscore_per_lead(phys, out=phys, return_stats=True)
    assert np.array_equal(host(streamed), x) and np.array_equal(host(streamed_stats).reshape(2, W * leads, 2), stats)
    assert unchanged(c)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_filtered_sample_does_not_depend_on_its_window(hip, case):
    half, leads, T, _ = case
    c = case_data(case)
    first, hop, W, last, starts = c["plan"]
    whole = host(hip.fir_filter(c["dx"], c["taps"]))
    assert whole.shape == (2, leads, c["Ttot"])
    for r in range(2):
        assert np.array_equal(whole[r], c["y"][r].T)
    phys = host(hip.fir_windows(c["dx"], c["taps"], T, first, hop, W, last, normalize=False))
    for w, s in enumerate(starts):
        assert np.array_equal(phys[:, w], whole[:, :, s:s + T])
    # the same recording in both slots of a batch: the same bits
    two = host(hip.fir_windows(guarded(np.stack([c["x"][0], c["x"][0]]))[0], c["taps"], T, first, hop, W, last,
                               normalize=False))
    assert np.array_equal(two[0], two[1]) and np.array_equal(two[0], phys[0])
    assert unchanged(c)


def test_invalid_samples_poison_what_the_restatement_says(hip):
    leads, T, half = 12, 64, 20
    Ttot = 8 * T
    rng = np.random.default_rng(5)
    d = rng.integers(-3000, 3000, size=(1, Ttot, leads)).astype(np.int16)
    d[0, Ttot // 2, 3] = -32768         # poisons Ttot/2 - half .. Ttot/2 + half of lead 3
    d[0, 0, 7] = -32768                 # at the edge the clamp repeats it: 0 .. half of lead 7
    gain, base = np.full((1, leads), 1000.0), np.zeros((1, leads), np.int32)
    c = rng.uniform(-1, 1, size=half + 1).astype(np.float32)
    taps = np.concatenate([c[:0:-1], c])
    first, hop, W, last, starts = plan_on(Ttot, T, T // 2 + 1, 0)
    p = fr.physical(d[0], gain[0], base[0])
    y = fr.fir(p, c)
    nan_t = np.isnan(y)
    assert np.array_equal(np.nonzero(nan_t[:, 3])[0], np.arange(Ttot // 2 - half, Ttot // 2 + half + 1))
    assert np.array_equal(np.nonzero(nan_t[:, 7])[0], np.arange(0, half + 1))
    assert not np.delete(nan_t, [3, 7], axis=1).any()
    want = fr.windows(y, starts, T)
    bad = np.isnan(want)
    dx, _ = guarded(np.ascontiguousarray(p.T)[None])
    phys = host(hip.fir_windows(dx, taps, T, first, hop, W, last, normalize=False))[0]
    assert np.array_equal(np.isnan(phys), bad) and np.array_equal(phys, want, equal_nan=True)
    # score_recording: exactly the windows the restatement poisons are flagged
    s = _score(_model(), dev(d), dev(gain), dev(base), window=T, hop=hop, filter=taps)
    assert s.starts == starts
    assert np.array_equal(host(s.finite)[0], ~bad.any(axis=(1, 2)))
    assert not host(s.finite).all() and host(s.finite).any()
    # ... which are more than the unfiltered recording loses
    plain = _score(_model(), dev(d), dev(gain), dev(base), window=T, hop=hop)
    assert host(plain.finite).sum() > host(s.finite).sum()


def test_bad_arguments_are_refused(hip):
    from ecg_hip import EcgHipError
    from ecg_hip.filter import device_one_sided
    x, _ = guarded(np.zeros((1, 12, 120), np.float32))
    c, half = device_one_sided(np.array([0.25, 0.5, 0.25]), x.device)
    assert half == 1
    ok = dict(window=50, first=0, hop=25, W=3, last_start=-1, half=1)

    def call(xx=x, **kw):
        return hip._fir_call(xx, c, **{**ok, **kw})

    assert tuple(call().shape) == (1, 3, 12, 50)
    for kw, msg in ((dict(half=-1), "half=-1"), (dict(half=4097), "half=4097"), (dict(first=71), "past"),
                    (dict(last_start=71), "last_start"), (dict(window=121, W=1), "longer than"), (dict(hop=0), "hop")):
        with pytest.raises(EcgHipError, match=msg):
            call(**kw)
    with pytest.raises(EcgHipError, match="leads=17"):
        call(xx=guarded(np.zeros((1, 17, 120), np.float32))[0])
    many = torch.zeros(60, 12, 120, device="cuda")
    with pytest.raises(EcgHipError, match="65535"):        # rows for the statistics: 6000 windows x 12 leads
        hip._fir_call(many, c, 1, 0, 1, 100, -1, 1)
    assert tuple(hip._fir_call(many, c, 1, 0, 1, 100, -1, 1, normalize=False).shape) == (60, 100, 12, 1)
    taps = np.array([0.25, 0.5, 0.25])
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.fir_windows(x.cpu(), taps, 50, 0, 25, 3)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.fir_filter(x.cpu(), taps)
    with pytest.raises(EcgHipError, match="float32"):
        hip.fir_windows(x.double(), taps, 50, 0, 25, 3)
    with pytest.raises(EcgHipError, match="float32"):
        hip.fir_windows(x.to(torch.int16), taps, 50, 0, 25, 3)
    with pytest.raises(EcgHipError, match=r"\[R, leads, Ttot\]"):
        hip.fir_filter(x[0], taps)
    with pytest.raises(ValueError, match="symmetric"):
        hip.fir_windows(x, np.array([0.25, 0.5, 0.26]), 50, 0, 25, 3)
    with pytest.raises(ValueError, match="4096"):
        hip.fir_windows(x, np.ones(2 * 4097 + 1), 50, 0, 25, 3)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _drifting(R, Ttot, fs, seed):
    """int16 [R, Ttot, 12] at 1000 counts per mV: noise + a 2 mV, 0.15 Hz drift of its own phase on every lead."""
    rng = np.random.default_rng(seed)
    t = np.arange(Ttot)[None, :, None] / fs
    drift = 2000.0 * np.sin(2 * np.pi * 0.15 * t + rng.uniform(0, 6.28, size=(R, 1, 12)))
    return (rng.integers(-300, 300, size=(R, Ttot, 12)) + drift).astype(np.int16)


@pytest.mark.parametrize("R,batch", [(1, 8), (3, 64)])
def test_score_recording_with_a_filter_equals_the_manual_loop(hip, R, batch):
    """fs=500 -> model_fs=100 with FilterSpec(): the spec is designed at 100 Hz, the resampled recording is written once
    per recording group and every chunk comes from fir_windows.  (1, 8): one recording chunked over its windows;
    (3, 64): groups of two recordings."""
    from ecg_hip.filter import FilterSpec
    from ecg_hip.recording import plan_chunks, window_plan
    from ecg_hip.resample import resampled_length
    model = _model()
    Ttot, window = 15003, 200
    d = _drifting(R, Ttot, 500, 41)
    dd, dg, db = dev(d), dev(np.full((R, 12), 1000.0)), dev(np.zeros((R, 12), np.int32))
    Tout = resampled_length(Ttot, 1, 5)
    plan = window_plan(Tout, window, window // 2)
    first, hop, W, last, starts = plan
    chunks = plan_chunks(R, plan, batch)
    assert len(chunks) > 1 and Tout == 3001
    taps = FilterSpec().taps(100)
    want = torch.empty(R, W, 5, device="cuda")
    for r0, r1, w0, f, Wc, l in chunks:
        whole = hip.wfdb16_windows_resampled(dd[r0:r1], dg[r0:r1], db[r0:r1], Tout, 0, 1, 1, -1, 1, 5, normalize=False)[:, 0]
        x = hip.fir_windows(whole, taps, window, f, hop, Wc, l)
        with torch.no_grad():
            want[r0:r1, w0:w0 + Wc] = model(x.view(-1, 12, window)).view(r1 - r0, Wc, 5)
    s = _score(model, dd, dg, db, window=window, batch_size=batch, fs=500, model_fs=100, filter=FilterSpec())
    assert s.starts == starts and s.fs == 100 and s.source_len == Ttot and bool(s.finite.all())
    assert torch.equal(s.logits, want)
    assert torch.equal(_score(model, dd, dg, db, window=window, batch_size=batch, fs=500, model_fs=100, filter=taps).logits, want)
    plain = _score(model, dd, dg, db, window=window, batch_size=batch, fs=500, model_fs=100)
    assert plain.starts == s.starts and not torch.equal(plain.logits, s.logits)
    # the filter is what the windows were cut from: 2 mV of drift is gone from the conditioned signal
    whole = hip.wfdb16_windows_resampled(dd[:1], dg[:1], db[:1], Tout, 0, 1, 1, -1, 1, 5, normalize=False)[:, 0]
    y = hip.fir_filter(whole, taps)
    assert float(whole[..., 400:-400].abs().max()) > 1.9 and float(y[..., 400:-400].abs().max()) < 0.5


def test_without_a_filter_nothing_new_is_reached_and_a_spec_needs_a_rate(hip, monkeypatch):
    """filter=None: the existing path, bit for bit — neither new binding is called."""
    from ecg_hip.filter import FilterSpec
    model = _model()
    d = _drifting(1, 700, 100, 42)
    dd, dg, db = dev(d), dev(np.full((1, 12), 1000.0)), dev(np.zeros((1, 12), np.int32))
    base = _score(model, dd, dg, db, window=200)
    filtered = _score(model, dd, dg, db, window=200, fs=100, filter=FilterSpec())
    assert filtered.fs == 100 and filtered.starts == base.starts and not torch.equal(filtered.logits, base.logits)
    with pytest.raises(ValueError, match="sampling rate"):
        _score(model, dd, dg, db, window=200, filter=FilterSpec())                      # no rate at all
    with pytest.raises(ValueError, match="sampling rate"):
        _score(model, dd, dg, db, window=200, model_fs=100, filter=FilterSpec())        # not resampled: fs is the axis

    def boom(*a, **kw):
        raise AssertionError("the filter entry point was called")

    monkeypatch.setattr(hip, "fir_windows", boom)
    monkeypatch.setattr(hip, "_fir_call", boom)
    for kw in (dict(), dict(filter=None), dict(fs=100, filter=None), dict(fs=100, model_fs=100)):
        s = _score(model, dd, dg, db, window=200, **kw)
        assert s.starts == base.starts and torch.equal(s.logits, base.logits)
    with pytest.raises(AssertionError, match="filter entry point"):
        _score(model, dd, dg, db, window=200, fs=100, filter=FilterSpec())


def test_score_wfdb_record_passes_the_filter_through(hip, tmp_path):
    from ecg_hip import wfdb16
    from ecg_hip.filter import FilterSpec
    from ecg_hip.recording import score_wfdb_record
    model = _model()
    d = _drifting(1, 2501, 250, 43)[0]
    gain, base = np.full(12, 1000.0), np.zeros(12, np.int32)
    wfdb16.write_record(str(tmp_path / "strip"), d, 250, gain, base)
    spec = FilterSpec(highpass=1.0, notch=50, width=2.0)
    a = score_wfdb_record(str(tmp_path / "strip"), model, window=400, filter=spec, cam_classes=[1])
    b = _score(model, dev(d), dev(gain), dev(base), window=400, fs=250, filter=spec.taps(250), cam_classes=[1])
    assert a.fs == 250 and a.source_len == 2501 and a.starts == b.starts
    assert torch.equal(a.logits, b.logits) and torch.equal(a.cam, b.cam) and tuple(a.cam.shape) == (1, 1, 2501)
    plain = score_wfdb_record(str(tmp_path / "strip"), model, window=400)
    assert not torch.equal(plain.logits, a.logits)
    # resampled to the model's rate: the spec is designed there (where a 50 Hz notch no longer fits)
    c = score_wfdb_record(str(tmp_path / "strip"), model, model_fs=500, window=400, filter=spec)
    e = _score(model, dev(d), dev(gain), dev(base), window=400, fs=250, model_fs=500, filter=spec.taps(500))
    assert c.fs == 500 and torch.equal(c.logits, e.logits)
    with pytest.raises(ValueError, match="resampler"):
        score_wfdb_record(str(tmp_path / "strip"), model, model_fs=100, window=400, filter=spec)
