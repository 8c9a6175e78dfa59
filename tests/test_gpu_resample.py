"""GPU checks of the on-device polyphase resampler (ecg_wfdb16_windows_resampled): the physical output, the z-scored output
and its statistics are BIT-IDENTICAL to the numpy restatement (tests/resample_ref.py + oracle/input_oracle.py), a resampled
sample does not depend on the window that asks for it, invalid samples poison exactly what the restatement says, bad
arguments are refused, and score_recording scores a recording at another rate end to end.

Every recording is a slice out of the middle of a larger int16 tensor filled with 12345 (at an odd element offset): a read
outside the recording changes a value and faults nothing."""
import functools

import numpy as np
import pytest
import torch

import resample_ref as rr
from input_util import _model, _score, dev, guarded, hip, host, plan_on  # noqa: F401

pytestmark = pytest.mark.gpu


# ((up, down), leads, T, first).  T = 37: an odd tail, less than one tile; 256: whole tiles; 1000, 1500: more than one tile
# per window, either side of the length up to which a 12-lead window fits in LDS.  (125, 32) and (500, 257) read the
# table from global memory, the others from LDS; (1, 5) at 12 leads takes the 128-output tile, the others 256.
CASES = [((1, 5), 12, 1000, 0), ((1, 5), 5, 37, 3), ((2, 1), 12, 256, 3), ((2, 1), 1, 1500, 0), ((25, 18), 12, 1500, 0),
         ((1, 5), 12, 1500, 3), ((125, 32), 12, 1000, 0),
         ((25, 18), 1, 37, 3), ((5, 18), 5, 256, 0), ((5, 18), 12, 37, 3), ((125, 32), 12, 256, 0), ((125, 32), 5, 1000, 3),
         ((500, 257), 12, 37, 0)]
IDS = [f"{u}:{d}-l{l}-T{T}-f{f}" for (u, d), l, T, f in CASES]


@functools.lru_cache(maxsize=None)
def case_data(case):
    """One case's recording (R = 2, its own gain and baseline per recording), plan and restatement, computed once."""
    from ecg_hip.resample import design_taps, resampled_length
    (up, down), leads, T, first = case
    R = 2
    Ttot = -(-(2 * T + T // 2 + 7) * down // up)         # Tout holds about 2.5 windows
    Tout = resampled_length(Ttot, up, down)
    rng = np.random.default_rng(up * 1000 + down + leads + T)
    d = rng.integers(-4000, 4000, size=(R, Ttot, leads)).astype(np.int16)
    d[0, 0, 0], d[-1, -1, -1] = 32767, -32767
    gain = rng.choice([200.0, 1000.0, 1000.5, 3.3333e3], size=(R, leads))
    base = rng.integers(-50, 50, size=(R, leads)).astype(np.int32)
    plan = plan_on(Tout, T, T // 2 + 1, first)
    assert plan[3] == Tout - T and plan[4][0] == first      # the left edge in window 0, the right one in the shifted tail
    g, half = design_taps(up, down)
    y = [rr.resample(rr.physical(d[r], gain[r], base[r]), g, half, up, down) for r in range(R)]     # [Tout, leads] each
    return dict(d=d, gain=gain, base=base, plan=plan, Tout=Tout, y=y, dd=guarded(d)[0], dg=dev(gain), db=dev(base))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_physical_windows_equal_the_restatement(hip, case):
    (up, down), leads, T, _ = case
    c = case_data(case)
    first, hop, W, last, starts = c["plan"]
    phys = host(hip.wfdb16_windows_resampled(c["dd"], c["dg"], c["db"], T, first, hop, W, last, up, down, normalize=False))
    assert phys.shape == (2, W, leads, T)
    for r in range(2):
        assert np.array_equal(phys[r], rr.windows(c["y"][r], starts, T))
    assert bool((c["dd"].cpu() == torch.from_numpy(c["d"])).all())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zscored_windows_and_stats_equal_the_oracle_on_the_restatement(hip, case):
    (up, down), leads, T, _ = case
    c = case_data(case)
    first, hop, W, last, starts = c["plan"]
    x, stats = hip.wfdb16_windows_resampled(c["dd"], c["dg"], c["db"], T, first, hop, W, last, up, down, return_stats=True)
    assert tuple(x.shape) == (2, W, leads, T) and tuple(stats.shape) == (2 * W * leads, 2)
    x, stats = host(x), host(stats).reshape(2, W * leads, 2)
    for r in range(2):
        want, want_stats = rr.zscored(c["y"][r], starts, T)
        assert np.array_equal(x[r], want)
        assert np.array_equal(stats[r], want_stats)
    only = hip.wfdb16_windows_resampled(c["dd"], c["dg"], c["db"], T, first, hop, W, last, up, down)
    assert np.array_equal(host(only), x)
    # the plan spelled out: the resampling launch (all a call without statistics runs), then ecg_zscore_rows in place
    phys = hip.wfdb16_windows_resampled(c["dd"], c["dg"], c["db"], T, first, hop, W, last, up, down, normalize=False)
    streamed, streamed_stats = hip.zscore_per_lead(phys, out=phys, return_stats=True)
    assert np.array_equal(host(streamed), x) and np.array_equal(host(streamed_stats).reshape(2, W * leads, 2), stats)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_resampled_sample_does_not_depend_on_its_window(hip, case):
    (up, down), leads, T, _ = case
    c = case_data(case)
    first, hop, W, last, starts = c["plan"]
    Tout = c["Tout"]
    whole = host(hip.wfdb16_windows_resampled(c["dd"], c["dg"], c["db"], Tout, 0, 1, 1, -1, up, down, normalize=False))
    assert whole.shape == (2, 1, leads, Tout)
    for r in range(2):
        assert np.array_equal(whole[r, 0], c["y"][r].T)
    phys = host(hip.wfdb16_windows_resampled(c["dd"], c["dg"], c["db"], T, first, hop, W, last, up, down, normalize=False))
    for w, s in enumerate(starts):
        assert np.array_equal(phys[:, w], whole[:, 0, :, s:s + T])
    # the same recording in both slots of a batch: the same bits
    twice = np.stack([c["d"][0], c["d"][0]])
    two = host(hip.wfdb16_windows_resampled(guarded(twice)[0], c["dg"][:1].repeat(2, 1), c["db"][:1].repeat(2, 1), T, first, hop,
                                            W, last, up, down, normalize=False))
    assert np.array_equal(two[0], two[1]) and np.array_equal(two[0], phys[0])


@pytest.mark.parametrize("ratio", [(1, 5), (25, 18)])
def test_invalid_sample_poisons_what_the_restatement_says(hip, ratio):
    from ecg_hip.resample import design_taps, resampled_length
    up, down = ratio
    leads, T = 12, 64
    Ttot = -(-8 * T * down // up)
    rng = np.random.default_rng(5)
    d = rng.integers(-3000, 3000, size=(1, Ttot, leads)).astype(np.int16)
    d[0, Ttot // 2, 3] = -32768
    gain, base = np.full((1, leads), 1000.0), np.zeros((1, leads), np.int32)
    Tout = resampled_length(Ttot, up, down)
    first, hop, W, last, starts = plan_on(Tout, T, T // 2 + 1, 0)
    g, half = design_taps(up, down)
    y = rr.resample(rr.physical(d[0], gain[0], base[0]), g, half, up, down)
    want = rr.windows(y, starts, T)
    bad = np.isnan(want)
    assert bad[:, 3].any() and not np.delete(bad, 3, axis=1).any()
    phys = host(hip.wfdb16_windows_resampled(guarded(d)[0], dev(gain), dev(base), T, first, hop, W, last, up, down,
                                             normalize=False))[0]
    assert np.array_equal(np.isnan(phys), bad) and np.array_equal(phys, want, equal_nan=True)
    # score_recording: exactly the windows that hold one are flagged
    model = _model()
    s = _score(model, guarded(d)[0], dev(gain), dev(base), window=T, hop=hop, fs=down * 100, model_fs=up * 100)
    assert s.starts == starts
    assert np.array_equal(host(s.finite)[0], ~bad.any(axis=(1, 2)))
    assert not host(s.finite).all() and host(s.finite).any()


def test_bad_arguments_are_refused(hip):
    from ecg_hip import EcgHipError
    from ecg_hip.resample import device_taps
    d = guarded(np.zeros((1, 600, 12), np.int16))[0]
    gain, base = dev(np.full((1, 12), 1000.0)), dev(np.zeros((1, 12), np.int32))
    taps, ntap, half = device_taps(1, 5, d.device)           # Tout = 120
    assert (ntap, half) == (101, 50)
    ok = dict(window=50, first=0, hop=25, W=3, last_start=-1, up=1, down=5, ntap=ntap, half=half)

    def call(dd=d, g=gain, b=base, **kw):
        return hip._resampled_call(dd, g, b, taps, **{**ok, **kw})

    assert tuple(call().shape) == (1, 3, 12, 50)
    for kw, msg in ((dict(up=0), "up=0"), (dict(down=513), "down=513"), (dict(ntap=100), "filter length"),
                    (dict(ntap=257), "ntap=257"), (dict(half=-1), "half"), (dict(first=71), "past"),
                    (dict(last_start=71), "last_start"), (dict(window=121, W=1), "longer than")):
        with pytest.raises(EcgHipError, match=msg):
            call(**kw)
    d17 = guarded(np.zeros((1, 600, 17), np.int16))[0]
    with pytest.raises(EcgHipError, match="leads=17"):
        call(dd=d17, g=dev(np.full((1, 17), 1000.0)), b=dev(np.zeros((1, 17), np.int32)))
    for kw in (dict(up=0, down=5), dict(up=1, down=513)):
        with pytest.raises(EcgHipError, match="outside"):
            hip.wfdb16_windows_resampled(d, gain, base, 50, 0, 25, 3, -1, **kw)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.wfdb16_windows_resampled(d.cpu(), gain.cpu(), base.cpu(), 50, 0, 25, 3, -1, 1, 5)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_score_recording_at_another_rate(hip):
    import ecg_hip
    from ecg_hip.resample import design_taps, resampled_length
    model = _model()
    Ttot, window = 6003, 200
    rng = np.random.default_rng(31)
    d = rng.integers(-3000, 3000, size=(1, Ttot, 12)).astype(np.int16)
    gain, base = np.full((1, 12), 1000.0), rng.integers(-9, 9, size=(1, 12)).astype(np.int32)
    dd, dg, db = guarded(d)[0], dev(gain), dev(base)
    Tout = resampled_length(Ttot, 1, 5)
    assert Tout == 1201
    g, half = design_taps(1, 5)
    y = rr.resample(rr.physical(d[0], gain[0], base[0]), g, half, 1, 5)
    plan = plan_on(Tout, window, window // 2, 0)
    x = dev(rr.zscored(y, plan[4], window)[0])                  # the restatement's windows, uploaded
    with torch.no_grad():
        want = model(x)
    s = _score(model, dd, dg, db, window=window, fs=500, model_fs=100)
    assert s.starts == plan[4] and s.fs == 100 and s.source_len == Ttot and s.cam is None
    assert torch.equal(s.logits[0], want)
    sc = _score(model, dd[0], dg[0], db[0], window=window, fs=500, model_fs=100, cam_classes=[1])
    assert sc.fs == 100 and sc.source_len == Ttot and sc.starts == plan[4]
    assert tuple(sc.cam.shape) == (1, 1, Tout) and tuple(sc.cover.shape) == (Tout,)
    cam, lg = ecg_hip.grad_cam(model, x, None, class_idx=[1], signal_length=window, normalize=None, return_logits=True)
    assert torch.equal(sc.cam, hip.overlap_mean(cam.reshape(1, plan[2], 1, window), plan, Tout))
    print("cam-call logits - model(x):", float((sc.logits[0] - want).abs().max()))
    assert torch.equal(sc.logits[0], lg)
    assert torch.equal(sc.logits[0], want)


def test_equal_or_missing_rates_never_reach_the_resampler(hip, monkeypatch):
    """fs == model_fs, or either None: the existing path, bit for bit — the new binding is not called."""
    model = _model()
    rng = np.random.default_rng(32)
    d = rng.integers(-3000, 3000, size=(1, 700, 12)).astype(np.int16)
    dd, dg, db = guarded(d)[0], dev(np.full((1, 12), 1000.0)), dev(np.zeros((1, 12), np.int32))
    base = _score(model, dd, dg, db, window=200)
    assert base.fs is None and base.source_len == 700

    def boom(*a, **kw):
        raise AssertionError("the resampled entry point was called")

    monkeypatch.setattr(hip, "wfdb16_windows_resampled", boom)
    for kw, fs in ((dict(fs=500, model_fs=500), 500), (dict(fs=250), 250), (dict(model_fs=100), None),
                   (dict(fs=500.0, model_fs=500), 500)):
        s = _score(model, dd, dg, db, window=200, **kw)
        assert s.starts == base.starts and torch.equal(s.logits, base.logits) and s.fs == fs and s.source_len == 700
    with pytest.raises(AssertionError, match="resampled entry point"):
        _score(model, dd, dg, db, window=200, fs=500, model_fs=250)


def test_score_wfdb_record_uses_the_header_rate(hip, tmp_path):
    from ecg_hip import wfdb16
    from ecg_hip.recording import score_wfdb_record
    model = _model()
    rng = np.random.default_rng(33)
    d = rng.integers(-3000, 3000, size=(701, 12)).astype(np.int16)
    gain, base = np.full(12, 1000.0), rng.integers(-9, 9, size=12).astype(np.int32)
    wfdb16.write_record(str(tmp_path / "strip"), d, 250, gain, base)
    a = score_wfdb_record(str(tmp_path / "strip"), model, model_fs=500, window=400, cam_classes=[1])
    b = _score(model, dev(d), dev(gain), dev(base), window=400, cam_classes=[1], fs=250, model_fs=500)
    assert a.fs == 500 and a.source_len == 701 and a.starts == b.starts == (0, 200, 400, 600, 800, 1000, 1002)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.cam, b.cam) and tuple(a.cam.shape) == (1, 1, 1402)
    # model_fs=None: today's result, at the record's own rate
    c = score_wfdb_record(str(tmp_path / "strip"), model, window=400, cam_classes=[1])
    e = _score(model, dev(d), dev(gain), dev(base), window=400, cam_classes=[1])
    assert c.fs == 250 and c.starts == e.starts == (0, 200, 301)
    assert torch.equal(c.logits, e.logits) and torch.equal(c.cam, e.cam)
