"""GPU checks of the signal-quality stage (ecg_wfdb16_quality): every field of every (recording, window, lead) EQUALS the
numpy restatement (tests/quality_ref.py) — integers, compared with ==; a row depends on the samples of its window only;
null rails are the (-32767, 32767) rails; score_recording(quality=) keeps the unusable windows out of prob_max /
prob_mean and changes nothing else, and nothing at all with quality=None.

Every int16 stream is a slice out of the middle of a larger buffer filled with 12345, starting at an odd element offset
(2-byte aligned only): a read outside the stream changes a value and faults nothing."""
import functools

import numpy as np
import pytest
import torch

import quality_ref as qr
from input_util import GUARD, _model, _score, dev, guarded, hip, host, plan_on, unchanged  # noqa: F401

pytestmark = pytest.mark.gpu


# (leads, T, first, hop, up, down), windows on the model's axis.  (1, 1, ...): no pair at all; (5, 37, 3, 20): window bases
# that are only 2-byte aligned, a shifted tail; (12, 1500, ...): two tiles per window; (2, 2049, ...): three tiles, the last
# of ONE sample; (12, 200, .., 2, 5): downsampling, Tq = 500, the tail's a_w clamped; (3, 300, .., 3, 2): upsampling, Tq = 200
CASES = [(1, 1, 0, 1, 1, 1), (5, 37, 3, 20, 1, 1), (12, 256, 0, 129, 1, 1), (16, 1000, 0, 501, 1, 1), (12, 1500, 3, 751, 1, 1),
         (2, 2049, 0, 1025, 1, 1), (12, 200, 0, 101, 2, 5), (3, 300, 7, 151, 3, 2)]
IDS = ["l%d-T%d-f%d-h%d-%dover%d" % c for c in CASES]


def plant(d, starts, Tq, rng):
    """The features of the issue, planted into random data d [2, Ttot, leads] in place."""
    R, Ttot, leads = d.shape
    for _ in range(12):                                     # equal-value runs of random length at random positions
        n = int(rng.integers(2, 60))
        t = int(rng.integers(0, max(1, Ttot - n)))
        d[rng.integers(R), t:t + n, rng.integers(leads)] = rng.integers(-4000, 4000)
    if leads >= 2:                                          # a stretch of -32768
        d[0, Tq // 2:Tq // 2 + Tq // 3 + 1, 1] = -32768
    for m in range(32, Ttot, 32):                           # a run across EVERY multiple of 32 samples of one lead
        d[0, m - 2:m + 3, 0] = 100 + (m // 32) % 50
    t = 0                                                   # a lead made of runs only: some run crosses any boundary
    while t < Ttot:
        n = int(rng.integers(1, 70))
        d[1, t:t + n, 0] = rng.integers(-4000, 4000)
        t += n
    c = leads - 1                                           # samples on both rails, and the 32767 / -32767 pair
    for t in rng.integers(0, Ttot, size=6):
        d[0, t, c] = 32767 if t % 2 else -32767
    p = min(Ttot - 2, starts[-1] + Tq // 2)
    d[0, p, c], d[0, p + 1, c] = 32767, -32767
    if leads >= 3:
        d[1, :, 2] = -32768                                 # a lead that is invalid throughout
    if leads >= 2 and len(starts) >= 2:                     # a run touching the first and the last sample of windows 0 and 1
        d[1, starts[0]:starts[1] + Tq, 1] = -1234


@functools.lru_cache(maxsize=None)
def case_data(case):
    """One case's stream (R = 2, about 2.5 windows on the source axis), plan and restatement, computed once."""
    leads, T, first, hop, up, down = case
    R = 2
    Tq0 = -(-T * down // up)
    Ttot = 2 * Tq0 + Tq0 // 2 + 6
    Tout = -(-Ttot * up // down)
    first, hop, W, last = plan_on(Tout, T, hop, first)[:4]
    a, Tq = qr.source_starts(Ttot, T, first, hop, W, last, up, down)
    assert Tq == Tq0 and W >= 3
    rng = np.random.default_rng(leads * 10000 + T)
    d = rng.integers(-4000, 4000, size=(R, Ttot, leads)).astype(np.int16)
    plant(d, a, Tq, rng)
    rails = (rng.integers(-3000, -1000, size=(R, leads)).astype(np.int32), rng.integers(1000, 3000, size=(R, leads)).astype(np.int32))
    dd, big = guarded(d)
    assert dd.data_ptr() % 4 == 2
    return dict(d=d, dd=dd, big=big, Ttot=Ttot, Tq=Tq, a=a, plan=(first, hop, W, last), rails=rails,
                want=qr.table(d, T, first, hop, W, last, up, down),
                want_rails=qr.table(d, T, first, hop, W, last, up, down, rails))


def mismatch(got, want):
    """'' when equal, else where and what (field by name)."""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    return "; ".join(f"(r,w,lead)={tuple(i[:3])} {qr.FIELDS[i[3]]}: got {got[tuple(i)]} want {want[tuple(i)]}" for i in bad[:8])


def test_the_cases_cover_what_they_claim():
    from ecg_hip import quality as Q
    tile = Q.tile()
    spans = {c: case_data(c)["Tq"] for c in CASES}
    assert spans[CASES[0]] == 1 and spans[CASES[6]] == 500 and spans[CASES[7]] == 200
    assert tile < spans[CASES[4]] <= 2 * tile and spans[CASES[5]] == 2 * tile + 1           # two tiles; three, the last of one sample
    assert all(spans[c] <= tile for c in CASES[:4])
    c = case_data(CASES[1])
    assert c["plan"][3] >= 0 and any((s * 5) % 8 for s in c["a"])                           # a shifted tail; bases off 16 bytes
    c = case_data(CASES[6])
    first, hop, W, last = c["plan"]
    assert qr.starts(first, hop, W, last)[-1] * 5 // 2 > c["Ttot"] - c["Tq"] == c["a"][-1]           # the clamp decides the last a_w
    c = case_data(CASES[7])
    assert c["a"][-1] == c["Ttot"] - c["Tq"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_field_equals_the_restatement(hip, case):
    leads, T, _, _, up, down = case
    c = case_data(case)
    first, hop, W, last = c["plan"]
    q = hip.wfdb16_quality(c["dd"], T, first, hop, W, last, up, down)
    assert q.dtype == torch.int64 and tuple(q.shape) == (2, W, leads, 10)
    assert mismatch(host(q), c["want"]) == ""
    # null rails are the (-32767, 32767) rails
    lo, hi = np.full((2, leads), -32767, np.int32), np.full((2, leads), 32767, np.int32)
    assert torch.equal(hip.wfdb16_quality(c["dd"], T, first, hop, W, last, up, down, rails=(lo, hi)), q)
    # rails of their own for every (recording, lead); one [leads] pair serves every recording
    qr_ = host(hip.wfdb16_quality(c["dd"], T, first, hop, W, last, up, down, rails=c["rails"]))
    assert mismatch(qr_, c["want_rails"]) == ""
    one = host(hip.wfdb16_quality(c["dd"][:1], T, first, hop, W, last, up, down, rails=(c["rails"][0][0], c["rails"][1][0])))
    assert np.array_equal(one, c["want_rails"][:1])
    assert unchanged(c)                                     # the kernel only reads


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_row_depends_on_its_window_only(hip, case):
    leads, T, _, _, up, down = case
    c = case_data(case)
    first, hop, W, last = c["plan"]
    q = hip.wfdb16_quality(c["dd"], T, first, hop, W, last, up, down, rails=c["rails"])
    # another guard value: the same table
    other, big = guarded(c["d"], -777)
    assert torch.equal(hip.wfdb16_quality(other, T, first, hop, W, last, up, down, rails=c["rails"]), q)
    assert (host(big)[:GUARD] == -777).all() and (host(big)[-GUARD:] == -777).all()
    # row (r, w) is the row of a W = 1, Ttot = Tq call on a copy of its slice: all R*W slices as recordings of one call
    Tq = c["Tq"]
    cut = np.stack([c["d"][r, a:a + Tq] for r in range(2) for a in c["a"]])
    rails = tuple(np.repeat(x, W, axis=0) for x in c["rails"])
    alone = hip.wfdb16_quality(guarded(cut)[0], Tq, 0, 1, 1, -1, rails=rails)
    assert tuple(alone.shape) == (2 * W, 1, leads, 10)
    assert torch.equal(alone.view(2, W, leads, 10), q)
    # the same recording in both slots: the same rows
    two = hip.wfdb16_quality(guarded(np.stack([c["d"][1], c["d"][1]]))[0], T, first, hop, W, last, up, down)
    assert torch.equal(two[0], two[1]) and np.array_equal(host(two[0]), c["want"][1])


def test_more_windows_than_a_grid_axis_holds(hip):
    """R*W = 70000 windows of one sample in one launch (the windowing kernels stop at 65535)."""
    rng = np.random.default_rng(3)
    d = rng.integers(-5, 5, size=(2, 35000, 3)).astype(np.int16)
    q = host(hip.wfdb16_quality(guarded(d)[0], 1, 0, 1, 35000))
    assert q.shape == (2, 35000, 3, 10)
    assert np.array_equal(q[..., 1], d) and np.array_equal(q[..., 2], d) and np.array_equal(q[..., 4], d.astype(np.int64) ** 2)
    assert (q[..., 5] == 1).all() and (q[..., 7] == 0).all() and (q[..., 0] == 0).all()


def test_bad_arguments_are_refused(hip):
    from ecg_hip import EcgHipError
    d, _ = guarded(np.zeros((1, 100, 12), np.int16))
    assert tuple(hip.wfdb16_quality(d, 50, 0, 25, 3).shape) == (1, 3, 12, 10)
    for args, kw, msg in (((50, 0, 25, 4), {}, "past"), ((50, 0, 0, 3), {}, "hop"), ((101, 0, 1, 1), {}, "longer than"),
                          ((50, 0, 25, 3, 51), {}, "last_start"), ((50, 0, 25, 3), dict(up=513), "up=513"),
                          ((50, 0, 25, 3), dict(up=2, down=5), "longer than")):
        with pytest.raises(EcgHipError, match=msg):
            hip.wfdb16_quality(d, *args, **kw)
    with pytest.raises(EcgHipError, match="leads=17"):
        hip.wfdb16_quality(guarded(np.zeros((1, 100, 17), np.int16))[0], 50, 0, 25, 3)
    with pytest.raises(EcgHipError, match="int16"):
        hip.wfdb16_quality(d.float(), 50, 0, 25, 3)
    with pytest.raises(EcgHipError, match=r"\[R, Ttot, leads\]"):
        hip.wfdb16_quality(d[0], 50, 0, 25, 3)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.wfdb16_quality(d.cpu(), 50, 0, 25, 3)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
WINDOW = 256


def _recordings(scale, seed):
    """int16 [3, 1024*scale, 12] at 1000 counts per mV (times are model-axis samples * scale).  Recording 0: lead 3 flat over
    [256, 512) — windows 1, 2, 3 at hop 128 —, lead 5 on the upper rail over [896, 1024): window 6.  Recording 1: clean.
    Recording 2: every lead silent, no usable window."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-300, 300, size=(3, 1024 * scale, 12)).astype(np.int16)
    d[0, 256 * scale:512 * scale, 3] = 17
    d[0, 896 * scale:, 5] = 32767
    d[2] = 0
    return d


def _check_gate(s, base, want_q, spec, fs, Tq):
    """s scored with quality=, base without: the table is the restatement's, usable is judge of it, the record-level
    numbers are torch's over finite & usable, and nothing else moved."""
    assert s.quality.dtype == torch.int64 and np.array_equal(host(s.quality), want_q)
    ok, usable = spec.judge(torch.from_numpy(want_q), torch.full((12,), 1000.0, dtype=torch.float64), fs, Tq)
    assert torch.equal(s.usable.cpu(), usable) and torch.equal(s.lead_ok.cpu(), ok)
    assert usable[0].tolist() == [True, False, False, False, True, True, False]
    assert bool(usable[1].all()) and not bool(usable[2].any())
    assert (~ok[0]).nonzero().tolist() == [[1, 3], [2, 3], [3, 3], [6, 5]]
    for name in ("logits", "prob", "finite"):
        assert torch.equal(getattr(s, name), getattr(base, name)), name
    assert s.starts == base.starts and bool(s.finite.all())
    keep = s.finite & s.usable
    for r in (0, 1):
        assert torch.equal(s.prob_max[r], s.prob[r][keep[r]].amax(0))
        assert torch.equal(s.prob_mean[r], s.prob[r][keep[r]].mean(0))
    assert bool(torch.isnan(s.prob_max[2]).all()) and bool(torch.isnan(s.prob_mean[2]).all())
    # where every window is usable the record-level numbers keep the bits of the ungated call
    assert torch.equal(s.prob_max[1], base.prob_max[1]) and torch.equal(s.prob_mean[1], base.prob_mean[1])
    assert base.quality is None and base.usable is None and base.lead_ok is None
    assert not bool(torch.isnan(base.prob_max).any())


def test_score_recording_gates_the_record_level_numbers(hip):
    from ecg_hip.quality import QualitySpec
    model = _model()
    d = _recordings(1, 11)
    dd, dg, db = guarded(d)[0], dev(np.full((3, 12), 1000.0)), dev(np.zeros((3, 12), np.int32))
    base = _score(model, dd, dg, db, window=WINDOW, fs=100)
    want_q = qr.table(d, WINDOW, 0, 128, 7, -1)
    for quality, batch in ((True, 256), (QualitySpec(), 4)):        # one call; one recording per call, chunked over w
        s = _score(model, dd, dg, db, window=WINDOW, fs=100, quality=quality, batch_size=batch)
        _check_gate(s, base, want_q, QualitySpec(), 100, WINDOW)
    # a spec of its own: two bad leads allowed, recording 2 still has none usable (12 silent leads)
    loose = _score(model, dd, dg, db, window=WINDOW, fs=100, quality=QualitySpec(max_bad_leads=2))
    assert bool(loose.usable[:2].all()) and not bool(loose.usable[2].any())
    assert torch.equal(loose.prob_max[:2], base.prob_max[:2])
    # flat_s is in seconds: no rate, no verdict
    with pytest.raises(ValueError, match="fs"):
        _score(model, dd, dg, db, window=WINDOW, quality=True)
    with pytest.raises(ValueError, match="QualitySpec"):
        _score(model, dd, dg, db, window=WINDOW, fs=100, quality="yes")


def test_quality_is_taken_from_the_raw_source_stream(hip):
    """Resampled (fs=250 -> model_fs=100: the windows are mapped onto the source samples they cover) and filtered (the
    table is the unfiltered stream's): the same verdicts."""
    from ecg_hip.quality import QualitySpec
    model = _model()
    dg, db = dev(np.full((3, 12), 1000.0)), dev(np.zeros((3, 12), np.int32))
    # 2560 source samples at 250 Hz -> 1024 on the model's axis; a model window covers 640 source samples
    d = np.repeat(_recordings(1, 12), 5, axis=1)[:, ::2].copy()     # the planted spans land on the same model-axis times
    assert d.shape == (3, 2560, 12)
    dd = guarded(d)[0]
    base = _score(model, dd, dg, db, window=WINDOW, fs=250, model_fs=100)
    s = _score(model, dd, dg, db, window=WINDOW, fs=250, model_fs=100, quality=True)
    assert s.fs == 100 and s.source_len == 2560 and len(s.starts) == 7
    _check_gate(s, base, qr.table(d, WINDOW, 0, 128, 7, -1, 2, 5), QualitySpec(), 250, 640)
    # filter=: the windows change, the table does not
    d = _recordings(1, 11)
    dd = guarded(d)[0]
    taps = np.array([0.25, 0.5, 0.25])
    base = _score(model, dd, dg, db, window=WINDOW, fs=100, filter=taps)
    s = _score(model, dd, dg, db, window=WINDOW, fs=100, filter=taps, quality=True)
    plain = _score(model, dd, dg, db, window=WINDOW, fs=100, quality=True)
    assert torch.equal(s.quality, plain.quality) and not torch.equal(s.logits[:2], plain.logits[:2])
    _check_gate(s, base, qr.table(d, WINDOW, 0, 128, 7, -1), QualitySpec(), 100, WINDOW)


def test_without_quality_nothing_new_is_reached(hip, monkeypatch):
    model = _model()
    d = _recordings(1, 13)
    dd, dg, db = dev(d), dev(np.full((3, 12), 1000.0)), dev(np.zeros((3, 12), np.int32))
    base = _score(model, dd, dg, db, window=WINDOW, fs=100)

    def boom(*a, **kw):
        raise AssertionError("the quality entry point was called")

    monkeypatch.setattr(hip, "wfdb16_quality", boom)
    for kw in (dict(), dict(quality=None), dict(quality=None, rails=None)):
        s = _score(model, dd, dg, db, window=WINDOW, fs=100, **kw)
        for name in ("logits", "prob", "finite", "prob_max", "prob_mean"):
            assert torch.equal(getattr(s, name), getattr(base, name)), name
        assert s.quality is None
    with pytest.raises(AssertionError, match="quality entry point"):
        _score(model, dd, dg, db, window=WINDOW, fs=100, quality=True)


def test_score_wfdb_record_takes_the_rails_from_the_header(hip, tmp_path):
    """A format-212 record with samples at +-2047: railed by the header's 12-bit ADC, not by the int16 range."""
    from ecg_hip import wfdbraw
    from ecg_hip.quality import N_RAIL
    from ecg_hip.recording import score_wfdb_record
    model = _model()
    rng = np.random.default_rng(14)
    d = rng.integers(-300, 300, size=(1024, 12))
    d[100:140:2, 4], d[101:141:2, 4], d[700:720, 9] = 2047, -2047, 2047
    gain, base = np.full(12, 200.0), np.zeros(12, np.int32)
    wfdbraw.write_raw_record(str(tmp_path / "holter"), d, 100, gain, base, fmt=212, adc_res=12)
    s = score_wfdb_record(str(tmp_path / "holter"), model, window=WINDOW, quality=True)
    dd = dev(d.astype(np.int16))[None]
    want = qr.table(d[None].astype(np.int16), WINDOW, 0, 128, 7, -1, rails=(np.full((1, 12), -2048), np.full((1, 12), 2047)))
    assert np.array_equal(host(s.quality), want)
    assert host(s.quality)[0, 0, 4, N_RAIL] == 20 and int(s.quality[0, :, 9, N_RAIL].sum()) == 40
    assert s.usable[0].tolist() == [False, False, True, True, False, False, True]        # lead 4: windows 0 and 1; lead 9: 4 and 5
    # the same stream with rails=None, and with the format's own range where the header gives no resolution
    none = _score(model, dd, dev(gain[None]), dev(base[None]), window=WINDOW, fs=100, quality=True, rails=None)
    assert torch.equal(none.logits, s.logits) and int(none.quality[..., N_RAIL].sum()) == 0
    assert torch.equal(none.quality[..., :N_RAIL], s.quality[..., :N_RAIL])
    wfdbraw.write_raw_record(str(tmp_path / "nores"), d, 100, gain, base, fmt=212, adc_res=0)
    assert torch.equal(score_wfdb_record(str(tmp_path / "nores"), model, window=WINDOW, quality=True).quality, s.quality)
    # a lead selection: the rails follow the selected signals, in the selected order
    order = [4, 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11]
    sel = score_wfdb_record(str(tmp_path / "holter"), model, leads=order, window=WINDOW, quality=True)
    assert torch.equal(sel.quality, s.quality[:, :, order])
