"""GPU checks of the beat stage (ecg_wfdb16_beats, ecg_beats_rhythm): the beat list, the counts and the rhythm table EQUAL
the numpy restatement (tests/beats_ref.py) — integers, compared with ==; a row depends on its recording only, a table row
on the beats inside its span only; score_recording(beats=) adds the four outputs and changes nothing else, and nothing at
all with beats=None.

Every int16 stream is a slice out of the middle of a larger buffer filled with 12345, starting at an odd element offset
(2-byte aligned only): a read outside the stream changes a value and faults nothing."""
import functools

import numpy as np
import pytest
import torch

import beats_ref as br
from quality_ref import starts as window_starts
from input_util import GUARD, _model, _score, dev, guarded, hip, host, plan_on, unchanged  # noqa: F401

pytestmark = pytest.mark.gpu

INV = -32768
NUM, DEN = 3, 8


def C():
    from ecg_hip import beats as B
    return B.chunk()


def spike(d, r, p, amp=1000, zone=12):
    """One sample of `amp` on every lead at p, in the middle of zeros.  With s = 1, h = 6 its g is a plateau of 2*leads*amp
    on [p-5, p+5] (12*amp less where the recording's end cuts the second slope term): the first of the equal maxima, p-5,
    is the candidate."""
    d[r, max(0, p - zone):p + zone + 1] = 0
    d[r, p] = amp


def pulse(d, r, p, amp, sigma, rng):
    t = np.arange(d.shape[1])
    d[r] += np.round(rng.choice([-1.0, 1.0], size=d.shape[2]) * amp * np.exp(-0.5 * ((t[:, None] - p) / sigma) ** 2)).astype(np.int16)


# name -> (leads, Ttot, s, h, ref, blk) with C the chunk of the kernels
def shapes():
    c = C()
    return {"one-sample": (1, 1, 1, 0, 1, 16), "three-samples": (2, 3, 1, 2, 7, 50), "ties": (3, 700, 1, 2, 7, 50),
            "boundaries": (12, 2 * c + 37, 1, 6, 25, 200), "500hz": (16, 3 * c + 5, 5, 30, 125, 1000),
            "limits": (5, c + 300, 64, 255, 1024, 16), "one-block": (5, c + 300, 64, 255, 1024, 1 << 20),
            "masked": (12, 2 * c, 1, 6, 25, 200)}


NAMES = ["one-sample", "three-samples", "ties", "boundaries", "500hz", "limits", "one-block", "masked"]


def make_stream(name):
    """-> (d int16 [2, Ttot, leads], g_min [2], lead_mask or None)."""
    leads, Ttot, s, h, ref, blk = shapes()[name]
    c = C()
    rng = np.random.default_rng(sum(map(ord, name if name != "one-block" else "limits")))
    mask = None
    if name == "one-sample":
        d, g_min = np.array([[[5]], [[-7]]], np.int16), [1, 1]
    elif name == "three-samples":           # recording 0: no valid slope term; recording 1: one term, one beat
        d, g_min = np.array([[[INV, INV], [4, 4], [9, 9]], [[0, 3], [1, 1], [5, -2]]], np.int16), [1, 2]
    elif name == "ties":
        d = rng.integers(-2, 3, size=(2, Ttot, leads)).astype(np.int16)
        d[0, 300:340, 0] = INV              # a stretch of invalid samples on one lead
        d[:, :, 2] = INV                    # a lead that is invalid throughout
        g_min = [1, 3]
    elif name == "boundaries":
        d = rng.integers(-20, 21, size=(2, Ttot, leads)).astype(np.int16)
        # recording 0: beats at 5 (within ref of sample 0), C-1, and 2C with an equal maximum exactly ref+1 before it
        # (the plateau of the spike at 2C-31 ends at 2C-26): both are beats; a taller spike on the last sample
        for p in (10, c + 4, 2 * c - 31, 2 * c + 5):
            spike(d, 0, p)
        spike(d, 0, Ttot - 1, amp=3000)
        # recording 1: the plateau of the spike at C-30 ends at C-25, the plateau of the identical spike at C+5 starts at C:
        # equal maxima exactly ref apart across the chunk boundary, only the first is a beat; a beat at 2C-1
        for p in (c - 30, c + 5, 2 * c + 4):
            spike(d, 1, p)
        g_min = [1, 5000]
    elif name == "500hz":
        d = rng.integers(-30, 31, size=(2, Ttot, leads)).astype(np.int16)
        for p in (300, 700, c - 4, 1900, 2 * c - 1, 2200, 2500, 2900, 3 * c - 12):
            pulse(d, 0, p, 800, 6.0, rng)
        for p in (140, 520, 1111, 1800, 2 * c + 2, 2600, 3 * c):
            pulse(d, 1, p, 500, 5.0, rng)
        pulse(d, 0, 1500, 2500, 6.0, rng)   # the maximum of block 1 = [1000, 2000), which starts in chunk 0, lies in chunk 1
        d[1, 2000:2100, 3] = INV
        g_min = [1, 20000]
    elif name in ("limits", "one-block"):
        d = rng.integers(-1000, 1001, size=(2, Ttot, leads)).astype(np.int16)
        pulse(d, 0, c + 3, 9000, 40.0, rng)
        pulse(d, 1, 200, 9000, 40.0, rng)
        pulse(d, 1, c + 290, 12000, 30.0, rng)
        d[0, 600:700, 1] = INV
        g_min = [1, 1000]
    else:
        assert name == "masked"
        d = rng.integers(-300, 301, size=(2, Ttot, leads)).astype(np.int16)
        for p in range(90, Ttot, 173):
            pulse(d, int(rng.integers(2)), p, 2500, 2.0, rng)
        d[0, 100:160, 5] = INV
        g_min, mask = [1, 7000], 0b000000100110
    assert d.shape == (2, Ttot, leads)
    return d, np.asarray(g_min, np.int64), mask


@functools.lru_cache(maxsize=None)
def case_data(name):
    """One case's stream (guarded, on the device), parameters and restatement, computed once and never changed."""
    leads, Ttot, s, h, ref, blk = shapes()[name]
    d, g_min, mask = make_stream(name)
    dd, big = guarded(d)
    assert dd.data_ptr() % 4 == 2
    want, n = br.detect(d, s, h, ref, blk, NUM, DEN, g_min, mask)
    return dict(d=d, dd=dd, big=big, g_min=g_min, mask=mask, par=(s, h, ref, blk, NUM, DEN), want=want, n=n, Ttot=Ttot, ref=ref)


def run(hip, c, rows=slice(None), dd=None, mask="case"):
    dd = c["dd"][rows] if dd is None else dd
    return hip.wfdb16_beats(dd, *c["par"], dev(c["g_min"][rows]), lead_mask=c["mask"] if mask == "case" else mask)


def mismatch(got, want, what="beats"):
    """'' when equal, else where and what."""
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    return "; ".join(f"{what}{tuple(i)}: got {got[tuple(i)]} want {want[tuple(i)]}" for i in bad[:8])


def test_the_cases_cover_what_they_claim():
    c_ = C()
    assert c_ >= 256 and c_ % 2 == 0
    c = case_data("one-sample")
    assert c["n"].tolist() == [0, 0] and c["want"].shape == (2, 1)
    c = case_data("three-samples")
    assert c["n"].tolist() == [0, 1] and c["want"].shape == (2, 1)
    # ties: beats with an equal g inside their radius, a stretch of invalid samples, a lead that is invalid throughout
    c = case_data("ties")
    s, h, ref, blk = c["par"][:4]
    ties = 0
    for r in range(2):
        g = br.feature(c["d"][r], s, h)[1]
        ties += sum(1 for x in c["want"][r, :c["n"][r]] if (g[x + 1:x + ref + 1] == g[x]).any())
    assert ties > 0 and c["n"].min() >= 10
    assert (c["d"][0, 300:340, 0] == INV).all() and (c["d"][:, :, 2] == INV).all()
    # boundaries: the first maxima of g's plateaus on C-1 and 2C (recording 0) and on C and 2C-1 (recording 1)
    c = case_data("boundaries")
    s, h, ref, blk = c["par"][:4]
    Ttot = c["Ttot"]
    g0, g1 = (br.feature(c["d"][r], s, h)[1] for r in range(2))
    b0, b1 = (set(c["want"][r, :c["n"][r]].tolist()) for r in range(2))
    top = 2 * 12 * 1000
    for g, x in ((g0, c_ - 1), (g0, 2 * c_), (g1, c_), (g1, 2 * c_ - 1)):
        assert g[x] == top and g[x - 1] < top and g[x - ref:x + ref + 1].max() == top
    assert {5, c_ - 1, 2 * c_, 2 * c_ - ref - 11} <= b0 and 2 * c_ - 1 in b1
    assert min(b0) <= ref and Ttot - 1 - max(b0) <= ref                       # a beat within ref of either end
    assert g0[2 * c_ - ref - 1] == top == g0[2 * c_] and g0[2 * c_ - ref] < top  # equal maxima ref + 1 apart: both are beats
    assert g1[c_ - ref] == top == g1[c_] and c_ - ref - 10 in b1 and c_ not in b1  # exactly ref apart, over the boundary: the first
    assert not any(c_ <= x <= c_ + ref for x in b1)
    # 500hz: blk divides neither C nor Ttot; block 1 starts in chunk 0 and has its maximum in chunk 1
    c = case_data("500hz")
    s, h, ref, blk = c["par"][:4]
    assert c_ % blk and c["Ttot"] % blk and blk < c_ < 2 * blk
    g = br.feature(c["d"][0], s, h)[1]
    assert blk + int(np.argmax(g[blk:2 * blk])) >= c_
    assert c["n"].min() >= 3
    # limits: every parameter at its maximum, blk far below ref; one-block: the same stream, a single block
    c, o = case_data("limits"), case_data("one-block")
    assert c["par"][:4] == (64, 255, 1024, 16) and o["par"][3] == 1 << 20 and np.array_equal(c["d"], o["d"])
    assert c["want"].shape == (2, 2) and c["n"].max() >= 1
    c = case_data("masked")
    assert c["mask"] == 0b100110 and c["n"].min() >= 3
    assert not np.array_equal(c["want"], br.detect(c["d"], *c["par"], c["g_min"])[0])          # the mask matters


@pytest.mark.parametrize("name", NAMES)
def test_beats_equal_the_restatement(hip, name):
    c = case_data(name)
    beats, n = run(hip, c)
    cap = (c["Ttot"] + c["ref"]) // (c["ref"] + 1)
    assert beats.dtype == torch.int32 and n.dtype == torch.int32 and tuple(beats.shape) == (2, cap) and tuple(n.shape) == (2,)
    b, n = host(beats), host(n)
    assert mismatch(n, c["n"], "n_beats") == "" and mismatch(b, c["want"]) == ""
    for r in range(2):                                      # the invariants, on what the device wrote
        x = b[r, :n[r]].astype(np.int64)
        assert n[r] <= cap and (b[r, n[r]:] == -1).all()
        assert (x >= 0).all() and (x < c["Ttot"]).all() and (np.diff(x) > c["ref"]).all()
    assert unchanged(c)                                     # the kernels only read the stream
    # row r equals the call on recording r alone; another guard value gives the same list
    for r in range(2):
        one, n1 = run(hip, c, slice(r, r + 1), dd=guarded(c["d"][r:r + 1], -777)[0])
        assert torch.equal(one[0], beats[r]) and int(n1[0]) == n[r]
    both, _ = run(hip, c, dd=guarded(np.stack([c["d"][1], c["d"][1]]))[0], rows=[1, 1])
    assert torch.equal(both[0], both[1]) and torch.equal(both[0], beats[1])


def test_a_lead_mask_is_the_call_on_those_leads(hip):
    c = case_data("masked")
    beats, n = run(hip, c)
    sub = np.ascontiguousarray(c["d"][:, :, [1, 2, 5]])
    b3, n3 = hip.wfdb16_beats(guarded(sub)[0], *c["par"], dev(c["g_min"]))
    assert torch.equal(b3, beats) and torch.equal(n3, n)
    full, _ = run(hip, c, mask=None)                        # None: every lead
    assert np.array_equal(host(full), br.detect(c["d"], *c["par"], c["g_min"])[0])


# ---------------------------------------------------------------------------------------------------------------------
# the rhythm table
# ---------------------------------------------------------------------------------------------------------------------
def plans(c):
    """(T, first, hop, W, last_start, up, down) for the four window rules of the issue, tail = "shift"."""
    out = []
    for T, first, hop, up, down in ((c["ref"] + 1, 0, 1, 1, 1), (1000, 3, 501, 1, 1), (200, 0, 101, 2, 5), (300, 7, 151, 3, 2)):
        Tout = -(-c["Ttot"] * up // down)
        first, hop, W, last = plan_on(Tout, T, hop, first)[:4]
        out.append((T, first, hop, W, last, up, down))
    return out


@functools.lru_cache(maxsize=None)
def rhythm_want(name, nn_delta):
    c = case_data(name)
    return [br.rhythm(c["want"], c["n"], c["Ttot"], T, first, hop, W, last, up, down, nn_delta)
            for T, first, hop, W, last, up, down in plans(c)]


def test_the_windows_hold_zero_one_two_and_more_beats():
    seen, differ = set(), False
    for name in ("boundaries", "500hz"):
        want = rhythm_want(name, 0)
        assert want[0][..., 0].max() == 1 and want[0][..., 0].min() == 0    # ref + 1 samples hold at most one beat
        assert any(p[4] >= 0 for p in plans(case_data(name)))               # a shifted tail
        for w in want:
            seen |= set(np.unique(w[..., 0]).tolist())
        assert any((w[..., 7] > 0).any() for w in rhythm_want(name, 3))     # nn_delta = 3 still counts something
        differ |= any((a[..., 7] != b[..., 7]).any() for a, b in zip(want, rhythm_want(name, 3)))
    assert {0, 1, 2} <= seen and max(seen) >= 3 and differ                  # some |dr| lies in (0, 3]


@pytest.mark.parametrize("nn_delta", [0, 3])
@pytest.mark.parametrize("name", ["boundaries", "500hz"])
def test_rhythm_equals_the_restatement(hip, name, nn_delta):
    c = case_data(name)
    beats, n = dev(c["want"]), dev(c["n"])
    guard, gbig = guarded(c["want"], -5)                    # the list inside a guard: nothing outside it is written or needed
    for (T, first, hop, W, last, up, down), want in zip(plans(c), rhythm_want(name, nn_delta)):
        got = hip.beats_rhythm(beats, n, c["Ttot"], T, first, hop, W, last, up, down, nn_delta)
        assert got.dtype == torch.int64 and tuple(got.shape) == (2, W, 8)
        bad = np.argwhere(host(got) != want)
        assert len(bad) == 0, [(tuple(i[:2]), br.FIELDS[i[2]], host(got)[tuple(i)], want[tuple(i)]) for i in bad[:8]]
        assert torch.equal(hip.beats_rhythm(guard, n, c["Ttot"], T, first, hop, W, last, up, down, nn_delta), got)
        # row (r, w) equals a W = 1 call for that window: the first, the last (the shifted tail) and four in between
        starts = window_starts(first, hop, W, last)
        for w in sorted({0, W - 1, W // 5, W // 3, W // 2, (3 * W) // 4}):
            alone = hip.beats_rhythm(beats, n, c["Ttot"], T, starts[w], 1, 1, -1, up, down, nn_delta)
            assert torch.equal(alone[:, 0], got[:, w]), (w, starts[w])
    assert (host(gbig)[:GUARD] == -5).all() and (host(gbig)[-GUARD:] == -5).all()
    # the table of what the device itself detected is the same table
    b2, n2 = run(hip, c)
    T, first, hop, W, last, up, down = plans(c)[1]
    assert np.array_equal(host(hip.beats_rhythm(b2, n2, c["Ttot"], T, first, hop, W, last, up, down, nn_delta)),
                          rhythm_want(name, nn_delta)[1])


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(hip):
    from ecg_hip import EcgHipError, _lib as L
    d, _ = guarded(np.zeros((1, 500, 12), np.int16))
    g1 = dev(np.ones(1, np.int64))
    b, n = hip.wfdb16_beats(d, 1, 6, 25, 200, 3, 8, g1)
    assert tuple(b.shape) == (1, 20) and int(n[0]) == 0 and bool((b == -1).all())
    for args, kw, msg in (((1, 256, 25, 200, 3, 8), {}, "h=256"), ((1, 6, 0, 200, 3, 8), {}, "ref=0"),
                          ((1, 6, 25, 15, 3, 8), {}, "blk=15"), ((1, 6, 25, 200, 9, 8), {}, "num=9"),
                          ((1, 6, 25, 200, 3, 8), dict(lead_mask=0), "lead_mask"), ((65, 6, 25, 200, 3, 8), {}, "s=65")):
        with pytest.raises(EcgHipError, match=msg):
            hip.wfdb16_beats(d, *args, g1, **kw)
    # g_min NULL, and Ttot > 2^30 (asked with NULL pointers: the integer limits come first): outputs stay as they were
    beats = torch.full((1, 20), 77, dtype=torch.int32, device="cuda")
    nb = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    ws = torch.zeros(L.query("ecg_wfdb16_beats_workspace_bytes", 1, 500, 200), dtype=torch.uint8, device="cuda")
    with pytest.raises(EcgHipError, match="null pointer"):
        L.call("ecg_wfdb16_beats", L.ptr(d), None, L.ptr(beats), L.ptr(nb), L.ptr(ws), 1, 500, 12, 0xFFF, 1, 6, 25, 200, 3, 8,
               L.stream())
    with pytest.raises(EcgHipError, match="Ttot="):
        L.call("ecg_wfdb16_beats", None, None, None, None, None, 1, 2 ** 30 + 1, 12, 0xFFF, 1, 6, 25, 200, 3, 8, L.stream())
    torch.cuda.synchronize()
    assert bool((beats == 77).all()) and int(nb[0]) == 77 and not bool(ws.any())
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.wfdb16_beats(d.cpu(), 1, 6, 25, 200, 3, 8, g1)
    with pytest.raises(EcgHipError, match="int16"):
        hip.wfdb16_beats(d.float(), 1, 6, 25, 200, 3, 8, g1)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.beats_rhythm(b.cpu(), n, 500, 100, 0, 50, 9)
    with pytest.raises(EcgHipError, match="int32"):
        hip.beats_rhythm(b.long(), n, 500, 100, 0, 50, 9)
    with pytest.raises(EcgHipError, match="past"):
        hip.beats_rhythm(b, n, 500, 100, 0, 50, 10)
    with pytest.raises(EcgHipError, match="nn_delta"):
        hip.beats_rhythm(b, n, 500, 100, 0, 50, 9, nn_delta=-1)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
SLOTS = ("logits", "prob", "finite", "prob_max", "prob_mean", "cam", "cover", "quality", "lead_ok", "usable")


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.is_floating_point():
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    return torch.equal(a, b)


def _end_to_end(fs, model_fs, up, down, **kw):
    from ecg_hip.beats import BeatSpec
    model = _model()
    d = np.stack([br.synth(fs, 35, 72, 0.05, 0.01, seed=1)[0], br.synth(fs, 35, 110, 0.10, 0.02, seed=2)[0]])
    gain, base = np.full((2, 12), 1000.0), np.zeros((2, 12), np.int32)
    c = dict(d=d)
    dd, c["big"] = guarded(d)
    args = (model, dd, dev(gain), dev(base))
    kw = dict(kw, window=1000, fs=fs, model_fs=model_fs)
    s, plain = _score(*args, beats=True, **kw), _score(*args, beats=None, **kw)
    p = BeatSpec().params(fs, gain)
    want, n = br.detect(d, p["s"], p["h"], p["ref"], p["blk"], p["num"], p["den"], br.g_min_of(0.05, p["h"], gain))
    assert n.min() >= 35 and s.beats.dtype == torch.int32 and s.rhythm.dtype == torch.int64
    assert mismatch(host(s.n_beats), n, "n_beats") == "" and mismatch(host(s.beats), want) == ""
    Ttot = d.shape[1]
    W = len(s.starts)
    assert s.source_len == Ttot and W == 6 and s.starts == plain.starts
    rh = br.rhythm(want, n, Ttot, 1000, 0, 500, W, -1, up, down, p["nn_delta"])
    assert np.array_equal(host(s.rhythm), rh) and rh[..., 0].min() >= 8
    k, span = rh[..., 0].astype(np.float64), (rh[..., 2] - rh[..., 1]).astype(np.float64)
    hr = 60.0 * fs * (k - 1) / span
    got = host(s.heart_rate)
    assert got.dtype == np.float64 and got.shape == (2, W) and np.abs(got - hr).max() <= 1e-9 * np.abs(hr).max()
    assert abs(np.median(got[0]) - 72) < 4 and abs(np.median(got[1]) - 110) < 6
    for name in SLOTS:
        assert same(getattr(s, name), getattr(plain, name)), name
    assert plain.beats is None and plain.n_beats is None and plain.rhythm is None and plain.heart_rate is None
    assert unchanged(c)
    return s


def test_score_recording_with_beats(hip):
    s = _end_to_end(100, None, 1, 1, cam_classes=[1], quality=True)
    assert s.cam is not None and s.quality is not None and s.fs == 100


def test_score_recording_with_beats_on_a_resampled_recording(hip):
    """fs = 250 -> model_fs = 100: the beats stay on the source axis, the windows are mapped onto it by up/down = 2/5."""
    s = _end_to_end(250, 100, 2, 5)
    assert s.fs == 100 and s.source_len == 8750 and int(s.beats.max()) > 3500


def test_without_beats_nothing_new_is_reached(hip, monkeypatch):
    from ecg_hip.beats import BeatSpec
    model = _model()
    d = br.synth(100, 20, 80, 0.05, 0.01, seed=3)[0][None]
    args = (model, dev(d), dev(np.full((1, 12), 1000.0)), dev(np.zeros((1, 12), np.int32)))
    with pytest.raises(ValueError, match="fs"):
        _score(*args, window=1000, beats=True)
    with pytest.raises(ValueError, match="BeatSpec"):
        _score(*args, window=1000, fs=100, beats="yes")
    loose = _score(*args, window=1000, fs=100, beats=BeatSpec(leads=(0, 1), refractory_s=0.2))
    assert int(loose.n_beats[0]) >= 20
    base = _score(*args, window=1000, fs=100)

    def boom(*a, **kw):
        raise AssertionError("a beat entry point was called")

    monkeypatch.setattr(hip, "wfdb16_beats", boom)
    monkeypatch.setattr(hip, "beats_rhythm", boom)
    for kw in (dict(), dict(beats=None)):
        s = _score(*args, window=1000, fs=100, **kw)
        for name in SLOTS:
            assert same(getattr(s, name), getattr(base, name)), name
        assert s.beats is None
    with pytest.raises(AssertionError, match="beat entry point"):
        _score(*args, window=1000, fs=100, beats=True)


def test_score_wfdb_record_passes_the_rate_through(hip, tmp_path):
    from ecg_hip import wfdbraw
    from ecg_hip.recording import score_wfdb_record
    d, planted = br.synth(250, 20, 66, 0.05, 0.01, seed=4)
    gain, base = np.full(12, 1000.0), np.zeros(12, np.int32)
    wfdbraw.write_raw_record(str(tmp_path / "strip"), d.astype(np.int64), 250, gain, base, fmt=16)
    s = score_wfdb_record(str(tmp_path / "strip"), _model(), model_fs=100, window=1000, beats=True)
    from ecg_hip.beats import BeatSpec
    p = BeatSpec().params(250, gain)
    want, n = br.detect(d[None], p["s"], p["h"], p["ref"], p["blk"], p["num"], p["den"], br.g_min_of(0.05, p["h"], gain[None]))
    assert np.array_equal(host(s.beats), want) and int(s.n_beats[0]) == n[0] == len(planted)
