"""CPU-side checks of the beat stage: the vectorised numpy restatement (tests/beats_ref.py) against a literal per-sample
double loop, BeatSpec.params' rounding, beats.summarize on a hand-written table, the detector's quality on synthetic
recordings (asserted on the restatement), and the host-side refusals of the two entry points (null pointers: nothing is
launched, no GPU is needed)."""
import math

import numpy as np
import pytest
import torch

import beats_ref as br

from ecg_hip import beats as B
from ecg_hip.beats import BeatSpec

INV = -32768


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, restated: every definition as a loop over samples
# ---------------------------------------------------------------------------------------------------------------------
def literal_beats(v, s, h, ref, blk, num, den, g_min, lead_mask=None):
    Ttot, leads = len(v), len(v[0])
    f = [0] * Ttot
    for n in range(s, Ttot - s):
        for l in range(leads):
            if lead_mask is not None and not (lead_mask >> l) & 1:
                continue
            a, b = int(v[n + s][l]), int(v[n - s][l])
            if a != INV and b != INV:
                f[n] += abs(a - b)
    g = [sum(f[j] for j in range(max(0, n - h), min(Ttot - 1, n + h) + 1)) for n in range(Ttot)]
    nblk = -(-Ttot // blk)
    M = [max(g[b * blk:(b + 1) * blk]) for b in range(nblk)]
    thr = []
    for b in range(nblk):
        near = sorted(M[bb] for bb in range(b - 2, b + 3) if 0 <= bb < nblk)
        thr.append(max(g_min, (num * near[(len(near) - 1) // 2]) // den))
    found = []
    for n in range(Ttot):
        if (g[n] >= thr[n // blk] and all(g[n] > g[j] for j in range(max(0, n - ref), n))
                and all(g[n] >= g[j] for j in range(n + 1, min(Ttot - 1, n + ref) + 1))):
            found.append(n)
    return f, g, M, thr, found


@pytest.mark.parametrize("leads,Ttot,s,h,ref,blk,lo,hi", [(1, 1, 1, 0, 1, 16, -5, 5), (2, 3, 1, 2, 7, 50, -5, 5),
                                                        (3, 230, 1, 2, 7, 50, -2, 3), (4, 190, 3, 5, 11, 16, -300, 300),
                                                        (2, 97, 2, 0, 1, 20, -2, 3), (3, 150, 4, 9, 40, 64, -50, 50)])
def test_the_restatement_equals_the_literal_loops(leads, Ttot, s, h, ref, blk, lo, hi):
    rng = np.random.default_rng(Ttot * 31 + leads)
    v = rng.integers(lo, hi, size=(Ttot, leads)).astype(np.int16)
    if Ttot > 60:
        v[20:45, 0] = INV
        v[rng.integers(0, Ttot, size=5), leads - 1] = INV
    for mask, g_min, (num, den) in ((None, 1, (3, 8)), ((1 << leads) - 1, 4, (1, 1)), (1 << (leads - 1), 1, (5, 7))):
        f, g, M, thr, found = literal_beats(v.tolist(), s, h, ref, blk, num, den, g_min, mask)
        rf, rg = br.feature(v, s, h, mask)
        rM, rthr = br.thresholds(rg, blk, num, den, g_min)
        assert rf.tolist() == f and rg.tolist() == g and rM.tolist() == M and rthr.tolist() == thr
        got = br.beats(v, s, h, ref, blk, num, den, g_min, mask)
        assert got.tolist() == found
        assert all(b - a > ref for a, b in zip(found, found[1:])) and len(found) <= br.capacity(Ttot, ref)
    table, n = br.detect(np.stack([v, v[::-1]]), s, h, ref, blk, 3, 8, [1, 2])
    assert table.shape == (2, br.capacity(Ttot, ref)) and table.dtype == np.int32
    assert table[0, :n[0]].tolist() == literal_beats(v.tolist(), s, h, ref, blk, 3, 8, 1)[4] and (table[0, n[0]:] == -1).all()
    assert table[1, :n[1]].tolist() == literal_beats(v[::-1].tolist(), s, h, ref, blk, 3, 8, 2)[4]


def test_ties_go_to_the_first_and_written_out_answers():
    # one lead, s = 1, h = 0: g[n] = |v[n+1] - v[n-1]|, so a lone spike at 10 gives equal peaks at 9 and 11
    v = np.zeros((40, 1), np.int16)
    v[10, 0] = 9
    _, g = br.feature(v, 1, 0)
    assert g.tolist()[8:13] == [0, 9, 0, 9, 0]
    assert br.beats(v, 1, 0, 1, 16, 1, 1, 1).tolist() == [9, 11]            # more than ref = 1 apart: both
    assert br.beats(v, 1, 0, 2, 16, 1, 1, 1).tolist() == [9]                # exactly ref apart: the first of equal maxima
    v[20, 0] = 9                                                            # equal peaks at 9, 11, 19, 21
    assert br.beats(v, 1, 0, 7, 16, 1, 1, 1).tolist() == [9, 19]
    assert br.beats(v, 1, 0, 8, 16, 1, 1, 1).tolist() == [9]                # 19 is exactly ref after the equal peak at 11
    assert br.beats(v, 1, 0, 7, 16, 1, 1, 10).tolist() == []                # under g_min
    # a flat stream has g = 0 < g_min everywhere; an invalid sample removes its lead's terms only
    assert br.beats(np.full((50, 2), 7, np.int16), 1, 2, 3, 16, 1, 1, 1).tolist() == []
    v = np.zeros((9, 2), np.int16)
    v[4] = (5, INV)
    assert br.feature(v, 1, 0)[0].tolist() == [0, 0, 0, 5, 0, 5, 0, 0, 0]


def test_rhythm_rows_with_written_out_answers():
    big = 2 ** 31 - 1
    assert br.FIELDS == B.FIELDS and len(B.FIELDS) == 8
    assert [B.FIELDS[i] for i in (B.N_BEATS, B.FIRST_BEAT, B.LAST_BEAT, B.SUM_RR_SQ, B.MIN_RR, B.MAX_RR, B.SUM_DRR_SQ,
                                  B.N_DRR_OVER)] == list(B.FIELDS)
    assert br.rhythm_row([], 0) == [0, -1, -1, 0, big, 0, 0, 0]
    assert br.rhythm_row([17], 0) == [1, 17, 17, 0, big, 0, 0, 0]
    assert br.rhythm_row([10, 110], 0) == [2, 10, 110, 10000, 100, 100, 0, 0]
    assert br.rhythm_row([10, 110, 200, 305], 10) == [4, 10, 305, 100 ** 2 + 90 ** 2 + 105 ** 2, 90, 105, 100 + 225, 1]
    assert br.rhythm_row([10, 110, 200, 305], 9) == [4, 10, 305, 29125, 90, 105, 325, 2]
    # windows on the model's axis, mapped by up/down: T = 200 at 2/5 covers 500 source samples
    table = np.array([[100, 400, 600, 1254, -1], [0, -1, -1, -1, -1]], np.int32)
    out = br.rhythm(table, [4, 1], 1255, 200, 0, 101, 4, 302, 2, 5)
    assert out.shape == (2, 4, 8) and out.dtype == np.int64         # source spans [0,500) [252,752) [505,1005) [755,1255)
    assert out[0, :, 0].tolist() == [2, 2, 1, 1] and out[0, 3, 1:3].tolist() == [1254, 1254] and out[1, :, 0].tolist() == [1, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# BeatSpec
# ---------------------------------------------------------------------------------------------------------------------
def test_params_rounding():
    want = {100: (1, 6, 25, 200, 5), 250: (3, 15, 63, 500, 13), 360: (4, 22, 90, 720, 18), 500: (5, 30, 125, 1000, 25)}
    for fs, (s, h, ref, blk, nn) in want.items():
        p = BeatSpec().params(fs, np.full(12, 1000.0))
        assert (p["s"], p["h"], p["ref"], p["blk"], p["nn_delta"]) == (s, h, ref, blk, nn), fs
        assert (p["num"], p["den"], p["lead_mask"]) == (3, 8, 0xFFF)
        assert p["g_min"].dtype == torch.int64 and p["g_min"].tolist() == [math.floor(0.05 * (2 * h + 1) * 12000.0)]
    assert math.floor(2.5 + 0.5) == 3 and BeatSpec().params(250, [1.0])["s"] == 3            # halves round up, not to even
    assert BeatSpec(slope_s=0.001).params(100, [1.0])["s"] == 1                              # s is at least 1
    assert BeatSpec(integ_half_s=0.0).params(100, [1.0])["h"] == 0
    # g_min per recording over the leads taking part, never under 1
    gain = np.array([[200.0, 1000.0, 50.0], [0.0, 0.0, 0.0]])
    p = BeatSpec(leads=(0, 2), floor_mv=0.05).params(100, gain)
    assert p["lead_mask"] == 0b101 and p["g_min"].tolist() == [math.floor(0.05 * 13 * 250.0), 1]
    assert p["g_min"].tolist() == br.g_min_of(0.05, 6, gain, 0b101).tolist()
    with pytest.raises(ValueError, match="lead 3"):
        BeatSpec(leads=(3,)).params(100, gain)
    with pytest.raises(ValueError, match="no lead"):
        BeatSpec(leads=()).params(100, gain)
    assert B.capacity(700, 7) == 88 and B.capacity(1, 1) == 1 and B.capacity(10, 1024) == 1


def test_summarize_on_a_hand_written_table():
    big = 2 ** 31 - 1
    rows = [br.rhythm_row(x, 10) for x in ([], [17], [10, 110], [10, 110, 200, 305], [0, 100, 200, 300, 400])]
    assert rows[0] == [0, -1, -1, 0, big, 0, 0, 0]
    s = B.summarize(torch.tensor([rows], dtype=torch.int64), 200.0)
    assert all(v.dtype == torch.float64 and tuple(v.shape) == (1, 5) for v in s.values())
    assert sorted(s) == ["heart_rate", "pnn", "rmssd_ms", "sdnn_ms"]
    for name in s:                                                  # fewer than 2 beats: NaN everywhere
        assert torch.isnan(s[name][0, :2]).all(), name
    assert s["heart_rate"][0, 2].item() == 60.0 * 200.0 * 1 / 100 and s["sdnn_ms"][0, 2].item() == 0.0
    assert torch.isnan(s["rmssd_ms"][0, 2]) and torch.isnan(s["pnn"][0, 2])                 # 2 beats: no successive difference
    rr = np.array([100.0, 90.0, 105.0])
    assert s["heart_rate"][0, 3].item() == pytest.approx(60.0 * 200.0 * 3 / 295, rel=1e-12)
    assert s["sdnn_ms"][0, 3].item() == pytest.approx(rr.std() * 5.0, rel=1e-9)
    assert s["rmssd_ms"][0, 3].item() == pytest.approx(math.sqrt((100 + 225) / 2) * 5.0, rel=1e-12)
    assert s["pnn"][0, 3].item() == 0.5
    assert s["heart_rate"][0, 4].item() == 120.0 and s["sdnn_ms"][0, 4].item() == 0.0       # a metronome
    assert s["rmssd_ms"][0, 4].item() == 0.0 and s["pnn"][0, 4].item() == 0.0
    with pytest.raises(ValueError, match="rhythm must be"):
        B.summarize(torch.zeros(2, 3, 7, dtype=torch.int64), 100)


# ---------------------------------------------------------------------------------------------------------------------
# detector quality on the synthetic ECG, asserted on the restatement with BeatSpec() defaults
# ---------------------------------------------------------------------------------------------------------------------
def _found(d, fs):
    p = BeatSpec().params(fs, np.full(12, 1000.0))
    return br.beats(d, p["s"], p["h"], p["ref"], p["blk"], p["num"], p["den"], int(p["g_min"][0]))


@pytest.mark.parametrize("fs", [100, 250, 360, 500])
@pytest.mark.parametrize("hr,jitter,noise", [(72, 0.05, 0.01), (45, 0.02, 0.03), (150, 0.10, 0.02)])
def test_detector_finds_the_planted_beats(fs, hr, jitter, noise):
    d, planted = br.synth(fs, 30, hr, jitter, noise, seed=fs + hr)
    found = _found(d, fs)
    tol = 0.050 * fs
    off = np.abs(found[:, None] - planted[None, :])
    print(f"fs={fs} hr={hr}: planted {len(planted)} found {len(found)} largest offset {off.min(0).max()} samples")
    assert len(planted) >= 20
    assert (off.min(0) <= tol).all(), "a planted beat has no detection within 50 ms"
    assert (off.min(1) <= tol).all(), "a detection is farther than 50 ms from every planted beat"
    assert len(found) == len(planted)


def test_noise_alone_gives_no_beat():
    d = np.round(10.0 * np.random.default_rng(5).standard_normal((3000, 12))).astype(np.int16)
    assert len(_found(d, 100)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the ABI's refusals (null pointers: nothing is launched)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_on_the_host():
    import ecg_hip
    from ecg_hip import _lib
    lib = ecg_hip.load()
    ok = dict(R=1, Ttot=1000, leads=12, mask=0xFFF, s=1, h=6, ref=25, blk=200, num=3, den=8)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.ecg_wfdb16_beats(None, None, None, None, None, a["R"], a["Ttot"], a["leads"], a["mask"], a["s"], a["h"],
                                  a["ref"], a["blk"], a["num"], a["den"], None)
        return rc, _lib.last_error()

    assert call() == (1, "wfdb16_beats: null pointer")              # every integer in range: the pointers are what is wrong
    for kw, msg in ((dict(h=256), "h=256"), (dict(h=-1), "h=-1"), (dict(ref=0), "ref=0"), (dict(ref=1025), "ref=1025"),
                    (dict(blk=15), "blk=15"), (dict(blk=2 ** 20 + 1), "blk="), (dict(num=9), "num=9"), (dict(num=0), "num=0"),
                    (dict(den=1025, num=3), "den=1025"), (dict(mask=0), "lead_mask"), (dict(mask=0x1000), "lead_mask"),
                    (dict(s=0), "s=0"), (dict(s=65), "s=65"), (dict(leads=17), "leads=17"), (dict(Ttot=2 ** 30 + 1), "Ttot="),
                    (dict(Ttot=0), "Ttot=0"), (dict(R=0), "R=0")):
        rc, err = call(**kw)
        assert rc == 1 and msg in err, (kw, err)
    # the size helper is pure: 0 for sizes the call refuses, otherwise room for g and the rest
    assert lib.ecg_wfdb16_beats_workspace_bytes(2, 1000, 200) >= 2 * 1000 * 4
    assert lib.ecg_wfdb16_beats_workspace_bytes(2, 1000, 15) == 0 and lib.ecg_wfdb16_beats_workspace_bytes(0, 1000, 200) == 0
    assert lib.ecg_wfdb16_beats_workspace_bytes(1, 2 ** 30, 2 ** 20) >= 2 ** 32
    assert lib.ecg_wfdb16_beats_chunk() == B.chunk() >= 256

    def rhythm(Ttot=1000, cap=39, T=100, first=0, hop=50, W=19, last=-1, up=1, down=1, Tq=100, nn=0):
        rc = lib.ecg_beats_rhythm(None, None, None, 1, Ttot, cap, T, first, hop, W, last, up, down, Tq, nn, None)
        return rc, _lib.last_error()

    assert rhythm() == (1, "beats_rhythm: null pointer")
    for kw, msg in ((dict(W=20), "past"), (dict(up=513), "up=513"), (dict(Tq=99), "Tq=99"), (dict(nn=-1), "nn_delta"),
                    (dict(cap=0), "cap=0"), (dict(hop=0), "hop"), (dict(up=2, down=5, Tq=250), "past")):
        rc, err = rhythm(**kw)
        assert rc == 1 and msg in err, (kw, err)
    assert rhythm(up=2, down=5, Tq=250, W=7) == (1, "beats_rhythm: null pointer")           # 400 model samples: 7 windows fit
