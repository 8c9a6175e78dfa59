"""CPU checks of the beat-morphology stage: the numpy restatement (tests/template_ref.py) against literal per-element
loops on tiny inputs, ecg_hip/template.py (params, mean_template, correlation, beat_correlation, physical) on exact cases
and against the restatement, and the separation the stage exists for: on twelve synthetic recordings the restatement's
beat_ok under TemplateSpec() is False for the three planted wide beats and True for every other beat."""
import functools

import numpy as np
import pytest
import torch

import beats_ref as br
import template_ref as tr

INV = -32768


def small(seed, R=2, Ttot=40, leads=3, cap=9):
    rng = np.random.default_rng(seed)
    d = rng.integers(-50, 51, size=(R, Ttot, leads)).astype(np.int16)
    d[rng.random(d.shape) < 0.1] = INV
    pos = rng.integers(-1, Ttot, size=(R, cap)).astype(np.int32)        # some -1, not ascending, duplicates likely
    pos[0, 1] = pos[0, 0]
    n = np.array([cap - 2, cap], np.int32)[:R]
    include = (rng.random((R, cap)) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=(R, cap)).astype(np.uint8)
    return d, pos, n, include


def is_listed(pos, n, include, r, i):
    return i < n[r] and pos[r, i] >= 0 and (include is None or include[r, i] != 0)


@pytest.mark.parametrize("with_include", [False, True])
def test_sums_against_the_literal_loops(with_include):
    d, pos, n, include = small(1)
    include = include if with_include else None
    pre, post = 2, 3
    R, Ttot, leads = d.shape
    s, c = np.zeros((R, 6, leads), np.int64), np.zeros((R, 6, leads), np.int32)
    for r in range(R):
        for i in range(pos.shape[1]):
            x = int(pos[r, i])
            if not is_listed(pos, n, include, r, i) or x - pre < 0 or x + post >= Ttot:
                continue
            for t in range(6):
                for l in range(leads):
                    v = int(d[r, x - pre + t, l])
                    if v != INV:
                        s[r, t, l] += v
                        c[r, t, l] += 1
    got = tr.sums(d, pos, n, pre, post, include)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], s) and np.array_equal(got[1], c) and c.max() >= 2 and (c == 0).sum() == 0


@pytest.mark.parametrize("mask", [None, 0b101])
def test_match_against_the_literal_loops(mask):
    d, pos, n, include = small(2)
    rng = np.random.default_rng(3)
    pre, post, J = 2, 3, 4
    R, Ttot, leads = d.shape
    tmpl = rng.integers(-40, 41, size=(R, 6, leads)).astype(np.int16)
    tmpl[0, 2, 1] = INV
    pos[1, 0], pos[1, 1], pos[1, 2] = 0, Ttot - 1, 1               # candidates cut by either end
    lag, m = np.zeros(pos.shape, np.int32), np.zeros(pos.shape + (leads, 7), np.int64)
    for r in range(R):
        for i in range(pos.shape[1]):
            if not is_listed(pos, n, include, r, i):
                continue
            x, best, best_j = int(pos[r, i]), None, None
            for j in range(-J, J + 1):
                if x + j - pre < 0 or x + j + post >= Ttot:
                    continue
                score = 0
                for l in range(leads):
                    if mask is not None and not (mask >> l) & 1:
                        continue
                    for t in range(6):
                        v, q = int(d[r, x + j - pre + t, l]), int(tmpl[r, t, l])
                        if v != INV and q != INV:
                            score += v * q
                if best is None or score > best:
                    best, best_j = score, j
            if best is None:
                continue
            lag[r, i] = best_j
            for l in range(leads):
                for t in range(6):
                    v, q = int(d[r, x + best_j - pre + t, l]), int(tmpl[r, t, l])
                    if v != INV and q != INV:
                        m[r, i, l] += [1, v, v * v, q, q * q, v * q, abs(v - q)]
    got_lag, got_m = tr.match(d, pos, n, tmpl, pre, post, J, mask, include)
    assert np.array_equal(got_lag, lag) and np.array_equal(got_m, m)
    assert len(set(lag.flatten().tolist())) >= 4 and (m[..., 0] == 6).any() and (m[..., 0] == 5).any()


@pytest.mark.parametrize("up,down", [(1, 1), (2, 5), (5, 2)])
def test_series_mean_against_the_literal_loops(up, down):
    d, pos, n, include = small(4, cap=11)
    n = np.array([11, 7], np.int32)
    rng = np.random.default_rng(5)
    R, Ttot, K, pre, post, slab = 2, 40, 2, 2, 3, 4
    Tx = -(-Ttot * up // down) - 1                                   # one short: the clamp at Tx - 1 is reached
    x = rng.standard_normal((R, K, Tx)).astype(np.float32) * np.float32(1e3)
    want, count = np.zeros((R, K, 6), np.float32), np.zeros(R, np.int32)
    for r in range(R):
        take = [i for i in range(11) if is_listed(pos, n, include, r, i) and pos[r, i] - pre >= 0 and pos[r, i] + post < Ttot]
        count[r] = len(take)
        for k in range(K):
            for t in range(6):
                total = np.float32(0.0)
                for b in range(3):
                    partial = np.float32(0.0)
                    for i in take:
                        if b * slab <= i < (b + 1) * slab:
                            partial = np.float32(partial + x[r, k, min(Tx - 1, (int(pos[r, i]) - pre + t) * up // down)])
                    total = np.float32(total + partial)
                want[r, k, t] = np.float32(total / np.float32(count[r])) if count[r] else 0
    got, gcount = tr.series_mean(x, pos, n, Ttot, pre, post, up, down, slab, include)
    assert got.dtype == np.float32 and np.array_equal(gcount, count) and count.min() >= 3
    assert np.array_equal(got, want)
    # another slab size is another order: the same mean to rounding
    other, _ = tr.series_mean(x, pos, n, Ttot, pre, post, up, down, 64, include)
    assert np.allclose(other, want, rtol=1e-5, atol=1e-3)


def test_params_at_three_rates():
    from ecg_hip.template import TemplateSpec
    assert TemplateSpec().params(100) == dict(pre=25, post=45, match_pre=8, match_post=12, J=3)
    assert TemplateSpec().params(250) == dict(pre=63, post=113, match_pre=20, match_post=30, J=8)       # 62.5 and 112.5 round up
    assert TemplateSpec().params(500) == dict(pre=125, post=225, match_pre=40, match_post=60, J=15)
    assert TemplateSpec(max_lag_s=0.001).params(100)["J"] == 1
    for fs in (100, 250, 360, 500):
        assert TemplateSpec().params(fs) == tr.params(fs)
    assert TemplateSpec().lead_mask(12) == 0xFFF and TemplateSpec(leads=(0, 5)).lead_mask(12) == 0b100001
    with pytest.raises(ValueError, match="outside"):
        TemplateSpec(leads=(12,)).lead_mask(12)
    with pytest.raises(ValueError, match="no lead"):
        TemplateSpec(leads=()).lead_mask(12)
    spec = TemplateSpec()
    assert (spec.passes, spec.min_corr, spec.leads) == (2, 0.6, None)


def test_mean_template_rounding_and_centring():
    from ecg_hip.template import mean_template
    # one recording, one lead: sum / cnt = -3/2, 3/2, -1/2, 1/2, -5/2 (half-way values round up), 0/0, 7/3, -7/3, clamps
    s = np.array([-3, 3, -1, 1, -5, 0, 7, -7, 70000, -70000, 10], np.int64).reshape(1, -1, 1)
    c = np.array([2, 2, 2, 2, 2, 0, 3, 3, 2, 2, 1], np.int32).reshape(1, -1, 1)
    want = [-1, 2, 0, 1, -2, INV, 2, -2, 32767, -32767, 10]
    got = mean_template(torch.from_numpy(s), torch.from_numpy(c))
    assert got.dtype == torch.int16 and got.flatten().tolist() == want
    assert tr.mean_template(s, c).flatten().tolist() == want
    # centring: the floor-mean of the valid samples, (sum of the ten) // 10, per (recording, lead)
    vals = [-1, 2, 0, 1, -2, 2, -2, 35000, -35000, 10]
    mean = sum(vals) // 10
    assert mean == 1
    wantc = [max(-32767, min(32767, v - mean)) for v in vals]
    wantc.insert(5, INV)
    assert mean_template(torch.from_numpy(s), torch.from_numpy(c), centre=True).flatten().tolist() == wantc
    assert tr.mean_template(s, c, centre=True).flatten().tolist() == wantc
    # a negative floor-mean, two leads centred separately, a lead without any value
    s2 = np.array([[[-3, 10, 0], [-4, 20, 0], [0, 33, 0]]], np.int64)
    c2 = np.array([[[1, 1, 0], [1, 1, 0], [0, 1, 0]]], np.int32)
    got2 = mean_template(torch.from_numpy(s2), torch.from_numpy(c2), centre=True)[0].tolist()
    assert got2 == [[1, -11, INV], [0, -1, INV], [INV, 12, INV]]           # means -7 // 2 = -4 and 63 // 3 = 21
    assert np.array_equal(tr.mean_template(s2, c2, centre=True)[0], np.array(got2))
    rng = np.random.default_rng(0)
    s3, c3 = rng.integers(-10 ** 6, 10 ** 6, size=(3, 9, 4)), rng.integers(0, 40, size=(3, 9, 4)).astype(np.int32)
    for centre in (False, True):
        assert np.array_equal(mean_template(torch.from_numpy(s3), torch.from_numpy(c3), centre).numpy(), tr.mean_template(s3, c3, centre))


def fields_of(v, t):
    return tr.fields(np.asarray(v, np.int64), np.asarray(t, np.int64))


def test_correlation_on_exact_cases():
    from ecg_hip.template import beat_correlation, correlation
    t = [3, -7, 12, 0, 5, -32768, 9]
    rows = [fields_of(t, t),                                # the template itself: 1.0
            fields_of([-x if x != INV else x for x in t], t),   # negated: -1.0
            fields_of([4] * 7, t),                          # constant: a factor is 0 -> NaN
            fields_of([INV] * 6 + [5], t),                  # one pair: N < 2 -> NaN
            fields_of([1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 8])]
    assert rows[0][0] == 6 and rows[3][0] == 1
    m = np.array(rows, np.int64).reshape(1, 1, 5, 7)
    got = correlation(torch.from_numpy(m))[0, 0].numpy()
    assert got.dtype == np.float64
    assert got[0] == 1.0 and got[1] == -1.0 and np.isnan(got[2]) and np.isnan(got[3]) and 0.9 < got[4] < 1.0
    assert np.array_equal(got, tr.correlation(m)[0, 0], equal_nan=True)
    v, q = np.arange(1, 8.0), np.array([1, 2, 3, 4, 5, 6, 8.0])
    assert abs(got[4] - np.corrcoef(v, q)[0, 1]) < 1e-12
    # the lower median over the leads taking part that have a value: of (1, -1, r) it is r's neighbour below
    assert beat_correlation(torch.from_numpy(m))[0, 0].item() == got[4]             # sorted: -1, r, 1 -> r
    assert beat_correlation(torch.from_numpy(m), 0b00011)[0, 0].item() == -1.0       # of two values the lower
    assert np.isnan(beat_correlation(torch.from_numpy(m), 0b01100)[0, 0].item())     # none with a value
    for mask in (None, 0b00011, 0b01100, 0b10001):
        assert np.array_equal(beat_correlation(torch.from_numpy(m), mask).numpy(), tr.beat_correlation(m, mask), equal_nan=True)
    # extreme magnitudes stay exact: 1024 samples of +-32767
    big = np.where(np.arange(1024) % 2 == 0, 32767, -32767)
    mb = np.array([fields_of(big, big), fields_of(-big, big)], np.int64).reshape(1, 2, 1, 7)
    assert correlation(torch.from_numpy(mb)).flatten().tolist() == [1.0, -1.0]


def test_physical():
    from ecg_hip.template import physical
    t = np.array([[[100, -200], [INV, 50]]], np.int16)
    gain, base = np.array([[200.0, 400.0]]), np.array([[0, 50]], np.int32)
    got = physical(torch.from_numpy(t), torch.from_numpy(gain), torch.from_numpy(base)).numpy()
    assert got.dtype == np.float64 and np.array_equal(got, np.array([[[0.5, -0.625], [np.nan, 0.0]]]), equal_nan=True)
    assert np.array_equal(got, tr.physical(t, gain, base), equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# the separation check
# ---------------------------------------------------------------------------------------------------------------------
PLANTED = (5, 11, 20)
CONFIGS = [(fs, hr, seed) for fs in (100, 250, 500) for hr, seed in ((45, 1), (72, 2), (110, 3), (150, 4))]


def planted_recording(fs, hr, seed):
    """beats_ref.synth with a wide wave of 2 mV added to beats 5, 11 and 20, against the sign of every lead at the apex."""
    d, apex = br.synth(fs, 60, hr, 0.1, 0.02, seed)
    x = d.astype(np.float64)
    t = np.arange(d.shape[0])
    for b in PLANTED:
        sign = np.where(d[apex[b]] == 0, 1.0, -np.sign(d[apex[b]].astype(np.float64)))
        x += 2000.0 * sign[None, :] * np.exp(-0.5 * ((t[:, None] - (apex[b] + 0.020 * fs)) / (0.040 * fs)) ** 2)
    return np.clip(np.round(x), -32767, 32767).astype(np.int16), apex


@functools.lru_cache(maxsize=None)
def separation(fs, hr, seed):
    from ecg_hip.beats import BeatSpec
    from ecg_hip.template import TemplateSpec
    d, apex = planted_recording(fs, hr, seed)
    gain = np.full((1, 12), 1000.0)
    p = BeatSpec().params(fs, gain)
    beats, n = br.detect(d[None], p["s"], p["h"], p["ref"], p["blk"], p["num"], p["den"], br.g_min_of(0.05, p["h"], gain))
    spec = TemplateSpec()
    out = tr.stage(d[None], gain, np.zeros((1, 12), np.int32), beats, n, tr.params(fs), spec.min_corr, spec.passes)
    return beats[0, :n[0]], apex, out["beat_ok"][0, :n[0]], out["beat_corr"][0, :n[0]], out["beat_lag"][0, :n[0]]


@pytest.mark.parametrize("fs,hr,seed", CONFIGS)
def test_planted_wide_beats_are_told_from_the_others(fs, hr, seed):
    beats, apex, ok, corr, lag = separation(fs, hr, seed)
    assert len(beats) == len(apex)
    which = np.abs(beats[:, None] - apex[None, :]).argmin(1)                # the planted beat every detected beat belongs to
    assert np.array_equal(which, np.arange(len(apex)))
    planted = np.isin(which, PLANTED)
    print(f"fs={fs} hr={hr}: others min {np.nanmin(corr[~planted]):.3f}, planted max {np.nanmax(corr[planted]):.3f}, "
          f"lags {lag.min()}..{lag.max()}")
    assert not ok[planted].any(), corr[planted]
    assert ok[~planted].all(), (np.nonzero(~ok & ~planted)[0], corr[~ok & ~planted])
