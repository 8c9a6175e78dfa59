"""GPU checks of the beat-morphology stage (ecg_beats_sum, ecg_beats_match, ecg_beats_series_mean): every output EQUALS the
numpy restatement (tests/template_ref.py) — integers with ==, the fp32 series mean bit for bit (NaNs in the same places);
a row depends on its recording only; bad arguments are refused before any launch; score_recording(template=) adds its
fields, equal to the restatement fed the device's beats, and changes nothing else, and nothing at all with template=None.

Every stream, template and series is a slice out of the middle of a larger buffer filled with 12345, starting at an odd
element offset: a read outside it changes a value and faults nothing."""
import functools

import numpy as np
import pytest
import torch

import beats_ref as br
import template_ref as tr
from input_util import GUARD, _model, _score, dev, guarded, hip, host, unchanged  # noqa: F401

pytestmark = pytest.mark.gpu

INV = -32768


def S():
    from ecg_hip import template as T
    return T.slab()


def inc_dev(include):
    return None if include is None else dev(include)


# ---------------------------------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------------------------------
SUM_NAMES = ["one-sample", "edges", "37x5", "limit", "past-2^31"]


@functools.lru_cache(maxsize=None)
def sum_case(name):
    """-> dict(d [2, Ttot, leads], pos [2, cap], n [2], include [2, cap], pre, post) and the restatement, made once."""
    rng = np.random.default_rng(sum(map(ord, name)))
    s = S()
    if name == "one-sample":                # Ttot = 1, leads = 1, pre = post = 0: position 0 is the only whole one
        d = np.array([[[7]], [[INV]]], np.int16)
        pos, n = np.array([[0, 0, -1, 0], [0, 1, 5, 0]], np.int32), np.array([3, 3], np.int32)
        include, pre, post = np.array([[1, 9, 1, 1], [1, 1, 1, 1]], np.uint8), 0, 0
    elif name == "edges":
        Ttot, leads, pre, post = 50, 3, 4, 6
        d = rng.integers(-3000, 3001, size=(2, Ttot, leads)).astype(np.int16)
        # pre and Ttot-1-post are whole, one sample beyond each is skipped; -1 inside n; duplicates and overlaps; junk past n
        pos = np.array([[pre, pre - 1, Ttot - 1 - post, Ttot - post, -1, 10, 10, 12, 20, 25],
                        [30, 9, 9, 9, 2 ** 31 - 1, 11, -1, 43, 4, 15]], np.int32)
        n = np.array([8, 9], np.int32)
        include = np.array([[1, 1, 255, 1, 1, 7, 1, 128, 1, 1], [1, 0, 3, 1, 1, 0, 1, 1, 1, 1]], np.uint8)
        d[0, 10 - pre + 2, 1] = d[0, 12, 0] = d[1, 9, 2] = d[1, Ttot - 1, 0] = INV      # invalid samples at chosen (t, l)
        d[1, 5:9, 1] = INV
    elif name == "37x5":                    # Lseg*leads = 185, no multiple of 64; more than two slabs and a remainder
        Ttot, leads, pre, post = 900, 5, 15, 21
        cap = 2 * s + 7 + 5
        d = rng.integers(-32767, 32768, size=(2, Ttot, leads)).astype(np.int16)
        d[rng.random(d.shape) < 0.02] = INV
        pos = rng.integers(0, Ttot, size=(2, cap)).astype(np.int32)                     # not ascending, some not whole
        pos[0, 3] = pos[0, 2 * s + 1] = -1
        n = np.array([2 * s + 7, s + 1], np.int32)
        include = (rng.random((2, cap)) < 0.8).astype(np.uint8) * 200
    elif name == "limit":                   # Lseg = 1024, leads = 16
        Ttot, leads, pre, post = 1500, 16, 500, 523
        d = rng.integers(-32767, 32768, size=(2, Ttot, leads)).astype(np.int16)
        d[0, 700:720, 3] = INV
        pos = np.array([[500, 976, 700, 499, 977, 650], [976, 976, 500, -1, 800, 600]], np.int32)
        n, include = np.array([6, 5], np.int32), np.ones((2, 6), np.uint8)
    else:                                   # 70 000 beats of +-32767: the sums pass 2^31
        Ttot, leads, pre, post = 8, 2, 1, 1
        d = np.stack([np.full((Ttot, leads), 32767, np.int16), np.full((Ttot, leads), -32767, np.int16)])
        pos = rng.integers(1, Ttot - 1, size=(2, 70000)).astype(np.int32)
        n, include = np.array([70000, 69999], np.int32), np.ones((2, 70000), np.uint8)
    want = tr.sums(d, pos, n, pre, post, include)
    want_all = tr.sums(d, pos, n, pre, post, None)
    dd, big = guarded(d)
    assert dd.data_ptr() % 4 == 2
    return dict(d=d, dd=dd, big=big, pos=pos, n=n, include=include, pre=pre, post=post, want=want, want_all=want_all)


def test_the_sum_cases_cover_what_they_claim():
    s = S()
    assert s >= 2
    c = sum_case("one-sample")
    assert c["want"][0].flatten().tolist() == [14, 0] and c["want"][1].flatten().tolist() == [2, 0]
    c = sum_case("edges")
    assert c["want"][1].max() >= 3 and not np.array_equal(c["want"][1], c["want_all"][1])      # include matters
    assert len(np.unique(c["want"][1][0])) >= 3                                              # invalid samples left gaps
    c = sum_case("37x5")
    assert (c["pre"] + c["post"] + 1) * 5 == 185 and c["n"][0] > 2 * s and c["n"][0] % s
    c = sum_case("limit")
    assert c["want"][0].shape == (2, 1024, 16) and c["want"][1][0].max() == 4 == c["want"][1][1].max()
    c = sum_case("past-2^31")
    assert c["want"][0][0].max() > 2 ** 31 and c["want"][0][1].min() < -2 ** 31


@pytest.mark.parametrize("name", SUM_NAMES)
def test_sums_equal_the_restatement(hip, name):
    c = sum_case(name)
    pos, n = dev(c["pos"]), dev(c["n"])
    for include, want in ((c["include"], c["want"]), (None, c["want_all"])):
        s, k = hip.beats_sum(c["dd"], pos, n, c["pre"], c["post"], include=inc_dev(include))
        assert s.dtype == torch.int64 and k.dtype == torch.int32 and tuple(s.shape) == want[0].shape == tuple(k.shape)
        assert np.array_equal(host(s), want[0]) and np.array_equal(host(k), want[1])
    assert unchanged(c)
    # a bool mask is the same mask; row r equals the call on recording r alone, inside another guard value
    sb, kb = hip.beats_sum(c["dd"], pos, n, c["pre"], c["post"], include=dev(c["include"] != 0))
    assert np.array_equal(host(sb), c["want"][0]) and np.array_equal(host(kb), c["want"][1])
    for r in range(2):
        s1, k1 = hip.beats_sum(guarded(c["d"][r:r + 1], -777)[0], pos[r:r + 1], n[r:r + 1], c["pre"], c["post"],
                               include=dev(c["include"][r:r + 1]))
        assert np.array_equal(host(s1)[0], c["want"][0][r]) and np.array_equal(host(k1)[0], c["want"][1][r])


# ---------------------------------------------------------------------------------------------------------------------
# match
# ---------------------------------------------------------------------------------------------------------------------
MATCH_NAMES = ["j0", "j64", "zero-template", "masked", "too-short", "extreme"]


@functools.lru_cache(maxsize=None)
def match_case(name):
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    mask, include = None, None
    if name == "too-short":                 # Ttot < Lseg: no entry has a candidate
        Ttot, leads, pre, post, J = 10, 2, 5, 7, 3
        d = rng.integers(-100, 101, size=(2, Ttot, leads)).astype(np.int16)
        tmpl = rng.integers(-100, 101, size=(2, 13, leads)).astype(np.int16)
        pos, n = np.array([[0, 5, 9], [4, 4, -1]], np.int32), np.array([3, 3], np.int32)
    elif name == "extreme":                 # 1024 x 16 x J = 64, +-32767 everywhere: scores near 2^44
        Ttot, leads, pre, post, J = 1300, 16, 500, 523, 64
        d = (rng.choice([-32767, 32767], size=(2, Ttot, leads))).astype(np.int16)
        tmpl = np.stack([d[0, 17:17 + 1024], -d[1, 100:100 + 1024]])                      # recording 0: the segment at 517 itself
        pos, n = np.array([[500, 560, 700, 776], [540, 600, 436, 840]], np.int32), np.array([4, 4], np.int32)
    else:
        Ttot, leads, pre, post = 400, 4, 5, 7
        J = 0 if name == "j0" else 64 if name == "j64" else 9
        d = rng.integers(-2000, 2001, size=(2, Ttot, leads)).astype(np.int16)
        d[rng.random(d.shape) < 0.03] = INV
        tmpl = rng.integers(-2000, 2001, size=(2, 13, leads)).astype(np.int16)
        tmpl[0, 3, 1] = tmpl[1, 0, 0] = tmpl[1, 12, 3] = INV
        # candidates cut by either end, an entry with none at J = 0 (2 < pre; Ttot-1 at any J <= post... cut), -1, junk past n
        pos = np.array([[0, 2, 5, 60, 200, 200, Ttot - 8, Ttot - 1, -1, 333, 100, 50],
                        [392, 391, 70, 3, 250, 64, 69, 5, 300, 301, 2 ** 31 - 1, 7]], np.int32)
        n = np.array([10, 11], np.int32)
        include = np.ones((2, 12), np.uint8)
        include[0, 4], include[1, 8] = 0, 0
        if name == "zero-template":
            tmpl[:] = 0
            tmpl[0, 3, 1] = INV
        if name == "masked":
            mask = 0b0101
        # plant the template in recording 0 at 203 + 4: entry 5 (position 200, included) finds lag 7 when J >= 7
        if name in ("j64", "masked"):
            d[0, 207 - pre:207 + post + 1] = np.where(tmpl[0] == INV, 0, tmpl[0])
    want = tr.match(d, pos, n, tmpl, pre, post, J, mask, include)
    dd, big = guarded(d)
    tt, tbig = guarded(tmpl, 54)
    assert dd.data_ptr() % 4 == 2 and tt.data_ptr() % 4 == 2
    return dict(d=d, dd=dd, big=big, tmpl=tmpl, tt=tt, tbig=tbig, pos=pos, n=n, include=include, pre=pre, post=post, J=J,
                mask=mask, want=want)


def test_the_match_cases_cover_what_they_claim():
    lag, m = match_case("j0")["want"]
    assert (lag == 0).all() and (m[0, 1] == 0).all() and (m[0, 0] == 0).all() and m[0, 2, 0, 0] >= 11     # 0, 2 < pre: none
    assert (m[0, 4] == 0).all() and m[0, 5, 0, 0] > 0 and (m[0, 8] == 0).all() and (m[0, 10:] == 0).all()    # include; -1; past n
    c = match_case("j64")
    lag, m = c["want"]
    assert lag[0, 5] == 7 and lag.min() < -20 and lag.max() > 20
    assert lag[0, 0] >= 5 and lag[0, 7] <= -7 and (m[0, 0, :, 0] > 0).all()                             # cut by either end
    assert (m[..., 0][m[..., 0] > 0] < 13).any()                                                         # invalid pairs left out
    c = match_case("zero-template")
    lag, _ = c["want"]
    assert lag[0, :4].tolist() == [5, 3, 0, -9] and lag[0, 6] == -9 and lag[0, 7] == -9                  # the most negative candidate
    a, b = match_case("masked"), match_case("j64")
    assert not np.array_equal(a["want"][0], tr.match(a["d"], a["pos"], a["n"], a["tmpl"], 5, 7, 9, None, a["include"])[0])
    assert (a["want"][1][0, 3, [1, 3], 0] > 0).all()                                                    # fields of the leads left out
    assert (match_case("too-short")["want"][1] == 0).all()
    lag, m = match_case("extreme")["want"]
    assert lag[0, 0] == 17 and m[0, 0, 0].tolist()[5] == 1024 * 32767 ** 2 and m[0, 0, 0].tolist()[6] == 0
    assert b["J"] == 64


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_match_equals_the_restatement(hip, name):
    c = match_case(name)
    pos, n = dev(c["pos"]), dev(c["n"])
    lag, m = hip.beats_match(c["dd"], pos, n, c["tt"], c["pre"], c["post"], c["J"], lead_mask=c["mask"],
                             include=inc_dev(c["include"]))
    leads = c["d"].shape[2]
    assert lag.dtype == torch.int32 and m.dtype == torch.int64 and tuple(m.shape) == c["pos"].shape + (leads, 7)
    bad = np.argwhere(host(lag) != c["want"][0])
    assert len(bad) == 0, [(tuple(i), host(lag)[tuple(i)], c["want"][0][tuple(i)]) for i in bad[:8]]
    bad = np.argwhere(host(m) != c["want"][1])
    assert len(bad) == 0, [(tuple(i), host(m)[tuple(i)], c["want"][1][tuple(i)]) for i in bad[:8]]
    assert unchanged(c) and unchanged(dict(big=c["tbig"], d=c["tmpl"]), 54)
    for r in range(2):                                      # row r equals the call on recording r alone
        l1, m1 = hip.beats_match(guarded(c["d"][r:r + 1], -777)[0], pos[r:r + 1], n[r:r + 1], dev(c["tmpl"][r:r + 1]), c["pre"],
                                 c["post"], c["J"], lead_mask=c["mask"],
                                 include=None if c["include"] is None else dev(c["include"][r:r + 1]))
        assert torch.equal(l1[0], lag[r]) and torch.equal(m1[0], m[r])


# ---------------------------------------------------------------------------------------------------------------------
# series mean
# ---------------------------------------------------------------------------------------------------------------------
RATIOS = [(1, 1), (1, 5), (5, 1), (25, 32)]


@functools.lru_cache(maxsize=None)
def series_case(up, down):
    """Rows of list lengths slab-1, slab, slab+1, 2*slab, 2*slab+5 and 0 (R = 6), positions not ascending, a NaN in x."""
    s = S()
    rng = np.random.default_rng(up * 1000 + down)
    Ttot, K, pre, post = 600, 3, 7, 9
    lens = [s - 1, s, s + 1, 2 * s, 2 * s + 5, 0]
    R, cap = len(lens), 2 * s + 9
    Tx = (Ttot - 1) * up // down - 1                                     # the last source samples map past Tx - 1: the clamp
    x = (rng.standard_normal((R, K, Tx)) * 100).astype(np.float32)
    x[:, 1, 200 * up // down] = np.nan                                   # the image of source sample 200
    x[2, 2, Tx - 1] = np.nan                                             # met through the clamp only
    pos = rng.integers(0, Ttot, size=(R, cap)).astype(np.int32)          # some without a whole segment
    pos[:, 1], pos[:, 2] = Ttot - 1 - post, pre
    pos[0, 5] = pos[3, 0] = -1
    pos[2, s] = Ttot - 1 - post                                          # the one entry of row 2's second slab
    include = (rng.random((R, cap)) < 0.85).astype(np.uint8)
    include[2, s] = 1
    n = np.array(lens, np.int32)
    want = tr.series_mean(x, pos, n, Ttot, pre, post, up, down, s, include)
    xx, big = guarded(x, 12345.0)
    return dict(x=x, xx=xx, big=big, pos=pos, n=n, include=include, Ttot=Ttot, pre=pre, post=post, want=want)


@pytest.mark.parametrize("up,down", RATIOS)
def test_series_mean_equals_the_restatement(hip, up, down):
    c = series_case(up, down)
    want, count = c["want"]
    assert count[5] == 0 and (want[5] == 0).all() and count[:5].min() >= S() // 2
    nan = np.isnan(want)
    assert nan[:5, 1].any() and not nan[:5, 1].all() and not nan[:, 0].any() and nan[2, 2].any()
    pos, n = dev(c["pos"]), dev(c["n"])
    out, k = hip.beats_series_mean(c["xx"], pos, n, c["Ttot"], c["pre"], c["post"], up, down, include=dev(c["include"]))
    assert out.dtype == torch.float32 and k.dtype == torch.int32 and tuple(out.shape) == want.shape
    assert np.array_equal(host(k), count)
    got = host(out)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & nan)))
    assert len(bad) == 0, [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:8]]
    assert np.array_equal(got, want, equal_nan=True)
    big = host(c["big"])                                     # the series holds NaNs: compared as bits
    assert np.array_equal(big[GUARD:-GUARD].view(np.int32), c["x"].reshape(-1).view(np.int32))
    assert (big[:GUARD] == 12345.0).all() and (big[-GUARD:] == 12345.0).all()
    # include = None; and row r equals the call on recording r alone
    w2 = tr.series_mean(c["x"], c["pos"], c["n"], c["Ttot"], c["pre"], c["post"], up, down, S(), None)
    o2, k2 = hip.beats_series_mean(c["xx"], pos, n, c["Ttot"], c["pre"], c["post"], up, down)
    assert np.array_equal(host(o2), w2[0], equal_nan=True) and np.array_equal(host(k2), w2[1])
    for r in (2, 4, 5):
        o1, k1 = hip.beats_series_mean(guarded(c["x"][r:r + 1], -1.0)[0], pos[r:r + 1], n[r:r + 1], c["Ttot"], c["pre"],
                                       c["post"], up, down, include=dev(c["include"][r:r + 1]))
        assert np.array_equal(host(o1)[0], want[r], equal_nan=True) and int(k1[0]) == count[r]


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(hip):
    from ecg_hip import EcgHipError, _lib as L
    R, Ttot, leads, cap, pre, post, K, Tx = 1, 100, 3, 4, 2, 3, 2, 100
    d, _ = guarded(np.ones((R, Ttot, leads), np.int16))
    pos, n = dev(np.array([[10, 20, 30, 40]], np.int32)), dev(np.array([4], np.int32))
    tmpl = dev(np.ones((R, 6, leads), np.int16))
    x = dev(np.ones((R, K, Tx), np.float32))
    full = lambda shape, dt: torch.full(shape, 77, dtype=dt, device="cuda")        # noqa: E731
    s, c = full((R, 6, leads), torch.int64), full((R, 6, leads), torch.int32)
    lag, m = full((R, cap), torch.int32), full((R, cap, leads, 7), torch.int64)
    out, count = full((R, K, 6), torch.float32), full((R,), torch.int32)
    ws = torch.zeros(max(16, L.query("ecg_beats_series_mean_workspace_bytes", R, K, cap, 6)), dtype=torch.uint8, device="cuda")
    p = L.ptr

    def sum_(R=R, Ttot=Ttot, leads=leads, cap=cap, pre=pre, post=post, d=d, s=s):
        L.call("ecg_beats_sum", p(d), p(pos), p(n), None, p(s), p(c), R, Ttot, leads, cap, pre, post, L.stream())

    def match_(R=R, Ttot=Ttot, leads=leads, cap=cap, pre=pre, post=post, J=2, mask=7, tmpl=tmpl):
        L.call("ecg_beats_match", p(d), p(pos), p(n), None, p(tmpl), p(lag), p(m), R, Ttot, leads, cap, pre, post, J, mask,
               L.stream())

    def series_(R=R, K=K, Tx=Tx, Ttot=Ttot, cap=cap, pre=pre, post=post, up=1, down=1, ws=ws):
        L.call("ecg_beats_series_mean", p(x), p(pos), p(n), None, p(out), p(count), p(ws), R, K, Tx, Ttot, cap, pre, post, up,
               down, L.stream())

    shared = (dict(R=0), "R=0"), (dict(Ttot=0), "Ttot=0"), (dict(Ttot=2 ** 30 + 1), "Ttot="), (dict(cap=0), "cap=0"), \
        (dict(pre=-1), "pre=-1"), (dict(post=-1), "post=-1"), (dict(pre=1000, post=24), "Lseg=1025")
    for fn in (sum_, match_, series_):
        for kw, msg in shared:
            with pytest.raises(EcgHipError, match=msg):
                fn(**kw)
    for fn in (sum_, match_):
        for kw, msg in ((dict(leads=0), "leads=0"), (dict(leads=17), "leads=17")):
            with pytest.raises(EcgHipError, match=msg):
                fn(**kw)
    for kw, msg in ((dict(J=-1), "J=-1"), (dict(J=65), "J=65"), (dict(mask=0), "lead_mask"), (dict(mask=8), "lead_mask"),
                    (dict(tmpl=None), "null pointer")):
        with pytest.raises(EcgHipError, match=msg):
            match_(**kw)
    for kw, msg in ((dict(up=0), "up=0"), (dict(up=513), "up=513"), (dict(down=0), "down=0"), (dict(down=513), "down=513"),
                    (dict(K=0), "K=0"), (dict(K=65536), "K=65536"), (dict(Tx=0), "Tx=0"), (dict(ws=None), "null pointer"),
                    (dict(ws=ws[1:]), "aligned")):
        with pytest.raises(EcgHipError, match=msg):
            series_(**kw)
    for kw in (dict(d=None), dict(s=None)):
        with pytest.raises(EcgHipError, match="null pointer"):
            sum_(**kw)
    # the integer limits come first: they can be asked with NULL pointers
    with pytest.raises(EcgHipError, match="Lseg=1025"):
        L.call("ecg_beats_sum", None, None, None, None, None, None, 1, 5000, 12, 10, 1024, 0, L.stream())
    with pytest.raises(EcgHipError, match="J=65"):
        L.call("ecg_beats_match", None, None, None, None, None, None, None, 1, 5000, 12, 10, 8, 12, 65, 0xFFF, L.stream())
    with pytest.raises(EcgHipError, match="down=513"):
        L.call("ecg_beats_series_mean", None, None, None, None, None, None, None, 1, 1, 100, 5000, 10, 8, 12, 1, 513, L.stream())
    assert L.query("ecg_beats_series_mean_workspace_bytes", 1, 65536, 4, 6) == 0
    assert L.query("ecg_beats_series_mean_workspace_bytes", 1, 2, 4, 1025) == 0
    assert L.query("ecg_beats_series_mean_workspace_bytes", 2, 3, 2 * S() + 1, 6) == 4 * (2 * 3 * 3 * 6 + 2 * 3)
    torch.cuda.synchronize()
    for t in (s, c, lag, m, count):
        assert bool((t == 77).all())
    assert bool((out == 77).all()) and not bool(ws.any())
    # the wrappers' own checks
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.beats_sum(d.cpu(), pos, n, pre, post)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hip.beats_sum(d, pos.cpu(), n, pre, post)
    with pytest.raises(EcgHipError, match="int32"):
        hip.beats_sum(d, pos.long(), n, pre, post)
    with pytest.raises(EcgHipError, match="include"):
        hip.beats_sum(d, pos, n, pre, post, include=pos)
    with pytest.raises(EcgHipError, match="tmpl"):
        hip.beats_match(d, pos, n, tmpl[:, :5], pre, post, 2)
    with pytest.raises(EcgHipError, match="float32"):
        hip.beats_series_mean(x.double(), pos, n, Ttot, pre, post)
    # and the calls these were made from go through
    sum_(), match_(), series_()
    torch.cuda.synchronize()
    assert int(count[0]) == 4 and bool((c == 4).all()) and bool((lag == -2).all())      # all-ones: every score ties


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
OLD = ("logits", "prob", "finite", "prob_max", "prob_mean", "cam", "cover", "quality", "lead_ok", "usable", "beats", "n_beats",
       "rhythm", "heart_rate")
NEW = ("beat_pos", "beat_lag", "beat_ok", "beat_corr", "template", "template_n", "cam_beat", "cam_beat_n")


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.is_floating_point():
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    return torch.equal(a, b)


def against_the_restatement(s, d, gain, base, fs, up, down, spec=None):
    """The template fields of score s equal the restatement fed the device's own beats (and, for cam_beat, its cam)."""
    from ecg_hip.template import TemplateSpec
    spec = spec or TemplateSpec()
    cam = None if s.cam is None else host(s.cam)
    want = tr.stage(d, gain, base, host(s.beats), host(s.n_beats), tr.params(fs), spec.min_corr, spec.passes, None, cam,
                    None if s.cam is None else host(s.cover), up, down, S())
    assert s.beat_pos.dtype == torch.int32 and s.beat_lag.dtype == torch.int32 and s.beat_ok.dtype == torch.bool
    assert s.beat_corr.dtype == torch.float64 and s.template.dtype == torch.float64 and s.template_n.dtype == torch.int32
    for name in ("beat_lag", "beat_pos", "beat_ok", "template_n"):
        assert np.array_equal(host(getattr(s, name)), want[name]), name
    for name in ("beat_corr", "template"):
        assert np.array_equal(host(getattr(s, name)), want[name], equal_nan=True), name
    assert s.template_offsets == want["template_offsets"] and len(s.template_offsets) == s.template.shape[1]
    if cam is not None:
        assert s.cam_beat.dtype == torch.float32 and tuple(s.cam_beat.shape) == (d.shape[0], cam.shape[1], s.template.shape[1])
        assert np.array_equal(host(s.cam_beat), want["cam_beat"], equal_nan=True)
        assert np.array_equal(host(s.cam_beat_n), want["cam_beat_n"])
    else:
        assert s.cam_beat is None and s.cam_beat_n is None
    return want


def _end_to_end(fs, model_fs, up, down, **kw):
    model = _model()
    d = np.stack([br.synth(fs, 35, 72, 0.05, 0.01, seed=1)[0], br.synth(fs, 35, 110, 0.10, 0.02, seed=2)[0]])
    gain, base = np.full((2, 12), 1000.0), np.full((2, 12), 3, np.int32)
    c = dict(d=d)
    dd, c["big"] = guarded(d)
    args = (model, dd, dev(gain), dev(base))
    kw = dict(kw, window=1000, fs=fs, model_fs=model_fs, beats=True)
    s, plain = _score(*args, template=True, **kw), _score(*args, template=None, **kw)
    want = against_the_restatement(s, d, gain, base, fs, up, down)
    nb = host(s.n_beats)
    ok = host(s.beat_ok)
    assert nb.min() >= 35 and all(ok[r, :nb[r]].mean() > 0.9 for r in range(2)) and not ok[0, nb[0]:].any()
    assert np.abs(host(s.beat_lag)).max() >= 1 and host(s.template_n).max() >= 30
    for name in OLD:
        assert same(getattr(s, name), getattr(plain, name)), name
    for name in NEW + ("template_offsets",):
        assert getattr(plain, name) is None, name
    assert unchanged(c)
    return s, want


def test_score_recording_with_a_template(hip):
    s, want = _end_to_end(100, None, 1, 1, cam_classes=[1], quality=True)
    assert s.template.shape == (2, 71, 12) and s.cam_beat.shape == (2, 1, 71) and int(s.cam_beat_n.min()) >= 30
    # the mean beat has its complex at offset 0: the largest excursion of some lead lies within 30 ms of it
    t = np.nan_to_num(host(s.template)[0])
    t = np.abs(t - np.median(t, 0))
    assert abs(int(np.argmax(t.max(1))) - 25) <= 3


def test_score_recording_with_a_template_on_a_resampled_recording(hip):
    """fs = 250 -> model_fs = 100: positions and template on the source axis, the CAM read through up/down = 2/5."""
    s, want = _end_to_end(250, 100, 2, 5, cam_classes=[0, 3])
    assert s.fs == 100 and s.template.shape == (2, 177, 12) and s.cam_beat.shape == (2, 2, 177)
    assert int(s.beat_pos.max()) > 3500


def test_uncovered_samples_keep_beats_out_of_the_cam_mean(hip):
    """tail="drop" leaves the end of the recording without a CAM: the beats whose range reaches it take no part in cam_beat,
    and still take part in the template."""
    model = _model()
    d = br.synth(100, 38, 80, 0.05, 0.01, seed=5)[0][None]
    gain, base = np.full((1, 12), 1000.0), np.zeros((1, 12), np.int32)
    s = _score(model, guarded(d)[0], dev(gain), dev(base), window=1000, fs=100, beats=True, template=True, cam_classes=[2],
               tail="drop")
    want = against_the_restatement(s, d, gain, base, 100, 1, 1)
    assert int((host(s.cover) == 0).sum()) == 300
    assert (want["beat_ok"] & ~want["cam_include"]).sum() >= 2 and int(s.cam_beat_n[0]) == want["cam_include"].sum()
    assert int(s.cam_beat_n[0]) < host(s.template_n).max()


def test_without_a_template_nothing_new_is_reached(hip, monkeypatch):
    from ecg_hip.template import TemplateSpec
    model = _model()
    d = br.synth(100, 20, 80, 0.05, 0.01, seed=3)[0][None]
    args = (model, dev(d), dev(np.full((1, 12), 1000.0)), dev(np.zeros((1, 12), np.int32)))
    with pytest.raises(ValueError, match="beats="):
        _score(*args, window=1000, fs=100, template=True)
    with pytest.raises(ValueError, match="fs"):
        _score(*args, window=1000, beats=True, template=True)
    with pytest.raises(ValueError, match="TemplateSpec"):
        _score(*args, window=1000, fs=100, beats=True, template="yes")
    loose = _score(*args, window=1000, fs=100, beats=True, template=TemplateSpec(leads=(0, 1, 7), passes=1, min_corr=0.5))
    assert int(loose.beat_ok.sum()) >= 20 and loose.cam_beat is None
    base = _score(*args, window=1000, fs=100, beats=True)

    def boom(*a, **kw):
        raise AssertionError("a template entry point was called")

    for name in ("beats_sum", "beats_match", "beats_series_mean"):
        monkeypatch.setattr(hip, name, boom)
    for kw in (dict(), dict(template=None)):
        s = _score(*args, window=1000, fs=100, beats=True, **kw)
        for name in OLD:
            assert same(getattr(s, name), getattr(base, name)), name
        assert s.template is None and s.beat_ok is None
    with pytest.raises(AssertionError, match="template entry point"):
        _score(*args, window=1000, fs=100, beats=True, template=True)


def test_score_wfdb_record_passes_the_template_through(hip, tmp_path):
    from ecg_hip import wfdbraw
    from ecg_hip.recording import score_wfdb_record
    d, planted = br.synth(250, 20, 66, 0.05, 0.01, seed=4)
    gain, base = np.full(12, 1000.0), np.zeros(12, np.int32)
    wfdbraw.write_raw_record(str(tmp_path / "strip"), d.astype(np.int64), 250, gain, base, fmt=16)
    s = score_wfdb_record(str(tmp_path / "strip"), _model(), model_fs=100, window=1000, beats=True, template=True)
    against_the_restatement(s, d[None], gain[None], base[None], 250, 2, 5)
    assert int(s.beat_ok.sum()) == len(planted)
