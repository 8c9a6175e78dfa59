"""GPU checks of the operating points, the confusion at per-class thresholds and the reliability table
(ecg_metrics_operating, ecg_metrics_confusion, ecg_metrics_reliability, and their users in ecg_hip/metrics.py): every
integer equals the restatement (tests/operating_ref.py, itself held to scikit-learn by tests/test_operating_host.py), and
every ratio made from them has the restatement's bits.  Shapes are the smallest that can still go wrong: one lane, three
lanes, one wave row of four ranks per lane around 256, the 1 024-rank chunk of the walk minus one, exactly, plus one, and
2 049 ranks (three chunks)."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import metrics_ref as mr
import operating_ref as opr
from metrics_util import ROOT, dev, host, metrics_module, same_bits

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 2049)
CLASSES = (1, 3, 5)
KINDS = ("distinct", "levels8", "equal", "straddle", "mix")
LABELS = ("mixed", "all1", "all0", "bad")
WEIGHTS = ("unit", "boot", "zeros", "big")                  # "unit" is B = 1 (w == NULL), the others B = 3
SETS = (1, 3, 5, 16)                                        # T: one set of thresholds, a few, and the limit
BINS = (1, 10, 64)
TARGETS = ((0, 1), (1, 1), (9, 10), (999999, 1000000))


@pytest.fixture(scope="module")
def M():
    return metrics_module()


def make_scores(kind, N, C, rng):
    p = rng.random((N, C)).astype(np.float32)
    if kind == "levels8":                                   # long tie groups
        p = (np.floor(p * 8) / 8).astype(np.float32)
    elif kind == "equal":
        p[:] = np.float32(0.3)
    elif kind == "straddle":                                # one tie group from rank 1000 to rank 1050 (or to the end):
        for c in range(C):                                  # it crosses the chunk border 1023 / 1024 where N allows
            o = np.argsort(-p[:, c], kind="stable")
            p[o[1000:1051], c] = p[o[min(1000, N - 1)], c]
    elif kind == "mix":
        p = (np.floor(p * 20) / 20).astype(np.float32)
        sel = rng.random((N, C))
        for lo, v in ((0.00, np.nan), (0.08, np.inf), (0.14, -np.inf), (0.20, -0.0), (0.26, 1.5), (0.30, -0.25),
                      (0.34, np.nextafter(np.float32(1), np.float32(2))), (0.38, 1.0), (0.42, 0.0), (0.46, -1e-45)):
            p[(sel >= lo) & (sel < lo + 0.04)] = v
        p[::5, 0] = -np.nan                                 # another NaN payload: the same key
        if C > 1:
            p[:, C - 1] = np.nan                            # a whole column without a candidate
    return p


def make_labels(kind, N, C, rng):
    if kind == "all0":
        return np.zeros((N, C), np.float32)
    if kind == "all1":
        return np.ones((N, C), np.float32)
    y = (rng.random((N, C)) < 0.35).astype(np.float32)
    if kind == "bad":
        y[rng.random((N, C)) < 0.2] = 0.5
        y[::7, 0] = np.nan
    return y


def make_weights(kind, N, p, y, rng):
    if kind == "unit":
        return None
    if kind == "boot":
        return np.stack([np.bincount(rng.integers(0, N, N), minlength=N) for _ in range(3)]).astype(np.int32)
    if kind == "zeros":
        w = rng.integers(0, 10, (3, N))
        level = np.floor(np.nan_to_num(p[:, 0], nan=0.0, posinf=0.0, neginf=0.0) * 8).astype(np.int64) % 3
        w[0][level == 1] = 0                                # whole tie groups of column 0 without weight, of eight levels the top one
        w[1][(y == 1.0).any(1)] = 0                         # no positive weight
        w[2] = 0                                            # no weight at all
        return w.astype(np.int32)
    w = (rng.random((3, N)) < 10.0 / N).astype(np.int64)    # "big": about ten ones, and four rows near 2^28; sum < 2^30
    w = np.minimum(w, (np.cumsum(w, 1) <= 20).astype(np.int64))
    for b in range(3):
        rows = rng.choice(N, min(4, N), replace=False)
        w[b, rows] = (1 << 28) - np.array([1, 5, 7, 11])[:len(rows)]
    assert (w.sum(1) < (1 << 30)).all()
    return w.astype(np.int32)


def _cases():
    """Every size, C, kind, label set, weight form, T, M and target at least once, in a rotation instead of a product."""
    out = []
    for n, N in enumerate(SIZES * 3):
        out.append((N, CLASSES[(n + n // 9) % 3], KINDS[n % 5], LABELS[(n + n // 4) % 4], WEIGHTS[(n + n // 5) % 4],
                    SETS[n % 4], BINS[(n + n // 3) % 3], TARGETS[n % 4], TARGETS[(n + 1 + n // 4) % 4]))
    out += [(2049, 5, "straddle", "mixed", "boot", 3, 10, (9, 10), (9, 10)), (1025, 3, "straddle", "mixed", "big", 1, 10, (9, 10), (1, 1)),
            (1024, 5, "levels8", "mixed", "zeros", 3, 64, (9, 10), (9, 10)), (2049, 3, "mix", "bad", "big", 16, 10, (1, 1), (0, 1)),
            (1023, 1, "distinct", "mixed", "big", 5, 1, (999999, 1000000), (999999, 1000000))]
    return out


CASES = _cases()


def test_cases_cover_what_they_claim():
    for i, want in enumerate((SIZES, CLASSES, KINDS, LABELS, WEIGHTS, SETS, BINS, TARGETS, TARGETS)):
        assert {c[i] for c in CASES} == set(want), i
    assert any(c[0] > 1050 and c[2] == "straddle" for c in CASES)


@functools.lru_cache(maxsize=None)
def case_data(case):
    N, C, kind, lab, wk, T, nb, sens, spec = case
    rng = np.random.default_rng([N, C, KINDS.index(kind), LABELS.index(lab), WEIGHTS.index(wk), T, nb])
    p, y = make_scores(kind, N, C, rng), make_labels(lab, N, C, rng)
    w = make_weights(wk, N, p, y, rng)
    o, _ = mr.order(p)
    points, totals = opr.operating(p, y, o, w, sens, spec)
    finite = p[np.isfinite(p)]
    pool = np.concatenate([finite[:8], np.array([0.5, 0.0, -0.0, 1.0, np.nan, np.inf, -np.inf, 0.3], np.float32)])
    thr = rng.choice(pool, (T, C)).astype(np.float32)
    return p, y, w, o, (points, totals), thr, opr.confusion(p, y, thr, w), opr.reliability(p, y, w, nb)


def check(M, case, p_d, y_d, w_d, data):
    N, C, kind, lab, wk, T, nb, sens, spec = case
    p, y, w, o, (points, totals), thr, conf, (bins, tot) = data
    got_p, got_t = M.metrics_operating(p_d, y_d, weights=w_d, sensitivity=sens, specificity=spec)
    assert got_p.dtype == torch.int64 and got_t.dtype == torch.int64
    assert np.array_equal(host(got_t), totals)
    assert np.array_equal(host(got_p), points), np.argwhere(host(got_p) != points)[:5]
    got_c = M.metrics_confusion(p_d, y_d, dev(thr), weights=w_d)
    assert got_c.dtype == torch.int64 and np.array_equal(host(got_c), conf)
    got_b, got_tot = M.metrics_reliability(p_d, y_d, n_bins=nb, weights=w_d)
    assert np.array_equal(host(got_b), bins) and np.array_equal(host(got_tot), tot)
    return got_p, got_t


@pytest.mark.parametrize("case", CASES, ids=["N%d-C%d-%s-%s-%s-T%d-M%d-s%d_%d-p%d_%d" % (c[:7] + c[7] + c[8]) for c in CASES])
def test_integers_equal_the_restatement(M, case):
    data = case_data(case)
    p, y, w = data[:3]
    p_d, y_d, w_d = dev(p), dev(y), dev(w)
    got_p, got_t = check(M, case, p_d, y_d, w_d, data)
    # the cut reproduces its counts: the thresholds gathered from the points, fed to metrics_confusion
    res = M.operating_from_points(got_p, got_t, p_d)
    assert np.array_equal(res["threshold"].view(np.int32), opr.thresholds_of(data[4][0], p).view(np.int32))
    thr_d = M._gather_thresholds(got_p, p_d)                # [B, C, 4]
    for b in range(got_p.shape[0]):
        back = host(M.metrics_confusion(p_d, y_d, thr_d[b].t().contiguous(), weights=None if w_d is None else w_d[b:b + 1]))
        pts = data[4][0][b]                                 # [C, 4, 4]
        for u in range(4):
            chosen = pts[:, u, opr.RANK] >= 0
            assert np.array_equal(back[0, u, :, 0][chosen], pts[:, u, opr.TP][chosen])
            assert np.array_equal(back[0, u, :, 1][chosen], pts[:, u, opr.FP][chosen])
        want = opr.confusion(p, y, host(thr_d[b]).T, None if w is None else w[b:b + 1])
        assert np.array_equal(back, want)                   # also where no cut was chosen: the threshold is +inf there


@pytest.mark.parametrize("name", sorted(opr.HAND))
def test_hand_cases(M, name):
    p, y, w, want = opr.hand_case(name)
    points, totals = M.metrics_operating(dev(p), dev(y), weights=dev(w))
    assert np.array_equal(host(points)[0, 0], want)


@pytest.mark.parametrize("t", (0.5, 0.3, 0.0, 1.0))
def test_confusion_at_one_threshold_is_metrics_counts(M, t):
    case = next(c for c in CASES if c[2] == "mix" and c[0] >= 1023 and c[1] > 1)
    p, y, w = case_data(case)[:3]
    p_d, y_d, w_d = dev(p), dev(y), dev(w)
    fields, _ = M.metrics_counts(p_d, y_d, weights=w_d, threshold=t)
    conf = M.metrics_confusion(p_d, y_d, torch.full((1, p.shape[1]), t, device="cuda"), weights=w_d)
    assert torch.equal(conf[:, 0], fields[..., M.TP:M.TN + 1])


def test_side_stream_offset_views_and_refusals(M):
    from ecg_hip import EcgHipError, _lib as L
    case = (1025, 5, "levels8", "mixed", "boot", 3, 10, (9, 10), (9, 10))
    data = case_data(case)
    p, y, w = data[:3]
    N, C = p.shape
    buf = torch.full((N * C + 3,), 7.0, device="cuda")
    p_d = buf[1:1 + N * C].view(N, C)                       # 4-byte offset into a larger buffer
    p_d.copy_(torch.from_numpy(p))
    wbuf = torch.full((w.size + 3,), 9, dtype=torch.int32, device="cuda")
    w_d = wbuf[1:1 + w.size].view(w.shape)
    w_d.copy_(torch.from_numpy(w))
    assert p_d.data_ptr() % 8 == 4 and w_d.data_ptr() % 8 == 4 and p_d.is_contiguous() and w_d.is_contiguous()
    y_d = dev(y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        check(M, case, p_d, y_d, w_d, data)
    side.synchronize()
    assert float(buf[0]) == 7.0 and bool((buf[1 + N * C:] == 7.0).all()) and int(wbuf[0]) == 9 and bool((wbuf[1 + w.size:] == 9).all())
    wide = torch.zeros((N, 2 * C), device="cuda")
    for call in (lambda t: M.metrics_operating(t, y_d), lambda t: M.metrics_confusion(t, y_d, torch.zeros(1, C, device="cuda")),
                 lambda t: M.metrics_reliability(t, y_d)):
        with pytest.raises(EcgHipError, match="contiguous"):
            call(wide[:, ::2])
        with pytest.raises(EcgHipError, match="float32"):
            call(p_d.double())
    with pytest.raises(EcgHipError, match="int32"):
        M.metrics_reliability(p_d, y_d, weights=w_d.long())
    with pytest.raises(EcgHipError, match=r"thresholds must be \[T, C=5\]"):
        M.metrics_confusion(p_d, y_d, torch.zeros(2, 4, device="cuda"))
    with pytest.raises(EcgHipError, match=r"T=17 outside \[1,16\]"):
        M.metrics_confusion(p_d, y_d, torch.zeros(17, C, device="cuda"))
    with pytest.raises(EcgHipError, match=r"M=65 outside \[1,64\]"):
        M.metrics_reliability(p_d, y_d, n_bins=65)
    with pytest.raises(EcgHipError, match="target"):
        M.metrics_operating(p_d, y_d, sensitivity=1.5)
    # int64 outputs off 8 bytes are refused before any launch
    B = w.shape[0]
    off = torch.zeros(2 * B * C * 64 * 4 + 1, dtype=torch.int32, device="cuda")[1:]
    good = torch.zeros(B * C * 64 * 4, dtype=torch.int64, device="cuda")
    ws = torch.empty(N * C * 4 + 64, dtype=torch.uint8, device="cuda")
    order = M.metrics_order(p_d)[0]
    thr = torch.zeros(1, C, device="cuda")
    assert off.data_ptr() % 8 == 4
    for points, totals in ((off, good), (good, off)):
        with pytest.raises(EcgHipError, match="points and totals must be 8-byte aligned"):
            L.call("ecg_metrics_operating", L.ptr(p_d), L.ptr(y_d), L.ptr(order), L.ptr(w_d), points.data_ptr(), totals.data_ptr(),
                   L.ptr(ws), N, C, B, 9, 10, 9, 10, L.stream())
        with pytest.raises(EcgHipError, match="bins and tot must be 8-byte aligned"):
            L.call("ecg_metrics_reliability", L.ptr(p_d), L.ptr(y_d), L.ptr(w_d), points.data_ptr(), totals.data_ptr(), L.ptr(ws),
                   N, C, B, 10, L.stream())
    with pytest.raises(EcgHipError, match="out must be 8-byte aligned"):
        L.call("ecg_metrics_confusion", L.ptr(p_d), L.ptr(y_d), L.ptr(w_d), L.ptr(thr), off.data_ptr(), L.ptr(ws), N, C, B, 1,
               L.stream())
    torch.cuda.synchronize()
    assert int(off.abs().sum()) == 0 and int(good.abs().sum()) == 0


# ---- the user calls
N_BOOT, SEED = 12, 3
RULES = ("f1", "youden", ("sensitivity", 0.9), ("specificity", 0.9))
NAMES = ("f1", "youden", "sensitivity@0.9", "specificity@0.9")


@pytest.fixture(scope="module")
def boot(M):
    rng = np.random.default_rng(21)
    N, C = 300, 5
    p = (np.floor(opr.scores("uniform", N, C, rng, False) * 40) / 40).astype(np.float32)
    y = opr.labels(p, rng)
    p_d, y_d = dev(p), dev(y)
    run = lambda: (M.operating_points(y_d, p_d, rules=RULES, n_boot=N_BOOT, seed=SEED),                      # noqa: E731
                   M.calibration(y_d, p_d, n_bins=10, n_boot=N_BOOT, seed=SEED))
    return p, y, p_d, y_d, run(), run(), host(M.bootstrap_weights(N, N_BOOT, SEED, p_d.device))


def test_bootstrap_row_zero_is_the_point_value_and_a_seed_repeats(M, boot):
    p, y, p_d, y_d, (op_a, cal_a), (op_b, cal_b), w = boot
    op_0, cal_0 = M.operating_points(y_d, p_d, rules=RULES), M.calibration(y_d, p_d, n_bins=10)
    assert list(op_a) == list(NAMES) and "bootstrap" not in op_0["f1"] and "bootstrap" not in cal_0
    for name in NAMES:
        for k in ("threshold", "f1", "sensitivity", "specificity", "youden"):
            assert same_bits(op_a[name][k], op_0[name][k]) and same_bits(op_a[name]["replicates"][k], op_b[name]["replicates"][k])
            assert op_a[name]["replicates"][k].shape == (N_BOOT, 5)
            lo, hi = op_a[name]["bootstrap"][k]["lo"], op_a[name]["bootstrap"][k]["hi"]
            assert same_bits(lo, op_b[name]["bootstrap"][k]["lo"]) and (lo <= hi).all()
        assert np.array_equal(op_a[name]["tp"], op_0[name]["tp"]) and np.array_equal(op_a[name]["row"], op_0[name]["row"])
    for k in ("ece", "mce", "brier", "ece_macro", "mce_macro", "brier_macro", "frac_pos", "mean_prob"):
        assert same_bits(cal_a[k], cal_0[k]) and same_bits(cal_a["replicates"][k], cal_b["replicates"][k])
        assert same_bits(cal_a["bootstrap"][k]["hi"], cal_b["bootstrap"][k]["hi"])
    assert cal_a["ece"].shape == (5,) and cal_a["frac_pos"].shape == (5, 10) and cal_a["replicates"]["ece"].shape == (N_BOOT, 5)
    assert np.array_equal(cal_a["n"], cal_0["n"]) and cal_a["n"].sum() == 5 * 300


def test_bootstrap_replicates_are_the_restatement_on_the_drawn_rows(M, boot):
    p, y, _, _, (op_a, cal_a), _, w = boot
    C = p.shape[1]
    o, _ = mr.order(p)
    for c in range(C):                                      # the precondition under which weights and drawn rows choose alike:
        top = p[:, c] == p[:, c].max()                      # the highest tie group keeps some weight in every replicate
        assert (w[:, top].sum(1) > 0).all()
    for b in range(1, N_BOOT + 1):
        idx = opr.expand(w[b])
        pp, yy = p[idx], y[idx]
        oo, _ = mr.order(pp)
        points, totals = opr.operating(pp, yy, oo, None, (9, 10), (9, 10))
        thr = opr.thresholds_of(points, pp)
        for u, name in enumerate(NAMES):
            assert np.array_equal(op_a[name]["replicates"]["threshold"][b - 1].astype(np.float32), thr[0, :, u])
            for c in range(C):
                exact = opr.values_exact(points[0, c, u], int(totals[0, c, 0]), int(totals[0, c, 1]))
                for k, f in zip(("f1", "sensitivity", "specificity", "youden"), exact):
                    assert same_bits(op_a[name]["replicates"][k][b - 1, c], opr.as_double(f)), (b, name, c, k)
        want = M.calibration_from_tables(*opr.reliability(pp, yy, None, 10))
        for k in ("ece", "mce", "brier", "ece_macro", "frac_pos", "mean_prob"):
            assert same_bits(cal_a["replicates"][k][b - 1], want[k][0]), (b, k)


def test_a_float_threshold_keeps_its_bits_and_a_vector_goes_through_confusion(M, boot, monkeypatch):
    p, y, p_d, y_d = boot[:4]
    C = p.shape[1]
    from ecg_hip import _lib as L
    seen = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: seen.append(name) or real(name, *a))
    scalar = M.compute_metrics_device(y_d, p_d, 0.5)
    assert seen == ["ecg_metrics_order", "ecg_metrics_counts"]        # today's calls
    direct = M.summarize(*M._one_read(*M.metrics_counts(p_d, y_d, threshold=0.5)))
    for k, v in scalar.items():
        assert same_bits(v, direct[k][0])
    del seen[:]
    vector = M.compute_metrics_device(y_d, p_d, [0.5] * C)
    assert seen == ["ecg_metrics_order", "ecg_metrics_counts", "ecg_metrics_confusion"]
    assert set(vector) == set(scalar) and all(same_bits(vector[k], scalar[k]) for k in scalar)
    bs = M.bootstrap_metrics(y_d, p_d, n_boot=N_BOOT, seed=SEED, threshold=0.5)
    bv = M.bootstrap_metrics(y_d, p_d, n_boot=N_BOOT, seed=SEED, threshold=torch.full((C,), 0.5, device="cuda"))
    for k in M.MACRO_KEYS + ("f1_per_class",):
        assert same_bits(bs["replicates"][k], bv["replicates"][k]) and same_bits(bs[k]["point"], bv[k]["point"])
        assert same_bits(bs[k]["lo"], bv[k]["lo"]) and same_bits(bs[k]["hi"], bv[k]["hi"])
    # per-class thresholds: F1 is the F1 at those, the other two keys do not move
    thr = M.select_thresholds(y_d, p_d, "f1")
    assert thr.dtype == torch.float32 and thr.is_cuda and tuple(thr.shape) == (C,)
    tuned = M.compute_metrics_device(y_d, p_d, thr)
    o, _ = mr.order(p)
    points, totals = opr.operating(p, y, o, None, (9, 10), (9, 10))
    assert np.array_equal(host(thr), opr.thresholds_of(points, p)[0, :, opr.F1])
    want = [opr.as_double(opr.values_exact(points[0, c, opr.F1], *map(int, totals[0, c]))[0]) for c in range(C)]
    assert same_bits(tuned["f1_per_class"], want) and same_bits(tuned["auroc_macro"], scalar["auroc_macro"])
    assert same_bits(tuned["auprc_macro"], scalar["auprc_macro"]) and tuned["f1_macro"] >= scalar["f1_macro"]
    with pytest.raises(L.EcgHipError, match="one value per class"):
        M.compute_metrics_device(y_d, p_d, [0.5] * (C + 1))


@pytest.mark.parametrize("rule,u", (("f1", opr.F1), ("youden", opr.YOUDEN), (("sensitivity", 0.8), opr.SENS), (("specificity", 0.75), opr.SPEC)),
                         ids=("f1", "youden", "sensitivity", "specificity"))
def test_tuned_metrics_on_a_two_fold_split(M, rule, u):
    rng = np.random.default_rng(8)
    N, C = 700, 5
    p = (np.floor(opr.scores("logistic", N, C, rng, False) * 200) / 200).astype(np.float32)
    y = opr.labels(p, rng)
    fold = rng.random(N) < 0.4
    (pa, ya), (pb, yb) = (p[fold], y[fold]), (p[~fold], y[~fold])
    got = M.tuned_metrics(dev(ya), dev(pa), dev(yb), dev(pb), rule=rule, n_boot=N_BOOT, seed=SEED)
    oa, _ = mr.order(pa)
    points, _ = opr.operating(pa, ya, oa, None, (4, 5), (3, 4))
    thr = opr.thresholds_of(points, pa)[0, :, u]            # chosen on fold A by the restatement
    assert np.array_equal(got["thresholds"].view(np.int32), thr.view(np.int32))
    w = host(M.bootstrap_weights(len(pb), N_BOOT, SEED, torch.device("cuda")))
    for b in range(N_BOOT + 1):                             # applied by numpy on fold B, and on its drawn rows
        idx = opr.expand(w[b])
        pred, pos = pb[idx] >= thr[None, :], yb[idx] == 1.0
        tp, fp, fn, tn = ((m.sum(0)) for m in (pred & pos, pred & ~pos, ~pred & pos, ~pred & ~pos))
        if b == 0:
            assert np.array_equal(got["confusion"], np.stack([tp, fp, fn, tn], 1))
        f1 = [opr.as_double(Fraction(int(2 * a), int(2 * a + b_ + c_))) if 2 * a + b_ + c_ else 0.0 for a, b_, c_ in zip(tp, fp, fn)]
        sens = [opr.as_double(Fraction(int(a), int(a + c_))) if a + c_ else np.nan for a, c_ in zip(tp, fn)]
        spec = [opr.as_double(Fraction(int(d), int(d + b_))) if d + b_ else np.nan for d, b_ in zip(tn, fp)]
        for k, want in (("f1", f1), ("sensitivity", sens), ("specificity", spec)):
            per, macro = (got[k + "_per_class"], got[k + "_macro"]) if b == 0 else \
                (got["replicates"][k + "_per_class"][b - 1], got["replicates"][k + "_macro"][b - 1])
            assert same_bits(per, want) and same_bits(macro, np.mean(want)), (b, k)


def test_calibrate_predictions_tool_on_merged_csvs(M, tmp_path):
    import csv
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import calibrate_predictions as tool
    finally:
        sys.path.pop(0)
    labels = ["CD", "HYP", "MI", "NORM", "STTC"]
    rng = np.random.default_rng(65)
    folds = {}
    for fold, N in (("val", 90), ("test", 65)):
        base = (np.floor(opr.scores("uniform", N, 5, rng, False) * 30) / 30).astype(np.float32)
        y = opr.labels(base, rng)
        mm = np.clip(base + (rng.random((N, 5)) - 0.4).astype(np.float32) * np.float32(0.3), 0, 1).astype(np.float32)
        folds[fold] = (y, base, mm)
        with open(tmp_path / f"{fold}.csv", "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow([f"y_true_{s}" for s in labels] + [f"y_prob_{s}" for s in labels] + [f"y_prob_{s}_mm" for s in labels] +
                        (["y_true_AF", "y_prob_AF"] if fold == "test" else []))
            for i in range(N):
                wr.writerow([repr(float(v)) for v in np.concatenate([y[i], base[i], mm[i]])] +
                            ([repr(float(y[i, 0])), repr(float(base[i, 2]))] if fold == "test" else []))
    alone = tool.calibrate_csv(str(tmp_path / "test.csv"), n_boot=5, seed=2)
    assert [d["model"] for d in alone] == ["baseline", "multimodal", "af"] and all("tuned" not in d for d in alone)
    assert alone[2]["labels"] == ["AF"] and alone[0]["rows"] == 65 and alone[0]["thresholds_chosen_on"] == "test"
    y, base, mm = folds["test"]
    for d, p in zip(alone, (base, mm)):
        cal = M.calibration_from_tables(*opr.reliability(p, y, None, 10))
        o, _ = mr.order(p)
        points, totals = opr.operating(p, y, o, None, (9, 10), (9, 10))
        assert same_bits(d["calibration"]["ece"], cal["ece"][0]) and same_bits(d["calibration"]["brier_macro"], cal["brier_macro"][0])
        assert d["calibration"]["n"] == cal["n"][0].tolist() and same_bits(d["calibration"]["frac_pos"], cal["frac_pos"][0])
        assert list(d["thresholds"]) == list(NAMES) and set(d["calibration"]["bootstrap"]["ece"]) == {"lo", "hi"}
        for u, name in enumerate(NAMES):
            assert np.array_equal(np.array(d["thresholds"][name]["threshold"], np.float32), opr.thresholds_of(points, p)[0, :, u])
    json.dumps(alone)
    with pytest.raises(ValueError, match="no columns for the model 'af'"):
        tool.calibrate_csv(str(tmp_path / "test.csv"), val=str(tmp_path / "val.csv"))
    with open(tmp_path / "test.csv") as f:                  # the same file without the AF columns
        rows = [line.rstrip("\n").split(",")[:15] for line in f]
    with open(tmp_path / "test5.csv", "w") as f:
        f.write("\n".join(",".join(r) for r in rows) + "\n")
    both = tool.calibrate_csv(str(tmp_path / "test5.csv"), val=str(tmp_path / "val.csv"))
    yv, pv, _ = folds["val"]
    want = M.tuned_metrics(dev(yv), dev(pv), dev(y), dev(base), rule="youden")
    assert both[0]["thresholds_chosen_on"] == "val" and list(both[0]["tuned"]) == list(NAMES)
    assert same_bits(both[0]["tuned"]["youden"]["f1_per_class"], want["f1_per_class"])
    assert both[0]["tuned"]["youden"]["confusion"] == want["confusion"].tolist()
