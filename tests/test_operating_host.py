"""Host checks of the operating points and the calibration table.  (1) The restatement (tests/operating_ref.py) that the GPU
tests compare with == gives the hand cases written out there.  (2) It is held to scikit-learn: the best F1 is the maximum
over precision_recall_curve, the best J the maximum of tpr - fpr over roc_curve, and f1_score at the returned threshold
reproduces the former, each within 1e-12.  (3) The reliability table is sklearn.calibration.calibration_curve's on inputs
with no score on a bin edge (asserted, none left out), and the Brier score is brier_score_loss within the quantisation.
(4) calibration_from_tables and operating_from_points give the bits of the same ratios taken in Fractions.  (5) The entry
points refuse every size outside their limits before any launch, asked with NULL pointers."""
import ctypes
import warnings
from fractions import Fraction

import numpy as np
import pytest

import metrics_ref as mr
import operating_ref as opr
from metrics_util import load_lib, same_bits

NINE_TENTHS = (9, 10)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.mark.parametrize("name", sorted(opr.HAND))
def test_hand_cases(name):
    p, y, w, want = opr.hand_case(name)
    o, _ = mr.order(p)
    points, totals = opr.operating(p, y, o, w, NINE_TENTHS, NINE_TENTHS)
    assert points.shape == (1, 1, 4, 4) and np.array_equal(points[0, 0], want), (points[0, 0], want)
    ww = np.ones(len(p), np.int64) if w is None else w[0]
    assert totals[0, 0, 0] == ww[y[:, 0] == 1].sum() and totals[0, 0, 1] == ww[y[:, 0] == 0].sum()
    # the cut reproduces its counts
    thr = opr.thresholds_of(points, p)[0]                   # [C = 1, 4]
    conf = opr.confusion(p, y, thr.T, w)                    # [1, T = 4, 1, 4]
    for u in range(4):
        if want[u, 0] >= 0:
            assert conf[0, u, 0, 0] == want[u, 2] and conf[0, u, 0, 1] == want[u, 3]
        else:
            assert thr[0, u] == np.inf and conf[0, u, 0, 0] == 0 and conf[0, u, 0, 1] == 0


SK_CASES = [(kind, N, ties) for kind in ("uniform", "logistic") for N in (5, 64, 300, 2000) for ties in (False, True)]


@pytest.mark.parametrize("kind,N,ties", SK_CASES, ids=["%s-N%d-ties%d" % c for c in SK_CASES])
def test_restatement_matches_sklearn(kind, N, ties):
    from sklearn import metrics as skm
    rng = np.random.default_rng([sum(map(ord, kind)), N, int(ties)])
    C = 2
    p = opr.scores(kind, N, C, rng, ties)
    y = opr.labels(p, rng)
    o, _ = mr.order(p)
    points, totals = opr.operating(p, y, o, None, NINE_TENTHS, NINE_TENTHS)
    thr = opr.thresholds_of(points, p)
    for c in range(C):
        P, Q = (int(v) for v in totals[0, c])
        f1, _, _, _ = opr.values_exact(points[0, c, opr.F1], P, Q)
        _, _, _, j = opr.values_exact(points[0, c, opr.YOUDEN], P, Q)
        prec, rec, _ = skm.precision_recall_curve(y[:, c], p[:, c])
        with np.errstate(divide="ignore", invalid="ignore"):
            f1_curve = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
        assert abs(float(f1) - f1_curve.max()) <= 1e-12
        fpr, tpr, _ = skm.roc_curve(y[:, c], p[:, c], drop_intermediate=False)
        assert abs(float(j) - (tpr - fpr).max()) <= 1e-12
        hard = (p[:, c] >= thr[0, c, opr.F1]).astype(int)
        assert abs(skm.f1_score(y[:, c], hard, zero_division=0) - float(f1)) <= 1e-12
        # the target rules, by their definition on the curve
        ok = tpr >= 0.9 - 1e-12
        assert points[0, c, opr.SENS, opr.FP] == round(fpr[ok].min() * Q)
        ok = fpr <= 0.1 + 1e-12
        assert points[0, c, opr.SPEC, opr.TP] == round(tpr[ok].max() * P)


def _grid():
    return ((np.arange(1000) + 0.5) / 1000).astype(np.float32)[:, None]


def _calibration_inputs():
    out = []
    for kind in ("uniform", "logistic"):
        for N in (50, 1000, 20000):
            rng = np.random.default_rng([sum(map(ord, kind)), N, 7])
            p = opr.scores(kind, N, 1, rng, False)
            for M in (8, 10, 15, 16):
                out.append((f"{kind}-N{N}-M{M}", p, opr.labels(p, rng), M))
    rng = np.random.default_rng(77)
    p = _grid()
    y = opr.labels(p, rng)
    return out + [(f"grid-M{M}", p, y, M) for M in (8, 10, 15)]


CAL = _calibration_inputs()


@pytest.mark.parametrize("name,p,y,M", CAL, ids=[c[0] for c in CAL])
def test_table_matches_sklearn_calibration_curve(name, p, y, M):
    from sklearn.calibration import calibration_curve
    from sklearn.metrics import brier_score_loss
    from ecg_hip import metrics as Mx
    assert not opr.on_bin_edge(p, M).any()                  # (lo, hi] on p and [lo, hi) on q agree only off the edges
    N = len(p)
    bins, tot = opr.reliability(p, y, None, M)
    cal = Mx.calibration_from_tables(bins, tot)
    frac, mean = calibration_curve(y[:, 0].astype(int), p[:, 0].astype(np.float64), n_bins=M, strategy="uniform")
    filled = cal["n"][0, 0] > 0
    assert filled.sum() == len(frac) and cal["n"][0, 0].sum() == N and tot[0, 0, 2] == 0 and tot[0, 0, 3] == 0
    assert np.array_equal(cal["frac_pos"][0, 0][filled], frac)
    assert np.abs(cal["mean_prob"][0, 0][filled] - mean).max() <= 2.0 ** -24
    brier = brier_score_loss(y[:, 0].astype(int), p[:, 0].astype(np.float64))
    assert abs(cal["brier"][0, 0] - brier) <= 2.0 ** -23 + N * 2.0 ** -52


def test_the_two_bin_conventions_differ_on_an_edge():
    """The grid (k + 0.5) / 1000 with 16 bins is the counter-example: 0.0625 = 62.5 / 1000 is a score AND an inner edge
    (1/16).  scikit-learn's bins are (lo, hi], so it counts that row in bin 0; the table's bins are [lo, hi) on q, so it
    counts it in bin 1.  Neither is wrong; they are two conventions, and the comparison above holds off the edges only."""
    from sklearn.calibration import calibration_curve
    p = _grid()
    M = 16
    edge = opr.on_bin_edge(p, M)[:, 0]
    assert edge.any() and p[62, 0] == np.float32(0.0625) and edge[62]
    y = np.zeros_like(p)
    y[62] = 1.0                                             # the one positive sits on the edge
    bins, tot = opr.reliability(p, y, None, M)
    frac, _ = calibration_curve(y[:, 0].astype(int), p[:, 0].astype(np.float64), n_bins=M, strategy="uniform")
    assert bins[0, 0, 0, 1] == 0 and bins[0, 0, 1, 1] == 1  # ours: bin 1
    assert frac[0] > 0 and frac[1] == 0                     # scikit-learn's: bin 0


def test_from_tables_and_from_points_are_the_exact_ratios():
    from ecg_hip import metrics as Mx
    rng = np.random.default_rng(3)
    N, C, M = 400, 3, 10
    p = opr.scores("logistic", N, C, rng, True)
    y = opr.labels(p, rng)
    y[:, 2] = 0.5                                           # a class without any valid row: W == 0
    p[5, 0], p[6, 0], p[7, 1] = 1.5, np.nan, -0.25          # OUT
    big = np.zeros(N, np.int64)
    big[:4] = (1 << 28) - 3                                 # numerators beyond 2^53: the Python-integer route
    w = np.stack([np.ones(N, np.int64), np.bincount(rng.integers(0, N, N), minlength=N), big, np.zeros(N, np.int64)])
    bins, tot = opr.reliability(p, y, w, M)
    assert tot[0, 0, 2] == 2 and tot[0, 1, 2] == 1 and tot[0, 2, 3] == N
    cal = Mx.calibration_from_tables(bins, tot)
    for b in range(len(w)):
        defined = []
        for c in range(C):
            ece, mce, brier, frac, mean = opr.calibration_exact(bins[b, c], tot[b, c])
            assert same_bits(cal["ece"][b, c], opr.as_double(ece)) and same_bits(cal["mce"][b, c], opr.as_double(mce))
            assert same_bits(cal["brier"][b, c], opr.as_double(brier))
            assert same_bits(cal["frac_pos"][b, c], [opr.as_double(f) for f in frac])
            assert same_bits(cal["mean_prob"][b, c], [opr.as_double(f) for f in mean])
            if ece is not None:
                defined.append(c)
        for k in ("ece", "mce", "brier"):
            want = np.mean([cal[k][b, c] for c in defined]) if defined else np.nan
            assert same_bits(cal[k + "_macro"][b], want)
    assert np.isnan(cal["ece"][:, 2]).all() and np.isnan(cal["ece_macro"][3])
    # the operating points' values
    o, _ = mr.order(p)
    points, totals = opr.operating(p, y, o, w, NINE_TENTHS, (1, 2))
    got = Mx.operating_from_points(points, totals, p)
    assert np.array_equal(got["threshold"].view(np.int32), opr.thresholds_of(points, p).view(np.int32))
    assert np.array_equal(got["tp"], points[..., opr.TP]) and np.array_equal(got["rank"], points[..., opr.RANK])
    for b in range(len(w)):
        for c in range(C):
            for u in range(4):
                exact = opr.values_exact(points[b, c, u], int(totals[b, c, 0]), int(totals[b, c, 1]))
                for k, f in zip(("f1", "sensitivity", "specificity", "youden"), exact):
                    assert same_bits(got[k][b, c, u], opr.as_double(f)), (b, c, u, k)


def test_targets_are_fractions_of_their_decimal_text():
    from ecg_hip import EcgHipError
    from ecg_hip import metrics as Mx
    assert Mx._target("t", "sensitivity", 0.9) == (9, 10) and Mx._target("t", "sensitivity", 0.999999) == (999999, 1000000)
    assert Mx._target("t", "specificity", 1) == (1, 1) and Mx._target("t", "specificity", 0.0) == (0, 1)
    assert Mx._target("t", "specificity", (3, 4)) == (3, 4) and Mx._target("t", "specificity", Fraction(2, 3)) == (2, 3)
    for bad in (0.9999999, 1.5, -0.1, (3, 2), (1, 2000000), "x"):
        with pytest.raises(EcgHipError, match="target"):
            Mx._target("t", "sensitivity", bad)


def test_limits_are_refused_before_any_launch(lib):
    err = lambda: lib.ecg_last_error().decode()                                 # noqa: E731
    nul = ctypes.c_void_p(None)
    op = lambda N, C, B, sn=9, sd=10, pn=9, pd=10: lib.ecg_metrics_operating(nul, nul, nul, nul, nul, nul, nul, N, C, B, sn, sd, pn, pd, nul)  # noqa: E731
    cf = lambda N, C, B, T: lib.ecg_metrics_confusion(nul, nul, nul, nul, nul, nul, N, C, B, T, nul)        # noqa: E731
    rl = lambda N, C, B, M: lib.ecg_metrics_reliability(nul, nul, nul, nul, nul, nul, N, C, B, M, nul)      # noqa: E731
    calls = (("metrics_operating", lambda N, C, B: op(N, C, B), lambda N, C, B: lib.ecg_metrics_operating_workspace_bytes(N, C, B)),
             ("metrics_confusion", lambda N, C, B: cf(N, C, B, 1), lambda N, C, B: lib.ecg_metrics_confusion_workspace_bytes(N, C, B, 1)),
             ("metrics_reliability", lambda N, C, B: rl(N, C, B, 10), lambda N, C, B: lib.ecg_metrics_reliability_workspace_bytes(N, C, B, 10)))
    for who, call, ws in calls:
        for N in (0, -1, 65537):
            assert call(N, 5, 1) == 1 and f"{who}: N={N} outside [1,65536]" in err() and ws(N, 5, 1) == 0
        for C in (0, 65):
            assert call(10, C, 1) == 1 and f"{who}: C={C} outside [1,64]" in err() and ws(10, C, 1) == 0
        for B in (0, 65537):
            assert call(10, 5, B) == 1 and f"{who}: B={B} outside [1,65536]" in err() and ws(10, 5, B) == 0
        assert call(10, 5, 2) == 1 and "B=2 weight rows need w" in err()
        assert call(65536, 64, 1) == 1 and f"{who}: null pointer" in err()      # inside the limits: the pointers are next
        assert ws(65536, 64, 65536) >= 65536 * 64 * 4
    for T in (0, 17):
        assert cf(10, 5, 1, T) == 1 and f"metrics_confusion: T={T} outside [1,16]" in err()
        assert lib.ecg_metrics_confusion_workspace_bytes(10, 5, 1, T) == 0
    for M in (0, 65):
        assert rl(10, 5, 1, M) == 1 and f"metrics_reliability: M={M} outside [1,64]" in err()
        assert lib.ecg_metrics_reliability_workspace_bytes(10, 5, 1, M) == 0
    assert cf(10, 5, 1, 16) == 1 and "null pointer" in err() and rl(10, 5, 1, 64) == 1 and "null pointer" in err()
    for num, den in ((11, 10), (1, 1000001), (-1, 10), (0, 0)):                 # num > den, den > 10^6, negative, no denominator
        assert op(10, 5, 1, num, den) == 1 and f"metrics_operating: sensitivity {num}/{den}" in err()
        assert op(10, 5, 1, 9, 10, num, den) == 1 and f"metrics_operating: specificity {num}/{den}" in err()
    for num, den in ((0, 1), (1, 1), (999999, 1000000), (1000000, 1000000)):
        assert op(10, 5, 1, num, den, num, den) == 1 and "null pointer" in err()
    # misaligned bases: 8 bytes for the int64 outputs, 4 otherwise (addresses only; nothing is launched on a refusal)
    a = lambda v: ctypes.c_void_p(v)                                            # noqa: E731
    assert lib.ecg_metrics_operating(a(64), a(64), a(64), nul, a(68), a(64), a(64), 10, 5, 1, 9, 10, 9, 10, nul) == 1
    assert "points and totals must be 8-byte aligned" in err()
    assert lib.ecg_metrics_operating(a(64), a(64), a(64), nul, a(64), a(68), a(64), 10, 5, 1, 9, 10, 9, 10, nul) == 1
    assert "points and totals must be 8-byte aligned" in err()
    assert lib.ecg_metrics_operating(a(64), a(66), a(64), nul, a(64), a(64), a(64), 10, 5, 1, 9, 10, 9, 10, nul) == 1
    assert "not 4-byte aligned" in err()
    assert lib.ecg_metrics_confusion(a(64), a(64), nul, a(64), a(68), a(64), 10, 5, 1, 1, nul) == 1 and "out must be 8-byte aligned" in err()
    assert lib.ecg_metrics_confusion(a(64), a(64), nul, a(66), a(64), a(64), 10, 5, 1, 1, nul) == 1 and "not 4-byte aligned" in err()
    assert lib.ecg_metrics_reliability(a(64), a(64), nul, a(64), a(68), a(64), 10, 5, 1, 10, nul) == 1
    assert "bins and tot must be 8-byte aligned" in err()
    assert lib.ecg_metrics_reliability(a(66), a(64), nul, a(64), a(64), a(64), 10, 5, 1, 10, nul) == 1 and "not 4-byte aligned" in err()


def test_wrappers_refuse_cpu_tensors_and_are_reachable_from_functional():
    import torch
    from ecg_hip import EcgHipError, functional as F
    from ecg_hip import metrics as Mx
    import src.training.metrics as T
    for name in ("metrics_operating", "metrics_confusion", "metrics_reliability", "calibration_from_tables", "operating_from_points",
                 "calibration", "operating_points", "select_thresholds", "tuned_metrics"):
        assert getattr(F, name) is getattr(Mx, name)
    assert T.select_thresholds is Mx.select_thresholds and T.calibration is Mx.calibration and T.tuned_metrics is Mx.tuned_metrics
    z = torch.zeros(4, 2)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        F.metrics_operating(z, z)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        F.metrics_confusion(z, z, torch.zeros(1, 2))
    with pytest.raises(EcgHipError, match="CPU tensor"):
        F.metrics_reliability(z, z)
    for call in (lambda: Mx.calibration(z, z), lambda: Mx.operating_points(z, z), lambda: Mx.select_thresholds(z, z),
                 lambda: Mx.tuned_metrics(z, z, z, z)):
        with pytest.raises(EcgHipError, match="CUDA tensors"):
            call()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Mx.calibration_from_tables(np.zeros((2, 3, 4, 3), np.int64), np.zeros((2, 3, 4), np.int64))   # nothing but NaN, quietly
