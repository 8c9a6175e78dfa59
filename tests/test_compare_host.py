"""Host checks of the paired comparison.  (1) The restatement (tests/compare_ref.py) that the GPU tests compare with == is
held to cases worked by hand, to the identity sum_pos a == sum_neg b == U2 of the other restatement, and to DeLong's
covariance in its classic form (fp64 midranks, np.cov), written here and sharing nothing with it.  (2) The package's
delong_from_sums and mcnemar_from_sums give, bit for bit, what the restatement's exact rationals give.  (3) The new entry
points refuse every size outside their limits before any launch, asked with NULL pointers."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import compare_ref as cr
import metrics_ref as mr
from metrics_util import load_lib, same_bits

from ecg_hip.metrics import delong_from_sums, mcnemar_from_sums      # absent before this stage existed

F = Fraction


# scores of model A, of model B, labels; then by hand: the placements of A and B, U2 of each, Cov[A,A], Cov[B,B], Cov[A,B]
# and var = Cov[A,A] + Cov[B,B] - 2 Cov[A,B].
#   N = 4, ties, m = n = 2, every term over 4 n^2 m^2 (m-1) = 64:
#     A: a_0 = 2*2 = 4, a_1 = 2*1 + 1 (row 2 ties) = 3; b_2 = 2*1 + 1 = 3, b_3 = 2*2 = 4.       U2 = 7
#     B: a_0 = 2 (only row 2 is below 0.6), a_1 = 4; b_2 = 4, b_3 = 2 (only row 1 is above 0.65).    U2 = 6
#     SPOS: AA 16+9 = 25, BB 4+16 = 20, AB 8+12 = 20; SNEG the same three numbers.
#     Cov AA = (50-49)/64 + (50-49)/64 = 1/32;  BB = 2 (40-36)/64 = 1/8;  AB = 2 (40-42)/64 = -1/16;  var = 9/32
#   N = 6, ties, m = n = 3, every term over 4*9*9*2 = 648:
#     A: a = 6 (row 0), 2*1 + 2 = 4 (row 2), 0 + 1 = 1 (row 4); b = 2*1 + 1 = 3 (rows 1, 3), 2*2 + 1 = 5 (row 5).      U2 = 11
#     B: a = 2*1 + 1 = 3 (rows 0, 4), 6 (row 2); b = 2*1 + 2 = 4 (row 1), 6 (row 3), 2 (row 5).                        U2 = 12
#     SPOS: AA 53, BB 54, AB 18+24+3 = 45; SNEG: AA 43, BB 56, AB 12+18+10 = 40.
#     Cov AA = (159-121 + 129-121)/648 = 23/324;  BB = (162-144 + 168-144)/648 = 7/108;  AB = (135-132 + 120-132)/648 = -1/72
#     var = 23/324 + 21/324 + 9/324 = 53/324
#   N = 6, no ties, m = n = 3:
#     A: a = 4, 6, 6 (rows 2, 4, 5); b = 6, 6, 4 (rows 0, 1, 3).    B: a = 4, 6, 6; b = 4, 6, 6.      U2 = 16 and 16
#     SPOS: 88, 88, 88; SNEG: AA 88, BB 88, AB 24+36+24 = 84.
#     Cov AA = BB = 2 (264-256)/648 = 2/81;  AB = (264-256 + 252-256)/648 = 1/162;  var = 4/81 - 1/81 = 1/27;  z = 0, p = 1
HAND = {
    "n4_ties": ([0.8, 0.5, 0.5, 0.2], [0.6, 0.7, 0.1, 0.65], [1, 1, 0, 0],
                [4, 3, 3, 4], [2, 4, 4, 2], 7, 6, F(1, 32), F(1, 8), F(-1, 16), F(9, 32)),
    "n6_ties": ([0.9, 0.7, 0.7, 0.7, 0.4, 0.4], [0.3, 0.3, 0.8, 0.1, 0.3, 0.5], [1, 0, 1, 0, 1, 0],
                [6, 3, 4, 3, 1, 5], [3, 4, 6, 6, 3, 2], 11, 12, F(23, 324), F(7, 108), F(-1, 72), F(53, 324)),
    "n6_untied": ([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [0.35, 0.15, 0.25, 0.05, 0.65, 0.45], [0, 0, 1, 0, 1, 1],
                  [6, 6, 4, 4, 6, 6], [4, 6, 4, 6, 6, 6], 16, 16, F(2, 81), F(2, 81), F(1, 162), F(1, 27)),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_cases_worked_by_hand(name):
    a, b, y, pa, pb, ua, ub, caa, cbb, cab, var = HAND[name]
    probs = np.array([a, b], np.float32)[:, :, None]
    y = np.array(y, np.float32)[:, None]
    place, single, pair, dl, mc = cr.compare(y, probs)
    assert place[0, 0].tolist() == pa and place[1, 0].tolist() == pb
    assert single[0, :, 0].tolist() == [ua, ub]
    theta, cov, v = cr.delong_exact(single, pair)
    m = n = len(a) // 2
    assert theta[0] == [F(ua, 2 * m * n), F(ub, 2 * m * n)]
    assert (cov[0][0][0], cov[0][1][1], cov[0][0][1], cov[0][1][0]) == (caa, cbb, cab, cab)
    assert v[0][0][1] == v[0][1][0] == var and v[0][0][0] == 0
    z = (ua / (2 * m * n) - ub / (2 * m * n)) / math.sqrt(float(var))
    assert same_bits(dl["z"][0, 0, 1], z) and same_bits(dl["p"][0, 0, 1], math.erfc(abs(z) / math.sqrt(2.0)))
    back = (ub / (2 * m * n) - ua / (2 * m * n)) / math.sqrt(float(var))
    assert same_bits(dl["z"][0, 1, 0], back) and np.isnan(dl["z"][0, 0, 0]) and np.isnan(dl["p"][0, 1, 1])
    got = delong_from_sums(single, pair)
    assert all(same_bits(got[k], dl[k]) for k in dl)


def test_mcnemar_by_hand():
    pair = np.zeros((1, 1, 4, 6), np.int64)
    pair[0, 0, 0, 2:4] = (0, 0)                             # no disagreement: 1
    pair[0, 0, 1, 2:4] = (3, 1)                             # 2 (C(4,0) + C(4,1)) / 16 = 10/16
    pair[0, 0, 2, 2:4] = (2, 2)                             # 2 (1 + 4 + 6) / 16 > 1: 1
    pair[0, 0, 3, 2:4] = (0, 10)                            # 2 / 1024
    want = [1.0, 0.625, 1.0, 2.0 / 1024]
    assert cr.mcnemar(pair)[0, 0].tolist() == want and mcnemar_from_sums(pair)[0, 0].tolist() == want
    # every small (b, c) and some large ones, far in the tail and near the centre: the package's two routes to the doubled
    # tail against the sum of math.comb terms
    bc = [(b, c) for b in range(13) for c in range(13)] + [(40, 3), (3, 40), (300, 10), (500, 480), (480, 500), (301, 300),
                                                           (400, 400), (560, 640)]
    pair = np.zeros((1, 1, len(bc), 6), np.int64)
    pair[0, 0, :, 2:4] = bc
    assert same_bits(mcnemar_from_sums(pair), cr.mcnemar(pair))


CASES = [(kind, lab, N, rel) for kind in cr.KINDS for lab, N, rel in (("mixed", 67, "independent"), ("mixed", 130, "one_row"))] + \
        [("untied", "all0", 40, "independent"), ("q3", "all1", 40, "same"), ("untied", "mixed", 2, "independent"),
         ("q3", "mixed", 1, "same"), ("q3", "mixed", 1030, "monotone")]


def _data(kind, lab, N, rel, C=3):
    rng = np.random.default_rng([cr.KINDS.index(kind), cr.LABELS.index(lab), N, cr.RELATIONS.index(rel)])
    a, y = cr.scores(kind, N, C, rng), cr.labels(lab, N, C, rng)
    return y, np.stack([a, cr.related(rel, a, kind, rng), cr.scores(kind, N, C, rng)])


@pytest.mark.parametrize("kind,lab,N,rel", CASES, ids=["%s-%s-N%d-%s" % c for c in CASES])
def test_identity_and_package_equals_the_exact_rationals(kind, lab, N, rel):
    y, probs = _data(kind, lab, N, rel)
    place, single, pair, dl, mc = cr.compare(y, probs, 0.3)
    for k, p in enumerate(probs):
        fields, _, _ = mr.counts(p, y, mr.order(p)[0], None, 0.3, 64)
        for c in range(y.shape[1]):
            pos, neg = y[:, c] == 1.0, y[:, c] == 0.0
            assert place[k, c][pos].sum() == place[k, c][neg].sum() == fields[0, c, mr.U2] == single[c, k, 0]
            assert (place[k, c][~pos & ~neg] == -1).all() and (place[k, c][pos | neg] >= 0).all()
            assert (single[c, k, 1], single[c, k, 2]) == (fields[0, c, mr.POS], fields[0, c, mr.NEG])
            # right and wrong at the threshold are the confusion counts of the other restatement
            assert pair[c, k, k, 4] == fields[0, c, mr.TP] + fields[0, c, mr.TN]
            assert pair[c, k, k, 5] == fields[0, c, mr.FP] + fields[0, c, mr.FN]
    # the diagonal of pair reproduces single: S(k,k) are sums of squares whose Cov is a variance, and nobody is "only" right
    assert (pair[:, range(3), range(3), 2:4] == 0).all()
    assert (pair[..., 2:].sum(-1) == (single[:, :1, 1] + single[:, :1, 2])[:, :, None]).all()
    assert (pair[..., 0] == pair[..., 0].transpose(0, 2, 1)).all() and (pair[..., 2] == pair[..., 3].transpose(0, 2, 1)).all()
    got, got_mc = delong_from_sums(single, pair), mcnemar_from_sums(pair)
    for key in dl:
        assert same_bits(got[key], dl[key]), key
    assert same_bits(got_mc, mc)
    theta = dl["theta"]
    with np.errstate(invalid="ignore"):
        auroc = np.where((single[..., 1] > 0) & (single[..., 2] > 0), single[..., 0] / (2.0 * single[..., 1] * single[..., 2]), np.nan)
    assert same_bits(theta, auroc)                          # summarize's value and rule
    if rel in ("same", "monotone"):
        assert (place[0] == place[1]).all()
        assert (dl["var"][:, 0, 1][~np.isnan(dl["var"][:, 0, 1])] == 0).all()
        assert np.isnan(dl["z"][:, 0, 1]).all() and np.isnan(dl["p"][:, 0, 1]).all()
    if lab != "mixed" or N < 4:
        assert np.isnan(dl["z"]).all() and np.isnan(dl["var"]).all()
    elif rel == "independent" and kind == "untied":
        assert (single[..., 1:] >= 2).all() and (dl["var"][:, 0, 1] > 0).all() and np.isfinite(dl["p"][:, 0, 1]).all()


def _midrank(x):
    order = np.argsort(x, kind="stable")
    xs, out = x[order], np.empty(len(x))
    i = 0
    while i < len(x):
        j = i
        while j < len(x) and xs[j] == xs[i]:
            j += 1
        out[order[i:j]] = 0.5 * (i + j - 1) + 1.0
        i = j
    return out


def classic_delong_cov(y, probs):
    """DeLong's covariance as the fast-DeLong papers state it (Sun & Xu 2014): V10 = (TZ - TX) / n, V01 = 1 - (TZ - TY) / m
    from fp64 midranks, Cov = cov(V10) / m + cov(V01) / n.  probs [M, N] finite, y [N] in {0, 1}."""
    pos, neg = y == 1.0, y == 0.0
    m, n = int(pos.sum()), int(neg.sum())
    v10, v01 = [], []
    for p in probs.astype(np.float64):
        x, yy = p[pos], p[neg]
        tz, tx, ty = _midrank(np.concatenate([x, yy])), _midrank(x), _midrank(yy)
        v10.append((tz[:m] - tx) / n)
        v01.append(1.0 - (tz[m:] - ty) / m)
    v10, v01 = np.array(v10), np.array(v01)
    return np.atleast_2d(np.cov(v10)) / m + np.atleast_2d(np.cov(v01)) / n, v10.mean(1)


@pytest.mark.parametrize("kind,N", [("untied", 67), ("untied", 300), ("q3", 300), ("zeros", 257), ("denormal", 130)])
def test_restatement_agrees_with_the_classic_form(kind, N):
    """Inputs with m, n >= 2 and at least three distinct scores.  The bound is N * 2^-50 * sqrt(Cov_kk * Cov_ll): what
    tests/test_metrics_host.py allows an fp64 sum of N terms, scaled to the covariance's size."""
    rng = np.random.default_rng([N, cr.KINDS.index(kind)])
    y = cr.labels("mixed", N, 1, rng)
    y[N // 2, 0] = 1.0                                      # no BAD row here: the classic form has no such thing
    probs = np.stack([cr.scores(kind, N, 1, rng) for _ in range(3)])
    assert (y == 1).sum() >= 2 and (y == 0).sum() >= 2 and all(len(np.unique(p)) >= 3 for p in probs)
    _, single, pair, dl, _ = cr.compare(y, probs)
    cov, theta = classic_delong_cov(y[:, 0], probs[:, :, 0])
    assert np.abs(theta - dl["theta"][0]).max() <= N * 2.0 ** -50
    for k in range(3):
        for l in range(3):
            bound = N * 2.0 ** -50 * math.sqrt(dl["cov"][0, k, k] * dl["cov"][0, l, l])
            print(kind, N, k, l, abs(cov[k, l] - dl["cov"][0, k, l]), bound)
            assert abs(cov[k, l] - dl["cov"][0, k, l]) <= bound, (k, l, cov[k, l], dl["cov"][0, k, l])


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def test_limits_are_refused_before_any_launch(lib):
    err = lambda: lib.ecg_last_error().decode()                                 # noqa: E731
    nul = ctypes.c_void_p(None)
    a = lambda v: ctypes.c_void_p(v)                                            # noqa: E731
    place = lambda N, C: lib.ecg_metrics_placements(nul, nul, nul, nul, nul, N, C, nul)                       # noqa: E731
    sums = lambda N, C, M, thr=0.5: lib.ecg_metrics_paired_sums(nul, nul, nul, nul, nul, nul, N, C, M, thr, nul)   # noqa: E731
    for N in (0, 65537):
        assert place(N, 5) == 1 and f"metrics_placements: N={N} outside [1,65536]" in err()
        assert sums(N, 5, 2) == 1 and f"metrics_paired_sums: N={N} outside [1,65536]" in err()
        assert lib.ecg_metrics_placements_workspace_bytes(N, 5) == 0 and lib.ecg_metrics_paired_sums_workspace_bytes(N, 5, 2) == 0
    for C in (0, 65):
        assert place(10, C) == 1 and f"metrics_placements: C={C} outside [1,64]" in err()
        assert sums(10, C, 2) == 1 and f"metrics_paired_sums: C={C} outside [1,64]" in err()
        assert lib.ecg_metrics_placements_workspace_bytes(10, C) == 0 and lib.ecg_metrics_paired_sums_workspace_bytes(10, C, 2) == 0
    for M in (0, 9):
        assert sums(10, 5, M) == 1 and f"metrics_paired_sums: M={M} outside [1,8]" in err()
        assert lib.ecg_metrics_paired_sums_workspace_bytes(10, 5, M) == 0
    assert sums(10, 5, 2, float("nan")) == 1 and "threshold is NaN" in err()
    assert place(65536, 64) == 1 and "metrics_placements: null pointer" in err()
    assert sums(65536, 64, 8) == 1 and "metrics_paired_sums: null pointer" in err()
    assert lib.ecg_metrics_placements_workspace_bytes(65536, 64) >= 2 * 65536 * 64 * 4
    assert lib.ecg_metrics_paired_sums_workspace_bytes(65536, 64, 8) > 0
    # misaligned bases (addresses only; nothing is launched on a refusal)
    assert lib.ecg_metrics_placements(a(64), a(64), a(66), a(64), a(64), 10, 5, nul) == 1 and "not 4-byte aligned" in err()
    assert lib.ecg_metrics_paired_sums(a(64), a(64), a(64), a(68), a(64), a(64), 10, 5, 2, 0.5, nul) == 1
    assert "single and pair must be 8-byte aligned" in err()
    assert lib.ecg_metrics_paired_sums(a(64), a(64), a(64), a(64), a(68), a(64), 10, 5, 2, 0.5, nul) == 1
    assert "single and pair must be 8-byte aligned" in err()
    assert lib.ecg_metrics_paired_sums(a(64), a(66), a(64), a(64), a(64), a(64), 10, 5, 2, 0.5, nul) == 1
    assert "not 4-byte aligned" in err()


def test_wrappers_refuse_cpu_tensors_and_are_reachable():
    import torch
    from ecg_hip import EcgHipError, functional as hipF, metrics as M
    from src.training import metrics as tm
    for name in ("metrics_placements", "metrics_paired_sums", "delong_from_sums", "mcnemar_from_sums", "compare_models"):
        assert getattr(hipF, name) is getattr(M, name)
    assert tm.compare_models is M.compare_models
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hipF.metrics_placements(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hipF.metrics_paired_sums(torch.zeros(2, 2, 4, dtype=torch.int32), torch.zeros(2, 4, 2), torch.zeros(4, 2))
    with pytest.raises(EcgHipError, match="CUDA tensors"):
        M.compare_models(torch.zeros(4, 2), [torch.zeros(4, 2), torch.zeros(4, 2)])
    with pytest.raises(EcgHipError, match="1 to 8 models"):
        M.compare_models(torch.zeros(4, 2), [])
