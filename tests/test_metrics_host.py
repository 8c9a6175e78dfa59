"""Host checks of the metrics stage.  (1) The numpy restatement (tests/metrics_ref.py) that the GPU tests compare with ==
is itself held to scikit-learn on replicated rows: AUROC and AP within N * 2^-50 absolute (at most N terms, a few fp64
roundings each), F1 with ==, the ROC and precision-recall curves at group ends within the same tolerance.  (2) summarize
gives what the reference's compute_metrics gives on the edge cases, NaN-ness included.  (3) The entry points refuse every
size outside their limits before any launch, asked with NULL pointers."""
import ctypes
import warnings

import numpy as np
import pytest

import metrics_ref as mr
from metrics_util import header_slab, load_lib, metrics_module, same_bits, tol


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.fixture(scope="module")
def slab(lib):
    return lib.ecg_metrics_slab()


def scores(kind, N, C, rng):
    p = rng.random((N, C)).astype(np.float32)
    if kind == "q3":
        p = (np.floor(p * 3) / 3).astype(np.float32)
    elif kind == "q50":
        p = (np.floor(p * 50) / 50).astype(np.float32)
    elif kind == "edge":                                    # scores exactly float32(0.3) and the float below it
        p = (np.floor(p * 50) / 50).astype(np.float32)
        p[::7] = np.float32(0.3)
        p[3::7] = np.nextafter(np.float32(0.3), np.float32(0))
    return p


def labels(N, C, rng):
    y = (rng.random((N, C)) < 0.3).astype(np.float32)
    y[0], y[1] = 1.0, 0.0                                   # both classes present in every column
    return y


def multiplicities(N, B, rng):
    return np.stack([np.bincount(rng.integers(0, N, N), minlength=N) for _ in range(B)]).astype(np.int64)


CASES = [(kind, N, weighted, thr) for kind in ("untied", "q3", "q50", "edge") for N, weighted in ((257, False), (300, True))
         for thr in (0.5, 0.3)] + [("q50", 2198, True, 0.5)]


@pytest.mark.parametrize("kind,N,weighted,thr", CASES, ids=["%s-N%d-w%d-t%s" % c for c in CASES])
def test_restatement_matches_sklearn_on_replicated_rows(kind, N, weighted, thr, slab):
    from sklearn import metrics as skm
    from ecg_hip import metrics as M
    from src.training.metrics import compute_metrics
    rng = np.random.default_rng([sum(map(ord, kind)), N, int(weighted)])
    C = 3
    p, y = scores(kind, N, C, rng), labels(N, C, rng)
    w = multiplicities(N, 2, rng) if weighted else None
    o, nonf = mr.order(p)
    assert (nonf == 0).all() and all(sorted(o[c]) == list(range(N)) for c in range(C))
    fields, ap, curve = mr.counts(p, y, o, w, thr, slab)
    s = M.summarize(fields, ap)
    for b in range(fields.shape[0]):
        idx = np.arange(N) if w is None else np.repeat(np.arange(N), w[b])
        yy, pp = y[idx], p[idx]
        n = len(idx)
        for c in range(C):
            assert abs(s["auroc_per_class"][b, c] - skm.roc_auc_score(yy[:, c], pp[:, c])) <= tol(n)
            assert abs(s["auprc_per_class"][b, c] - skm.average_precision_score(yy[:, c], pp[:, c])) <= tol(n)
            assert s["f1_per_class"][b, c] == skm.f1_score(yy[:, c], (pp[:, c] >= thr).astype(int), zero_division=0)
            # the curves: scikit-learn's points are the group ends
            k = mr.keys(p[o[c], c])
            end = np.append(k[1:] != k[:-1], True)
            tp, fp = curve[b, c, end, 0], curve[b, c, end, 1]
            keep = np.append(True, (np.diff(tp) != 0) | (np.diff(fp) != 0))     # a group whose rows all have weight 0 is no
            tp, fp = tp[keep], fp[keep]                                         # point of the replicated data
            if tp[0] == 0 and fp[0] == 0:
                tp, fp = tp[1:], fp[1:]
            fpr, tpr, _ = skm.roc_curve(yy[:, c], pp[:, c], drop_intermediate=False)
            assert len(fpr) == len(tp) + 1
            assert np.abs(tpr[1:] - tp / fields[b, c, mr.POS]).max() <= tol(n)
            assert np.abs(fpr[1:] - fp / fields[b, c, mr.NEG]).max() <= tol(n)
            prec, rec, _ = skm.precision_recall_curve(yy[:, c], pp[:, c])
            assert len(prec) == len(tp) + 1
            assert np.abs(prec[-2::-1] - tp / (tp + fp)).max() <= tol(n)
            assert np.abs(rec[-2::-1] - tp / fields[b, c, mr.POS]).max() <= tol(n)
        ref = compute_metrics(yy, pp, threshold=thr)
        assert abs(s["auroc_macro"][b] - ref["auroc_macro"]) <= tol(n)
        assert abs(s["auprc_macro"][b] - ref["auprc_macro"]) <= tol(n)
        assert s["f1_macro"][b] == ref["f1_macro"]


def test_vectorised_restatement_equals_the_literal_one(slab):
    rng = np.random.default_rng(5)
    for N in (1, 2, 60, slab + 1, 3 * slab + 1):
        p, y = scores("q3", N, 2, rng), labels(N, 2, rng) if N > 1 else np.ones((1, 2), np.float32)
        if N > 4:
            p[2, 0], p[3, 0], p[4, 1], y[3, 1] = np.nan, -0.0, np.inf, 0.5
        o, _ = mr.order(p)
        w = multiplicities(N, 2, rng)
        for ww in (None, w):
            fields, ap, curve = mr.counts(p, y, o, ww, 0.5, slab)
            for b in range(fields.shape[0]):
                for c in range(2):
                    f, a, cv = mr.counts_literal(p, y, o[c], None if ww is None else ww[b], c, 0.5, slab)
                    assert (f == fields[b, c]).all() and (cv == curve[b, c]).all()
                    assert np.float64(a).view(np.int64) == ap[b, c].view(np.int64)


def test_order_restatement_on_special_values():
    p = np.array([0.5, np.nan, -0.0, 0.0, np.inf, -np.inf, 0.5, -np.nan, 1e-45, -1e-45], np.float32)[:, None]
    o, nonf = mr.order(p)
    assert list(o[0]) == [4, 0, 6, 8, 2, 3, 9, 5, 1, 7] and nonf[0] == 4


def _edge_cases():
    rng = np.random.default_rng(11)
    N, C = 40, 3
    base_p, base_y = scores("q50", N, C, rng), labels(N, C, rng)
    out = {}
    y = base_y.copy()
    y[:, 1] = 0.0
    out["all_negative_column"] = (base_p, y)
    y = base_y.copy()
    y[:, 2] = 1.0
    out["all_positive_column"] = (base_p, y)
    p = base_p.copy()
    p[5, 0] = np.nan
    out["one_nan"] = (p, base_y)
    p = base_p.copy()
    p[7, 1] = np.inf
    out["one_inf"] = (p, base_y)
    out["n1"] = (np.array([[0.7, 0.2, 0.5]], np.float32), np.array([[1.0, 0.0, 1.0]], np.float32))
    return out


@pytest.mark.parametrize("name", sorted(_edge_cases()))
def test_summarize_follows_the_reference_on_edge_cases(name, slab):
    from ecg_hip import metrics as M
    from src.training.metrics import compute_metrics
    p, y = _edge_cases()[name]
    o, _ = mr.order(p)
    fields, ap, _ = mr.counts(p, y, o, None, 0.5, slab)
    s = M.summarize(fields, ap)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = compute_metrics(y, p, threshold=0.5)
    for k in ("auroc_macro", "auprc_macro"):
        got = float(s[k][0])
        assert np.isnan(got) == np.isnan(ref[k]), (k, got, ref[k])
        assert np.isnan(got) or abs(got - ref[k]) <= tol(len(p))
    assert float(s["f1_macro"][0]) == ref["f1_macro"]


def test_limits_are_refused_before_any_launch(lib):
    err = lambda: lib.ecg_last_error().decode()                                 # noqa: E731
    nul = ctypes.c_void_p(None)
    order = lambda N, C: lib.ecg_metrics_order(nul, nul, nul, nul, N, C, nul)   # noqa: E731
    counts = lambda N, C, B, thr=0.5: lib.ecg_metrics_counts(nul, nul, nul, nul, nul, nul, nul, nul, N, C, B, thr, nul)   # noqa: E731
    for N in (0, -1, 65537):
        assert order(N, 5) == 1 and f"metrics_order: N={N} outside [1,65536]" in err()
        assert counts(N, 5, 1) == 1 and f"metrics_counts: N={N} outside [1,65536]" in err()
        assert lib.ecg_metrics_order_workspace_bytes(N, 5) == 0 and lib.ecg_metrics_counts_workspace_bytes(N, 5, 1) == 0
    for C in (0, 65):
        assert order(10, C) == 1 and f"metrics_order: C={C} outside [1,64]" in err()
        assert counts(10, C, 1) == 1 and f"metrics_counts: C={C} outside [1,64]" in err()
        assert lib.ecg_metrics_order_workspace_bytes(10, C) == 0 and lib.ecg_metrics_counts_workspace_bytes(10, C, 1) == 0
    for B in (0, 65537):
        assert counts(10, 5, B) == 1 and f"metrics_counts: B={B} outside [1,65536]" in err()
        assert lib.ecg_metrics_counts_workspace_bytes(10, 5, B) == 0
    assert counts(10, 5, 2) == 1 and "B=2 weight rows need w" in err()
    assert counts(10, 5, 1, float("nan")) == 1 and "threshold is NaN" in err()
    # inside the limits the next thing looked at is the pointers
    assert order(65536, 64) == 1 and "metrics_order: null pointer" in err()
    assert counts(65536, 64, 1) == 1 and "metrics_counts: null pointer" in err()
    assert lib.ecg_metrics_order_workspace_bytes(65536, 64) >= 65536 * 64 * 4
    assert lib.ecg_metrics_counts_workspace_bytes(1, 1, 65536) > 0
    # misaligned bases: 8 bytes for fields and ap, 4 otherwise (addresses only; nothing is launched on a refusal)
    a = lambda v: ctypes.c_void_p(v)                                            # noqa: E731
    assert lib.ecg_metrics_counts(a(64), a(64), a(64), nul, a(68), a(64), nul, a(64), 10, 5, 1, 0.5, nul) == 1
    assert "fields and ap must be 8-byte aligned" in err()
    assert lib.ecg_metrics_counts(a(66), a(64), a(64), nul, a(64), a(64), nul, a(64), 10, 5, 1, 0.5, nul) == 1
    assert "not 4-byte aligned" in err()
    assert lib.ecg_metrics_order(a(64), a(66), a(64), a(64), 10, 5, nul) == 1 and "not 4-byte aligned" in err()


def test_slab_is_the_headers(lib):
    assert lib.ecg_metrics_slab() == header_slab()
    M = metrics_module()
    assert M.slab() == lib.ecg_metrics_slab() and len(M.FIELDS) == mr.FIELDS


def test_wrappers_refuse_cpu_tensors_and_are_reachable_from_functional():
    import torch
    from ecg_hip import EcgHipError, functional as F
    from ecg_hip import metrics as M
    assert F.metrics_order is M.metrics_order and F.metrics_counts is M.metrics_counts
    with pytest.raises(EcgHipError, match="CPU tensor"):
        F.metrics_order(torch.zeros(4, 2))
    with pytest.raises(EcgHipError, match="CPU tensor"):
        F.metrics_counts(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(EcgHipError, match="CUDA tensors"):
        M.compute_metrics_device(torch.zeros(4, 2), torch.zeros(4, 2))


def _literal_percentiles(reps, alpha):
    """The percentile rule column by column: NaN replicates left out, NaN bounds when none is left."""
    q = (100.0 * alpha / 2, 100.0 * (1 - alpha / 2))
    flat = reps.reshape(reps.shape[0], -1)
    lo, hi, n_nan = np.empty(flat.shape[1]), np.empty(flat.shape[1]), np.empty(flat.shape[1], np.int64)
    for j in range(flat.shape[1]):
        kept = flat[:, j][~np.isnan(flat[:, j])]
        with np.errstate(invalid="ignore"):                                     # +inf among the values
            lo[j], hi[j] = np.percentile(kept, q) if kept.size else (np.nan, np.nan)
        n_nan[j] = flat.shape[0] - kept.size
    return lo.reshape(reps.shape[1:]), hi.reshape(reps.shape[1:]), n_nan.reshape(reps.shape[1:])


def test_percentiles_fast_path_and_column_path_agree_by_bits():
    for shape in ((50,), (50, 5), (50, 5, 4)):
        _check_percentiles(metrics_module(), shape, np.random.default_rng(17))


def _check_percentiles(M, shape, rng):
    clean = rng.random(shape)
    holes = np.where(rng.random(shape) < 0.2, np.nan, clean)                    # NaN in some columns (the vector: some entries)
    holes[0] = clean[0]
    lost = holes.copy()
    lost.reshape(shape[0], -1)[:, -1] = np.nan                                  # one column all NaN
    inf = clean.copy()
    inf.reshape(shape[0], -1)[rng.integers(0, shape[0], 7), rng.integers(0, inf[0].size, 7)] = np.inf
    inf_holes = np.where(np.isnan(holes), np.nan, inf)
    for name, reps in (("clean", clean), ("holes", holes), ("lost", lost), ("inf", inf), ("inf_holes", inf_holes)):
        assert np.isnan(reps).any() == (name not in ("clean", "inf"))            # the first and fourth take the fast path
        for alpha in (0.05, 0.5):
            got, want = M._percentiles(reps, alpha), _literal_percentiles(reps, alpha)
            for g, w in zip(got[:2], want[:2]):
                assert np.shape(g) == shape[1:] and np.asarray(g).dtype == np.float64, name
                assert same_bits(g, w), (name, alpha)
            assert np.array_equal(got[2], want[2]) and np.asarray(got[2]).dtype == np.int64, name
    assert np.isnan(M._percentiles(lost, 0.05)[0].reshape(-1)[-1]) and M._percentiles(lost, 0.05)[2].reshape(-1)[-1] == shape[0]


def test_read_once_round_trips_bit_patterns_on_cpu_tensors():
    import torch
    M = metrics_module()
    i64 = np.array([[2 ** 62, -2 ** 62, -1], [0, 2 ** 63 - 1, -2 ** 63]], np.int64)
    i32 = np.array([-1, 2 ** 31 - 1, -2 ** 31, 0, 7], np.int32)
    f64 = np.array([0x8000000000000000, 0x7ff8000000abcdef, 0xfff0000000000001, 1, 0x3ff0000000000001], np.uint64).view(np.float64)
    f32 = np.array([[0x7f800000, 0x80000000], [0x7fc12345, 0xff800001], [0x3f800001, 1]], np.uint32).view(np.float32)
    assert f64[0] == 0 and np.signbit(f64[0]) and np.isnan(f64[1:3]).all() and 0 < f64[3] < 2.3e-308   # -0.0, NaN payloads, a denormal
    assert np.isposinf(f32[0, 0]) and np.isnan(f32[1]).all() and f32[2, 0] == np.nextafter(np.float32(1), np.float32(2))
    arrays = [i64, f32, np.empty((0, 3), np.float64), i32, f64, np.empty(0, np.float32), f64.reshape(5, 1, 1), i32[:1].reshape(())]
    calls = []
    real = torch.Tensor.cpu
    torch.Tensor.cpu = lambda t, *a, **k: calls.append(1) or real(t, *a, **k)
    try:
        got = M._read_once(*[torch.from_numpy(np.array(a)) for a in arrays])
    finally:
        torch.Tensor.cpu = real
    assert len(calls) == 1 and len(got) == len(arrays)
    for g, a in zip(got, arrays):
        assert isinstance(g, np.ndarray) and g.dtype == a.dtype and g.shape == a.shape
        assert g.tobytes() == a.tobytes()
