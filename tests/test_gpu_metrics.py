"""GPU checks of the metrics stage (ecg_metrics_order, ecg_metrics_counts, ecg_hip/metrics.py): order, nonfinite, every
field, the curve and the BITS of ap equal the numpy restatement (tests/metrics_ref.py, itself held to scikit-learn by
tests/test_metrics_host.py).  Shapes are the smallest that can still go wrong: around one wave, around one slab of the
average-precision sum and several of them, 1 000 ranks (just under one chunk of the scan), 4 097 (two tiles of the order
kernel's key stream, five chunks of the scan)."""
import functools

import numpy as np
import pytest
import torch

import metrics_ref as mr
from metrics_util import header_slab, metrics_module, same_bits, tol

pytestmark = pytest.mark.gpu

SLAB = header_slab()
SIZES = sorted({1, 2, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, 3 * SLAB + 1, 1000, 4097})
KINDS = ("equal", "q3", "untied", "zeros", "denormal", "nonfinite")
LABELS = ("mixed", "all0", "all1")
WEIGHTS = (None, 1, 3, 70)
THRESHOLDS = (0.5, 0.3, 0.0, 1.0)


@pytest.fixture(scope="module")
def M():
    assert metrics_module().slab() == SLAB
    return metrics_module()


def make_scores(kind, N, C, rng):
    p = rng.random((N, C)).astype(np.float32)
    if kind == "equal":
        p[:] = np.float32(0.3)
    elif kind == "q3":                                      # tie groups far longer than a slab
        p = (np.floor(p * 3) / 3).astype(np.float32)
    elif kind == "zeros":
        p = np.where(p < 0.4, np.float32(-0.0), np.where(p < 0.8, np.float32(0.0), p)).astype(np.float32)
    elif kind == "denormal":
        p = (rng.integers(-3, 4, (N, C)) * np.float32(1e-45)).astype(np.float32)
    elif kind == "nonfinite":
        p = (np.floor(p * 20) / 20).astype(np.float32)
        sel = rng.random((N, C))
        p[sel < 0.10] = np.nan
        p[(sel >= 0.10) & (sel < 0.17)] = np.inf
        p[(sel >= 0.17) & (sel < 0.24)] = -np.inf
        p[:: 5, 0] = -np.nan                                # another NaN payload: the same key
        if C > 1:
            p[:, C - 1] = np.nan                            # a whole column
        if C > 2:
            p[:, C - 2] = np.inf
    return p


def make_labels(kind, N, C, rng):
    if kind == "all0":
        return np.zeros((N, C), np.float32)
    if kind == "all1":
        return np.ones((N, C), np.float32)
    y = (rng.random((N, C)) < 0.35).astype(np.float32)
    if N >= 3:
        y[N // 2, 0] = 0.5                                  # BAD
    return y


def make_weights(B, N, y, rng):
    if B is None:
        return None
    w = rng.integers(0, 10, (B, N)) * (rng.random((B, N)) < 0.7)
    if B >= 3:
        w[1][(y == 1.0).any(1)] = 0                         # a replicate whose whole positive weight is 0
        w[2] = 0                                            # and one with no weight at all
    return w.astype(np.int32)


def _cases():
    """Every size, kind, label set, weight form, threshold and C at least once, in a rotation instead of a product."""
    out = []
    for n, N in enumerate(SIZES * 2):
        kind = KINDS[n % len(KINDS)]
        lab = LABELS[0] if n % 4 else LABELS[1 + (n // 4) % 2]
        out.append((N, (1, 5, 7)[n % 3], kind, lab, WEIGHTS[(n + n // len(WEIGHTS)) % len(WEIGHTS)], THRESHOLDS[n % 4]))
    out += [(1000, 5, "q3", "mixed", 70, 0.5), (4097, 5, "nonfinite", "mixed", 3, 0.3), (3 * SLAB + 1, 7, "equal", "mixed", 70, 0.3),
            (SLAB + 1, 5, "zeros", "mixed", None, 0.0), (4097, 1, "untied", "mixed", None, 0.5)]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case_data(case):
    N, C, kind, lab, B, thr = case
    rng = np.random.default_rng([N, C, KINDS.index(kind), LABELS.index(lab), B or 0])
    p, y = make_scores(kind, N, C, rng), make_labels(lab, N, C, rng)
    w = make_weights(B, N, y, rng)
    o, nonf = mr.order(p)
    return p, y, w, o, nonf, mr.counts(p, y, o, w, thr, SLAB)


def check(M, p_dev, y_dev, w_dev, thr, want):
    o, nonf, (fields, ap, curve) = want
    got_o, got_nf = M.metrics_order(p_dev)
    assert np.array_equal(got_o.cpu().numpy(), o) and np.array_equal(got_nf.cpu().numpy(), nonf)
    f, a, cv = M.metrics_counts(p_dev, y_dev, order=got_o, weights=w_dev, threshold=thr, curve=True)
    assert f.dtype == torch.int64 and a.dtype == torch.float64 and cv.dtype == torch.int32
    assert np.array_equal(f.cpu().numpy(), fields)
    assert np.array_equal(cv.cpu().numpy(), curve)
    assert same_bits(a.cpu().numpy(), ap)
    f2, a2 = M.metrics_counts(p_dev, y_dev, weights=w_dev, threshold=thr)           # no curve, its own order
    assert torch.equal(f2, f) and same_bits(a2.cpu().numpy(), ap)


@pytest.mark.parametrize("case", CASES, ids=["N%d-C%d-%s-%s-B%s-t%s" % c for c in CASES])
def test_order_and_counts_equal_the_restatement(M, case):
    p, y, w, o, nonf, want = case_data(case)
    dev = torch.device("cuda")
    check(M, torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev), None if w is None else torch.from_numpy(w).to(dev),
          case[5], (o, nonf, want))


def test_cases_cover_what_they_claim():
    assert {c[0] for c in CASES} == set(SIZES) and {c[1] for c in CASES} == {1, 5, 7}
    assert {c[2] for c in CASES} == set(KINDS) and {c[3] for c in CASES} == set(LABELS)
    assert {c[4] for c in CASES} == set(WEIGHTS) and {c[5] for c in CASES} == set(THRESHOLDS)


def test_side_stream_offset_view_and_refusals(M):
    from ecg_hip import EcgHipError
    case = (3 * SLAB + 1, 5, "q3", "mixed", 3, 0.3)
    p, y, w, o, nonf, want = case_data(case)
    dev = torch.device("cuda")
    N, C = p.shape
    buf = torch.full((N * C + 3,), 7.0, device=dev)
    p_dev = buf[1:1 + N * C].view(N, C)                     # 4-byte offset into a larger buffer
    p_dev.copy_(torch.from_numpy(p))
    assert p_dev.data_ptr() % 8 == 4 and p_dev.is_contiguous()
    y_dev, w_dev = torch.from_numpy(y).to(dev), torch.from_numpy(w).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        check(M, p_dev, y_dev, w_dev, case[5], (o, nonf, want))
    side.synchronize()
    assert float(buf[0]) == 7.0 and bool((buf[1 + N * C:] == 7.0).all())
    wide = torch.zeros((N, 2 * C), device=dev)
    for bad in (wide[:, ::2], wide.t()[:C].t()):
        assert not bad.is_contiguous()
        with pytest.raises(EcgHipError, match="contiguous"):
            M.metrics_order(bad)
        with pytest.raises(EcgHipError, match="contiguous"):
            M.metrics_counts(bad, y_dev)
    with pytest.raises(EcgHipError, match="float32"):
        M.metrics_order(p_dev.double())
    with pytest.raises(EcgHipError, match="int32"):
        M.metrics_counts(p_dev, y_dev, weights=w_dev.long())
    with pytest.raises(EcgHipError, match="threshold is NaN"):
        M.metrics_counts(p_dev, y_dev, threshold=float("nan"))


@pytest.fixture(scope="module")
def boot(M):
    rng = np.random.default_rng(21)
    N, C = 300, 5
    p = (np.floor(rng.random((N, C)) * 40) / 40).astype(np.float32)
    y = (rng.random((N, C)) < 0.3).astype(np.float32)
    dev = torch.device("cuda")
    pd, yd = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    run = lambda: dict(M.bootstrap_metrics(yd, pd, n_boot=20, seed=3, threshold=0.5),                   # noqa: E731
                       weights=M.bootstrap_weights(N, 20, 3, dev))
    return p, y, pd, yd, run(), run()


def test_bootstrap_row_zero_is_the_point_value_and_a_seed_repeats(M, boot):
    p, y, pd, yd, a, b = boot
    point = M.compute_metrics_device(yd, pd, threshold=0.5)
    for k in M.MACRO_KEYS:
        assert same_bits(a[k]["point"], point[k]) and same_bits(a[k]["point"], b[k]["point"])
        assert same_bits(a[k]["lo"], b[k]["lo"]) and same_bits(a[k]["hi"], b[k]["hi"])
        assert same_bits(a["replicates"][k], b["replicates"][k])
        assert a[k]["lo"] <= a[k]["hi"] and a["n_nan"][k] == 0
    assert torch.equal(a["weights"], b["weights"])
    w = a["weights"].cpu().numpy()
    assert w.shape == (21, 300) and (w[0] == 1).all() and (w.sum(1) == 300).all() and (w >= 0).all()
    assert len({w[i].tobytes() for i in range(21)}) == 21
    for k in ("auroc_per_class", "auprc_per_class", "f1_per_class"):
        assert same_bits(a[k]["point"], point[k]) and a[k]["lo"].shape == (5,)


def test_bootstrap_replicates_are_the_host_metrics_of_the_drawn_rows(M, boot):
    from src.training.metrics import compute_metrics
    p, y, _, _, a, _ = boot
    w = a["weights"].cpu().numpy()
    for b in range(1, w.shape[0]):
        idx = np.repeat(np.arange(len(p)), w[b])
        ref = compute_metrics(y[idx], p[idx], threshold=0.5)
        for k in M.MACRO_KEYS:
            assert abs(a["replicates"][k][b - 1] - ref[k]) <= tol(len(idx)), (b, k)


def test_curves_are_scikit_learns(M, boot):
    from sklearn import metrics as skm
    p, y, pd, yd, _, _ = boot
    c = 2
    roc, pr = M.roc_curve_device(yd, pd, c), M.pr_curve_device(yd, pd, c)
    fpr, tpr, thr = skm.roc_curve(y[:, c], p[:, c], drop_intermediate=False)
    assert np.array_equal(roc["thresholds"], thr[1:].astype(np.float32))
    assert np.abs(roc["tpr"] - tpr[1:]).max() <= tol(len(p)) and np.abs(roc["fpr"] - fpr[1:]).max() <= tol(len(p))
    prec, rec, thr = skm.precision_recall_curve(y[:, c], p[:, c])
    assert np.array_equal(pr["thresholds"][::-1], thr.astype(np.float32))
    assert np.abs(pr["precision"][::-1] - prec[:-1]).max() <= tol(len(p))
    assert np.abs(pr["recall"][::-1] - rec[:-1]).max() <= tol(len(p))


class _DS(torch.utils.data.Dataset):
    def __init__(self, x, y):
        self.x, self.y = x, y

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


def test_eval_one_epoch_with_device_metrics(M, monkeypatch):
    from src.models.ecg_cnn import ECGCNN
    from src.training.loop import eval_one_epoch
    from src.utils.seed import set_seed
    set_seed(5)
    model = ECGCNN(num_labels=5).cuda()
    rng = np.random.default_rng(2)
    n = 24                                                  # three batches of 8
    x = torch.from_numpy(rng.standard_normal((n, 12, 64)).astype(np.float32))
    y = torch.from_numpy((rng.random((n, 5)) < 0.4).astype(np.float32))
    y[0], y[1] = 1.0, 0.0
    loader = torch.utils.data.DataLoader(_DS(x, y), batch_size=8, shuffle=False)
    monkeypatch.delenv("ECG_HIP_DEVICE_METRICS", raising=False)
    host = eval_one_epoch(model, loader, "cuda")
    monkeypatch.setenv("ECG_HIP_DEVICE_METRICS", "1")
    seen = []
    monkeypatch.setattr("src.training.loop.compute_metrics_device", lambda *a, **k: seen.append(1) or M.compute_metrics_device(*a, **k))
    device = eval_one_epoch(model, loader, "cuda")
    assert seen == [1] and set(device) == set(host) == {"auroc_macro", "auprc_macro", "f1_macro", "bce_loss"}
    assert same_bits(device["bce_loss"], host["bce_loss"])
    for k in M.MACRO_KEYS:
        assert abs(device[k] - host[k]) <= tol(n), (k, device[k], host[k])
