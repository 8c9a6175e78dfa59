"""GPU checks of the paired comparison (ecg_metrics_placements, ecg_metrics_paired_sums, compare_models): placements, every
paired sum and every float of DeLong's and McNemar's tests equal the restatement (tests/compare_ref.py, itself held to hand
cases and to the classic form by tests/test_compare_host.py) with ==, floats as bits.  Sizes sit around one wave and around
one and two chunks of the scan (1024 ranks); 4097 is also two tiles of the order kernel."""
import csv
import functools
import os
import sys

import numpy as np
import pytest
import torch

import compare_ref as cr
from metrics_util import ROOT, metrics_module, same_bits

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)
CS = (1, 5, 7)
MS = (1, 2, 3)
THRESHOLDS = (0.5, 0.3)
SENTINEL = -7


@pytest.fixture(scope="module")
def M():
    return metrics_module()


def _cases():
    """Every size, kind, label set, C, M and relation at least once, in a rotation instead of a product."""
    out = []
    for n, N in enumerate(SIZES * 2):
        lab = cr.LABELS[0] if n % 4 else cr.LABELS[1 + (n // 4) % 2]
        out.append((N, CS[n % 3], cr.KINDS[n % len(cr.KINDS)], lab, MS[(n + n // 3) % 3], cr.RELATIONS[(n + n // 4) % 4],
                    THRESHOLDS[n % 2]))
    out += [(1025, 5, "q3", "mixed", 2, "independent", 0.5), (2049, 7, "q3", "mixed", 3, "one_row", 0.5),
            (4097, 5, "q3", "mixed", 2, "monotone", 0.3), (4097, 1, "equal", "mixed", 2, "independent", 0.5),
            (1024, 5, "nonfinite", "mixed", 3, "independent", 0.3), (65, 7, "untied", "mixed", 3, "same", 0.5)]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case_data(case):
    N, C, kind, lab, nm, rel, thr = case
    rng = np.random.default_rng([N, C, cr.KINDS.index(kind), cr.LABELS.index(lab), nm, cr.RELATIONS.index(rel)])
    a, y = cr.scores(kind, N, C, rng), cr.labels(lab, N, C, rng)
    probs = np.stack([a, cr.related(rel, a, kind, rng), cr.scores(kind, N, C, rng)][:nm])
    return y, probs, cr.compare(y, probs, thr)


def test_cases_cover_what_they_claim_and_are_not_vacuous():
    assert {c[0] for c in CASES} == set(SIZES) and {c[1] for c in CASES} == set(CS)
    assert {c[2] for c in CASES} == set(cr.KINDS) and {c[3] for c in CASES} == set(cr.LABELS)
    assert {c[4] for c in CASES} == set(MS) and {c[5] for c in CASES if c[4] > 1} == set(cr.RELATIONS)
    seen = 0
    for case in CASES:
        N, C, kind, lab, nm, rel, thr = case
        if lab == "mixed" and N >= 63 and nm >= 2:
            _, _, (_, single, _, dl, _) = case_data(case)
            assert (single[..., 1:] >= 2).all(), case
            k = 1 if rel == "independent" else nm - 1       # an independent model: the second, or the third of three
            if k > 0 and (rel == "independent" or nm == 3):
                assert np.isfinite(dl["var"][:, 0, k]).all(), case
                seen += int(np.isfinite(dl["z"][:, 0, k]).any())
    assert seen >= 5


def _device(y, probs):
    dev = torch.device("cuda")
    return torch.from_numpy(y).to(dev), [torch.from_numpy(p).to(dev) for p in probs]


def _call_with_sentinels(M, yd, pds, thr):
    """The two entry points through the C ABI, outputs prefilled, workspaces of exactly the size the helpers state."""
    from ecg_hip import _lib as L
    N, C = yd.shape
    nm = len(pds)
    dev = yd.device
    places = torch.full((nm, C, N), SENTINEL, dtype=torch.int32, device=dev)
    for k, p in enumerate(pds):
        order = M.metrics_order(p)[0]
        ws = torch.empty(L.query("ecg_metrics_placements_workspace_bytes", N, C), dtype=torch.uint8, device=dev)
        L.call("ecg_metrics_placements", L.ptr(p), L.ptr(yd), L.ptr(order), L.ptr(places[k]), L.ptr(ws), N, C, L.stream())
    single = torch.full((C, nm, 3), SENTINEL, dtype=torch.int64, device=dev)
    pair = torch.full((C, nm, nm, 6), SENTINEL, dtype=torch.int64, device=dev)
    ws = torch.empty(L.query("ecg_metrics_paired_sums_workspace_bytes", N, C, nm), dtype=torch.uint8, device=dev)
    L.call("ecg_metrics_paired_sums", L.ptr(places), L.ptr(torch.stack(pds)), L.ptr(yd), L.ptr(single), L.ptr(pair), L.ptr(ws),
           N, C, nm, float(thr), L.stream())
    return places, single, pair


@pytest.mark.parametrize("case", CASES, ids=["N%d-C%d-%s-%s-M%d-%s-t%s" % c for c in CASES])
def test_placements_sums_and_tests_equal_the_restatement(M, case):
    N, C, kind, lab, nm, rel, thr = case
    y, probs, (place, single, pair, dl, mc) = case_data(case)
    yd, pds = _device(y, probs)
    got_place, got_single, got_pair = _call_with_sentinels(M, yd, pds, thr)
    assert np.array_equal(got_place.cpu().numpy(), place)                   # -1 on BAD rows, no sentinel left
    assert np.array_equal(got_single.cpu().numpy(), single) and np.array_equal(got_pair.cpu().numpy(), pair)
    for k, p in enumerate(pds):
        order = M.metrics_order(p)[0]
        assert torch.equal(M.metrics_placements(p, yd), got_place[k])       # order computed
        assert torch.equal(M.metrics_placements(p, yd, order), got_place[k])   # order given
        fields, _ = M.metrics_counts(p, yd, order=order, threshold=thr)
        assert torch.equal(fields[0, :, M.U2], got_single[:, k, 0])         # the same number by another route
    s2, q2 = M.metrics_paired_sums(got_place, torch.stack(pds), yd, threshold=thr)
    assert torch.equal(s2, got_single) and torch.equal(q2, got_pair)
    if rel in ("same", "monotone") and nm >= 2:
        assert torch.equal(got_place[0], got_place[1])
    names = ["m%d" % k for k in range(nm)]
    out = M.compare_models(yd, dict(zip(names, pds)), threshold=thr)
    assert out["names"] == names and set(out["pairs"]) == {(a, b) for a in names for b in names if a != b}
    assert np.array_equal(out["nonfinite"], (~np.isfinite(probs)).sum(1))
    for k in range(nm):
        one = M.compute_metrics_device(yd, pds[k], threshold=thr)
        assert all(same_bits(out["models"][names[k]][key], one[key]) for key in one)
        assert same_bits(out["models"][names[k]]["auroc_per_class"], dl["theta"][:, k])
        for l in range(nm):
            if k == l:
                continue
            d = out["pairs"][(names[k], names[l])]
            assert same_bits(d["delta_auroc"], dl["delta"][:, k, l]) and same_bits(d["var"], dl["var"][:, k, l])
            assert same_bits(d["z"], dl["z"][:, k, l]) and same_bits(d["p_delong"], dl["p"][:, k, l])
            assert same_bits(d["p_mcnemar"], mc[:, k, l])
            assert np.array_equal(d["k_only"], pair[:, k, l, 2]) and np.array_equal(d["l_only"], pair[:, k, l, 3])
            other = M.compute_metrics_device(yd, pds[l], threshold=thr)
            for key in M.MACRO_KEYS:
                assert same_bits(d["delta_" + key], one[key] - other[key])


def test_side_stream_offset_view_and_refusals(M):
    from ecg_hip import EcgHipError
    case = (1025, 5, "q3", "mixed", 2, "independent", 0.5)
    y, probs, (place, single, pair, _, _) = case_data(case)
    yd, pds = _device(y, probs)
    N, C = y.shape
    buf = torch.full((N * C + 3,), 7.0, device=yd.device)
    p0 = buf[1:1 + N * C].view(N, C)                        # 4-byte offset into a larger buffer
    p0.copy_(pds[0])
    assert p0.data_ptr() % 8 == 4
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = torch.stack([M.metrics_placements(p0, yd), M.metrics_placements(pds[1], yd)])
        s, q = M.metrics_paired_sums(got, torch.stack([p0, pds[1]]), yd)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), place) and np.array_equal(s.cpu().numpy(), single)
    assert np.array_equal(q.cpu().numpy(), pair) and float(buf[0]) == 7.0 and bool((buf[1 + N * C:] == 7.0).all())
    wide = torch.zeros((N, 2 * C), device=yd.device)
    bad = wide[:, ::2]
    assert not bad.is_contiguous()
    with pytest.raises(EcgHipError, match="contiguous"):
        M.compare_models(yd, [pds[0], bad])
    with pytest.raises(EcgHipError, match="contiguous"):
        M.metrics_placements(bad, yd)
    with pytest.raises(EcgHipError, match="contiguous"):
        M.metrics_paired_sums(got.transpose(1, 2).contiguous().transpose(1, 2), torch.stack(pds), yd)
    with pytest.raises(EcgHipError, match="int32"):
        M.metrics_paired_sums(got.long(), torch.stack(pds), yd)
    with pytest.raises(EcgHipError, match="differ in shape"):
        M.metrics_placements(pds[0], yd[:-1])
    with pytest.raises(EcgHipError, match="threshold is NaN"):
        M.metrics_paired_sums(got, torch.stack(pds), yd, threshold=float("nan"))
    with pytest.raises(EcgHipError, match="y_true's shape"):
        M.compare_models(yd, [pds[0], pds[1][:-1]])


def test_paired_bootstrap_is_the_difference_of_two_bootstraps_on_the_same_draws(M):
    case = (1025, 5, "untied", "mixed", 2, "independent", 0.5)
    y, probs, _ = case_data(case)
    yd, pds = _device(y, probs)
    out = M.compare_models(yd, pds, names=["a", "b"], n_boot=8, seed=11)
    boots = [M.bootstrap_metrics(yd, p, n_boot=8, seed=11) for p in pds]
    points = [M.compute_metrics_device(yd, p) for p in pds]
    for (k, l) in ((0, 1), (1, 0)):
        d = out["pairs"][("ab"[k], "ab"[l])]
        assert set(d["bootstrap"]) == set(points[0])
        for key in points[0]:
            reps = boots[k]["replicates"][key] - boots[l]["replicates"][key]
            assert d["replicates"][key].shape[0] == 8 and same_bits(d["replicates"][key], reps)
            assert same_bits(d["bootstrap"][key]["point"], points[k][key] - points[l][key])
            lo, hi = d["bootstrap"][key]["lo"], d["bootstrap"][key]["hi"]
            assert np.all(lo <= hi) and np.all(d["n_nan"][key] == 0)
            assert np.all(reps.min(0) <= lo) and np.all(hi <= reps.max(0))
        assert np.abs(d["replicates"]["auroc_macro"]).max() > 0


def test_refusals_through_the_c_abi_launch_nothing(M):
    from ecg_hip import _lib as L
    lib = L.load()
    err = lambda: lib.ecg_last_error().decode()             # noqa: E731
    N, C = 64, 5
    dev = torch.device("cuda")
    y = torch.zeros((N, C), device=dev)
    p = torch.zeros((2, N, C), device=dev)
    order = torch.zeros((C, N), dtype=torch.int32, device=dev)
    place = torch.full((2, C, N), SENTINEL, dtype=torch.int32, device=dev)
    single = torch.full((C, 2, 3), SENTINEL, dtype=torch.int64, device=dev)
    pair = torch.full((C, 2, 2, 6), SENTINEL, dtype=torch.int64, device=dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    s = L.stream()
    for n, c in ((0, C), (65537, C), (N, 0), (N, 65)):
        assert lib.ecg_metrics_placements(None, None, None, None, None, n, c, s) == 1 and "outside" in err()
        assert lib.ecg_metrics_paired_sums(None, None, None, None, None, None, n, c, 2, 0.5, s) == 1 and "outside" in err()
        assert lib.ecg_metrics_placements_workspace_bytes(n, c) == 0
        assert lib.ecg_metrics_paired_sums_workspace_bytes(n, c, 2) == 0
    for m in (0, 9):
        assert lib.ecg_metrics_paired_sums(None, None, None, None, None, None, N, C, m, 0.5, s) == 1 and f"M={m} outside" in err()
        assert lib.ecg_metrics_paired_sums_workspace_bytes(N, C, m) == 0
    a = [L.ptr(t) for t in (p[0], y, order, place[0], ws)]
    for i in range(5):
        assert lib.ecg_metrics_placements(*[None if j == i else v for j, v in enumerate(a)], N, C, s) == 1 and "null pointer" in err()
        assert lib.ecg_metrics_placements(*[v + 2 if j == i else v for j, v in enumerate(a)], N, C, s) == 1
        assert "not 4-byte aligned" in err()
    b = [L.ptr(t) for t in (place, p, y, single, pair, ws)]
    for i in range(6):
        assert lib.ecg_metrics_paired_sums(*[None if j == i else v for j, v in enumerate(b)], N, C, 2, 0.5, s) == 1
        assert "null pointer" in err()
        off = 4 if i in (3, 4) else 2                       # the int64 outputs: a base off 8 bytes; the others off 4
        assert lib.ecg_metrics_paired_sums(*[v + off if j == i else v for j, v in enumerate(b)], N, C, 2, 0.5, s) == 1
        assert ("must be 8-byte aligned" if i in (3, 4) else "not 4-byte aligned") in err()
    assert lib.ecg_metrics_paired_sums(*b, N, C, 2, float("nan"), s) == 1 and "threshold is NaN" in err()
    torch.cuda.synchronize()
    assert bool((place == SENTINEL).all()) and bool((single == SENTINEL).all()) and bool((pair == SENTINEL).all())


def test_compare_predictions_tool_on_a_merged_csv(M, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import compare_predictions as tool
    finally:
        sys.path.pop(0)
    labels = ["CD", "HYP", "MI", "NORM", "STTC"]
    rng = np.random.default_rng(65)
    N = 65
    y = (rng.random((N, 5)) < 0.4).astype(np.float32)
    base = (np.floor(rng.random((N, 5)) * 30) / 30).astype(np.float32)
    mm = np.clip(base + (rng.random((N, 5)) - 0.4).astype(np.float32) * np.float32(0.3), 0, 1).astype(np.float32)
    path = tmp_path / "merged.csv"
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow([f"y_true_{s}" for s in labels] + [f"y_prob_{s}" for s in labels] + [f"y_prob_{s}_mm" for s in labels] +
                    ["y_true_AF", "y_prob_AF"])
        for i in range(N):
            wr.writerow([repr(float(v)) for v in y[i]] + [repr(float(v)) for v in base[i]] + [repr(float(v)) for v in mm[i]] +
                        [repr(float(y[i, 0])), repr(float(base[i, 2]))])
    out = tool.compare_csv(str(path))
    _, single, pair, dl, mc = cr.compare(y, np.stack([base, mm]), 0.5)
    assert out["labels"] == labels and out["rows"] == N and out["threshold"] == 0.5
    d = out["pairs"]["baseline_vs_multimodal"]
    assert same_bits(d["delta_auroc"], dl["delta"][:, 0, 1]) and same_bits(d["var"], dl["var"][:, 0, 1])
    assert same_bits(d["z"], dl["z"][:, 0, 1]) and same_bits(d["p_delong"], dl["p"][:, 0, 1])
    assert same_bits(d["p_mcnemar"], mc[:, 0, 1]) and np.isfinite(d["z"]).all()
    assert d["k_only"] == pair[:, 0, 1, 2].tolist() and d["l_only"] == pair[:, 0, 1, 3].tolist()
    assert same_bits(out["models"]["baseline"]["auroc_per_class"], dl["theta"][:, 0])
    assert same_bits(out["models"]["multimodal"]["auroc_per_class"], dl["theta"][:, 1])
    af = M.compute_metrics_device(torch.from_numpy(y[:, :1]).cuda(), torch.from_numpy(base[:, 2:3].copy()).cuda())
    assert same_bits(out["af"]["auroc_macro"], af["auroc_macro"])
    import json
    json.dumps(out)                                         # what the command line prints
