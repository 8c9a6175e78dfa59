"""Host side of the BatchNorm split tests: the table of tests/bn_split_cases.py against the
library's own split counts, the regimes the table must reach, and tests/bn_ref.py against torch autograd and the C oracle.
The split counts are pure host functions asked with integers only — no device is needed, and this file is how the table
is checked before tests/test_gpu_bn_splits.py runs it."""
import ctypes

import numpy as np
import pytest
import torch

import bn_ref as R
import bn_split_cases as T


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from ecg_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def queried(lib, case):
    """(S, Sw, S2, Sg) as the library answers; the splits do not depend on L, so the row-pass query (which refuses L < 2)
    is asked with L = 2 and strides of 8 where the case's rows are shorter"""
    _, (N, C, L), _, _ = case
    f = (ctypes.c_int * 7)()
    Lq = max(L, 2)
    rc = lib.ecg_bn_relu_pool_h_forms(N, C, Lq, T.up(Lq // 2, 8), T.up(Lq, 8), f)
    assert rc == 0, lib.ecg_last_error().decode()
    assert f[1] == f[5], "the forward and the dx pass stream with the same split count"
    return lib.ecg_bn_stat_partials_count(N, C, L), f[3], f[1], f[6]


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c[0])
def test_case_gets_the_split_counts_the_table_states(lib, case):
    name, (N, C, L), want, _ = case
    S, Sw, S2, Sg = queried(lib, case)
    assert (S, Sw, S2) == want[:3], (name, (S, Sw, S2, Sg))
    assert want[3] == (Sg if L >= 2 else None), (name, Sg)
    # the workspace of the backward holds the wider of the two reduce passes' partials, and (dbeta, dgamma)
    assert lib.ecg_bn_relu_pool_bwd_ws_floats(N, C, L) == C * Sw * 2 + C * 2 and S <= Sw
    assert lib.ecg_bn_bwd_ws_floats(N, C, L) == C * Sw * 2 + C * 2


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c[0])
def test_case_reaches_the_regimes_it_exists_for(case):
    assert set(case[3]) <= T.regimes_of(case), (case[0], sorted(T.regimes_of(case)))


def test_the_table_reaches_every_regime_of_every_pass():
    got = T.reached()
    for p, need in T.REQUIRED.items():
        assert need <= got[p], (p, sorted(need - got[p]))


def test_the_regime_check_notices_a_dropped_case():
    """The coverage assertion above is only worth something if it can fail: for these regimes ONE case is all the table
    has, and without it the regime is not reached."""
    for name, tag in (("gap_two_trips", "gap:rows_gt_16"), ("equal", "reduce:equal"), ("equal", "stream:equal"),
                      ("equal", "wide:equal"), ("one_sample", "gap:one")):
        p, r = tag.split(":")
        assert r in T.reached()[p] and r not in T.reached([c for c in T.CASES if c[0] != name])[p], (name, tag)


def test_the_cases_are_small():
    for name, (N, C, L), _, _ in T.CASES:
        assert N * C * L <= 4_800_000 and N <= 65535 and C <= 65535, name


# ---- tests/bn_ref.py -----------------------------------------------------------------------------------------------------
SHAPES = [(5, 3, 7), (4, 6, 10)]


def _operands(shape, seed):
    N, C, L = shape
    rng = np.random.default_rng(seed)
    y = rng.standard_normal(shape) * 1.5 + 0.3
    gamma, beta = 1 + 0.2 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    dout = rng.standard_normal(shape)
    return y, gamma, beta, dout


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("train", [True, False])
def test_bn_bwd_is_torch_autograd_in_float64(shape, train):
    import torch.nn.functional as TF
    N, C, L = shape
    y, gamma, beta, dout = _operands(shape, 11 + L)
    eps = 1e-5
    if train:
        mean, var = y.mean(axis=(0, 2)), y.var(axis=(0, 2))
    else:
        rng = np.random.default_rng(5)
        mean, var = 0.1 * rng.standard_normal(C), rng.uniform(0.5, 2.0, C)
    invstd = 1.0 / np.sqrt(var + eps)
    ty, tg, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (y, gamma, beta))
    if train:
        out = TF.batch_norm(ty, None, None, tg, tb, True, 0.1, eps)
    else:
        out = TF.batch_norm(ty, torch.tensor(mean), torch.tensor(var), tg, tb, False, 0.1, eps)
    out.backward(torch.tensor(dout))
    dy, dgamma, dbeta = R.bn_bwd(y, dout, gamma, mean, invstd, train)
    np.testing.assert_allclose(dy, ty.grad.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(dgamma, tg.grad.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(dbeta, tb.grad.numpy(), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_split_sums_partition_the_batch_and_give_the_oracles_statistics(oracle, shape):
    N, C, L = shape
    y = _operands(shape, 3)[0].astype(np.float32)
    omean, oinv = oracle.bn_stats(y)
    y64 = y.astype(np.float64)
    for S in range(1, N + 1):
        a, q = R.stat_split_sums(y, S)
        assert a.shape == q.shape == (C, S)
        starts = R.split_starts(N, S) + [N]
        assert list(np.diff(starts)) == list(R.split_counts(N, S)) == T.sizes(N, S)
        for s in range(S):             # each partial is the sum over its own sample range: the partition, not only the total
            np.testing.assert_allclose(a[:, s], y64[starts[s]:starts[s + 1]].sum(axis=(0, 2)), rtol=1e-13, atol=1e-13)
            np.testing.assert_allclose(q[:, s], (y64[starts[s]:starts[s + 1]] ** 2).sum(axis=(0, 2)), rtol=1e-13)
        mu = a.sum(axis=1) / (N * L)
        var = q.sum(axis=1) / (N * L) - mu * mu
        np.testing.assert_allclose(mu, omean, atol=1e-7)
        np.testing.assert_allclose(1.0 / np.sqrt(var + 1e-5), oinv, rtol=1e-6)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("train", [True, False])
def test_routed_backward_is_the_oracles_fused_backward(oracle, shape, train):
    """routing_mask + routed_da + bn_bwd restate oracle.bn_relu_pool_bwd: the fused passes' dgamma / dbeta references are
    the per-split sums of exactly the terms the oracle adds up."""
    N, C, L = shape
    y, gamma, beta, _ = (a.astype(np.float32) for a in _operands(shape, 9))
    dp = np.random.default_rng(2).standard_normal((N, C, L // 2)).astype(np.float32)
    mean, invstd = oracle.bn_stats(y)
    mask = R.routing_mask(oracle, y, gamma, beta, mean, invstd)
    assert mask.shape == y.shape and not mask[:, :, 2 * (L // 2):].any()
    assert np.all(mask[:, :, 0:2 * (L // 2):2].astype(int) + mask[:, :, 1:2 * (L // 2):2] <= 1)      # at most one of a pair
    da = R.routed_da(dp, mask, L)
    dy, dgamma, dbeta = R.bn_bwd(y, da, gamma, mean, invstd, train)
    ody, odg, odb = oracle.bn_relu_pool_bwd(y, dp, gamma, beta, mean, invstd, train)
    np.testing.assert_allclose(dy, ody, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(dgamma, odg, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(dbeta, odb, rtol=1e-6, atol=1e-7)
    for S in (1, 2, N):
        a, q, aa, qa = R.grad_split_sums(y, da, mean, invstd, S)
        np.testing.assert_allclose(a.sum(axis=1), dbeta, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(q.sum(axis=1), dgamma, rtol=1e-12, atol=1e-12)
        assert np.all(aa >= np.abs(a)) and np.all(qa >= np.abs(q))


def test_chain_bound_is_the_stated_formula():
    t = np.array([1.0, -2.0, 0.5])
    assert R.chain_bound(t, 3) == (1 + 12) * 2.0 ** -24 * 3.5
    assert R.chain_bound(t, 256) == (1 + 12) * 2.0 ** -24 * 3.5
    assert R.chain_bound(t, 257) == (2 + 12) * 2.0 ** -24 * 3.5
    assert np.array_equal(R.chain_factor(np.array([1, 256, 257, 2322])), (np.array([1, 1, 2, 10]) + 12) * 2.0 ** -24)
    assert R.gap_row_bound(86, 2.0) == (2 + 8) * 2.0 ** -24 * 2.0
