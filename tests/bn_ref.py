"""float64 numpy references of the BatchNorm pieces the C oracle lacks — TEST INFRASTRUCTURE ONLY.

    xhat   = (y - mean) * invstd
    dbeta  = sum da,  dgamma = sum da * xhat                              over (n, t) of a channel
    dy     = gamma * invstd * (da - dbeta / M - xhat * dgamma / M)        train, M = N * L
    dy     = gamma * invstd * da                                          eval

`da` is the gradient that reaches the BatchNorm output: dout itself for the unfused ecg_bn_bwd; for the fused passes the
pooled gradient routed through max-pool and ReLU (routed_da, from a routing mask the C oracle computed with the kernels' own
fmaf expression).  Everything is float64; mean and invstd are INPUTS (the fp32 numbers the kernels are handed).

split_sums gives the sums of one split [N*s/S, N*(s+1)/S) of the samples at a time — what one workgroup of a reduce pass
must produce — and chain_bound what fp32 may have done to such a sum.
"""
import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def split_starts(N, S):
    assert 1 <= S <= N
    return [N * s // S for s in range(S)]


def split_counts(N, S):
    """samples per split"""
    return np.array([N * (s + 1) // S - N * s // S for s in range(S)], dtype=np.int64)


def split_sums(terms, S):
    """terms [N][C][...] -> [C][S] float64: the sum over the samples [N*s/S, N*(s+1)/S) and everything behind the channel"""
    t = np.asarray(terms, dtype=np.float64)
    N, C = t.shape[:2]
    per = t.reshape(N, C, -1).sum(axis=2)                        # [N][C]
    return np.add.reduceat(per, split_starts(N, S), axis=0).T.copy()


def stat_split_sums(y, S):
    """-> (sum y, sum y^2) per split, each [C][S] float64: what ecg_bn_stat_partials must write at [c][s]"""
    y = np.asarray(y, dtype=np.float64)
    return split_sums(y, S), split_sums(y * y, S)


def chain_factor(count):
    """Relative first-order error of a sum of `count` terms taken the way every reduce pass takes it: 256 threads stride
    the terms (ceil(count / 256) additions in the longest thread), then six shuffle levels and three wave adds (9), and 3
    more roundings for the term itself (the fmaf, and the subtraction and the multiplication that make xhat)."""
    count = np.asarray(count)
    return (np.ceil(count / 256.0) + 12) * U


def chain_bound(terms, count):
    """(ceil(count / 256) + 12) * 2^-24 * sum |terms|"""
    return float(chain_factor(count)) * float(np.abs(np.asarray(terms, dtype=np.float64)).sum())


def xhat(y, mean, invstd):
    y = np.asarray(y, dtype=np.float64)
    return (y - np.asarray(mean, dtype=np.float64)[None, :, None]) * np.asarray(invstd, dtype=np.float64)[None, :, None]


def bn_bwd(y, da, gamma, mean, invstd, train):
    """plain BatchNorm1d backward -> (dy [N][C][L], dgamma [C], dbeta [C]) in float64"""
    da = np.asarray(da, dtype=np.float64)
    N, C, L = da.shape
    xh = xhat(y, mean, invstd)
    dbeta, dgamma = da.sum(axis=(0, 2)), (da * xh).sum(axis=(0, 2))
    gi = (np.asarray(gamma, dtype=np.float64) * np.asarray(invstd, dtype=np.float64))[None, :, None]
    if train:
        M = float(N * L)
        dy = gi * (da - dbeta[None, :, None] / M - xh * dgamma[None, :, None] / M)
    else:
        dy = gi * da
    return dy, dgamma, dbeta


def grad_split_sums(y, da, mean, invstd, S):
    """-> (sum da, sum da*xhat, sum |da|, sum |da*xhat|) per split, each [C][S] float64: the two numbers workgroup (c, s)
    of a backward reduce pass must write, and the magnitudes their error bounds scale with"""
    da = np.asarray(da, dtype=np.float64)
    q = da * xhat(y, mean, invstd)
    return split_sums(da, S), split_sums(q, S), split_sums(np.abs(da), S), split_sums(np.abs(q), S)


def routing_mask(oracle, y, gamma, beta, mean, invstd):
    """[N][C][L] bool: where the C oracle's eval-mode backward puts a pooled gradient of ones — its dy is
    gamma * invstd * da there and an exact zero elsewhere.  The oracle decides with the kernels' fmaf expression in fp32,
    so this is the routing the kernels must take, tie for tie."""
    y = np.asarray(y, dtype=np.float32)
    assert np.all(np.asarray(gamma) * np.asarray(invstd) != 0)
    ones = np.ones(y.shape[:2] + (y.shape[2] // 2,), np.float32)
    dy, _, _ = oracle.bn_relu_pool_bwd(y, ones, gamma, beta, mean, invstd, False)
    return dy != 0


def routed_da(dp, mask, L):
    """dp [N][C][L/2] and the routing mask [N][C][L] (True where the pooled gradient lands: the arg-max of a pair whose
    pooled value passed the ReLU) -> da [N][C][L] float64.  An odd tail sample never reaches the pool: da = 0."""
    dp = np.asarray(dp, dtype=np.float64)
    N, C, Lp = dp.shape
    da = np.zeros((N, C, L))
    da[:, :, :2 * Lp] = np.repeat(dp, 2, axis=2)
    return np.where(mask, da, 0.0)


def grad_bound(abs_split_sums, pairs_per_split, ref):
    """|device - ref| allowed for a dgamma / dbeta [C]: chain_bound of every split's own sum, summed over the S splits (the
    combine adds the partials in double), plus one fp32 rounding of the result."""
    f = chain_factor(pairs_per_split)[None, :]
    return (f * abs_split_sums).sum(axis=1) + U * np.abs(ref)


def gap_row_bound(Lp, row_mean):
    """|device - ref| allowed for a row mean of the pooled tensor: 64 lanes stride the Lp values (ceil(Lp / 64) additions),
    six shuffle levels, the division, and one to spare; the pooled values are >= 0, so mean |p| is the row mean itself."""
    return (math.ceil(Lp / 64) + 8) * U * np.abs(np.asarray(row_mean, dtype=np.float64))
