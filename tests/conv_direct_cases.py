"""The case table, the float64 restatement and the checkers of the shape-generic convolution tests (csrc/conv1d_direct.hip).
No torch, no device.

Shared by tests/test_conv_direct_host.py (confirms every class claim below against the library's own host queries, holds
the restatement to the oracle and feeds each checker a wrong answer) and tests/test_gpu_conv_direct.py (runs the cases in
guarded buffers).  The class of a case — which kernels it takes, their tiles, the slab count S, the reduce form and G — comes
from READING the dispatch (conv1d_api.hip, pick_co_tile, direct_wgrad_splits, wgrad_reduce_describe) and is restated in
`describe`; it is a claim until the host test has asked the library, and a claim that turns out wrong is corrected in the
table, never in the assertion.  The CLASS is the requirement of a case, the shape only the way to reach it.

A case is (N, Ci, Co, L, K, pad).  Operands are unit-variance white noise with w / sqrt(Ci K), seeded from the case, the
distribution every tolerance quoted by the checkers was set for (tests/test_gpu_ops.py: test_conv_vs_oracle,
test_conv_random_shapes_vs_oracle, test_conv_stats_epilogue_and_finalize).
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

TT = 256                     # outputs per workgroup of conv1d_direct_kernel and per t tile of the split weight-gradient kernel
CI_CHUNK = 8                 # input channels staged in LDS per pass
DIRECT = 3                   # ECG_WGRAD_SLABS_DIRECT
R_GROUPED, R_FLOAT4 = 0, 1   # ECG_WGRAD_REDUCE_*
EPS24 = 2.0 ** -24           # unit roundoff of fp32


def cdiv(a, b):
    return (a + b - 1) // b


def out_len(case):
    N, Ci, Co, L, K, pad = case
    return L + 2 * pad - K + 1


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------
def mfma_fwd(Ci, Co, K):
    """mfma_fwd_supported: the forward of (Ci -> Co), and with the roles swapped the input gradient"""
    return K == 15 and Ci % 4 == 0 and Co % 32 == 0


def mfma_wgrad(Co, K):
    return K == 15 and Co % 32 == 0


def co_tile(Co):
    return next((c for c in (16, 8, 4, 2) if Co % c == 0), 1)


def wgrad_splits(N, Ci, Co, K):
    if not (K == 15 and Co % 8 == 0):
        return 1
    return max(1, min(N, cdiv(2048, Ci * (Co // 8))))


def slab_ranges(N, S):
    """samples [n_begin, n_end) of slab s"""
    return [(N * s // S, N * (s + 1) // S) for s in range(S)]


def reduce_form(wslab, Co, S, aligned=True):
    """wgrad_reduce_describe -> (form, G); aligned: ws, dw and db (or a null db) all on 16 bytes"""
    groups = cdiv(wslab + Co, 64)
    if wslab % 4 == 0 and Co % 4 == 0 and groups >= 1024 and aligned:
        return R_FLOAT4, 1
    G = 1
    while G < 16 and groups * G < 1024 and S // (2 * G) >= 8:
        G *= 2
    return R_GROUPED, G


def describe(case):
    N, Ci, Co, L, K, pad = case
    Lo = out_len(case)
    S = wgrad_splits(N, Ci, Co, K)
    form, G = reduce_form(Co * Ci * K, Co, S)
    return {
        "Lo": Lo,
        "fwd_direct": not mfma_fwd(Ci, Co, K), "dgrad_direct": not mfma_fwd(Co, Ci, K), "wgrad_direct": not mfma_wgrad(Co, K),
        "fwd_co_t": co_tile(Co), "fwd_tiles": cdiv(Lo, TT), "fwd_chunks": cdiv(Ci, CI_CHUNK),
        # the input gradient is the forward of dy with the roles swapped and pad' = K - 1 - pad
        "dgrad_co_t": co_tile(Ci), "dgrad_tiles": cdiv(L, TT), "dgrad_chunks": cdiv(Co, CI_CHUNK), "dgrad_pad": K - 1 - pad,
        "wgrad_kernel": "split" if K == 15 and Co % 8 == 0 else "generic",
        "S": S, "slabs": slab_ranges(N, S), "reduce": form, "G": G,
        "rides": mfma_fwd(Co, Ci, K),          # ecg_conv1d_bwd_weight_data_ld: the reduce rides on a matrix-core input gradient
    }


# ---- the table: {case: what it is there for} -------------------------------------------------------------------------------------
SPLIT = {      # conv1d_wgrad_direct_kernel<15, 8>: K == 15, C_out % 8 == 0, C_out % 32 != 0
    (1, 3, 8, 40, 15, 7): "S = 1, one tile",
    (5, 3, 8, 257, 15, 0): "S = N, Lo = 243",
    (9, 12, 16, 513, 15, 7): "S = 9; three t tiles with a ragged last; forward CO_T = 16; two chunks",
    (4, 33, 24, 256, 15, 3): "Ci no multiple of 8, Lo = 248",
    (16, 3, 8, 70, 15, 14): "S = 16, grouped G = 2, pad = K - 1",
    (40, 1, 8, 33, 15, 7): "S = 40, G = 4, one input channel",
    (64, 1, 8, 20, 15, 7): "G = 8",
    (130, 1, 8, 20, 15, 7): "G = 16, rows shorter than one wave",
    (7, 128, 40, 70, 15, 7): "S = 4 over 7 samples (slabs of 1, 2, 2, 2); float4 reduce, riding a matrix-core input gradient",
    (7, 64, 72, 300, 15, 7): "the same with two t tiles",
    (3, 256, 72, 30, 15, 7): "S = 1 with N > 1, float4, 32 chunks",
    (16, 32, 8, 40, 15, 7): "direct slabs, grouped G = 2 riding a matrix-core input gradient",
    (40, 32, 8, 33, 15, 7): "the same with G = 4",
    (5, 112, 40, 20, 15, 7): "float4 reduce of direct slabs in front of a DIRECT input gradient (S = 4 over 5 samples)",
}
GENERIC = {    # conv1d_wgrad_generic_kernel: S = 1
    (2, 1, 1, 300, 1, 0): "K = 1, CO_T = 1, two tiles",
    (3, 9, 5, 257, 2, 1): "K = 2, Lo = 258 (two outputs in the second tile), 9 channels: a chunk of 8 and one more",
    (2, 17, 6, 64, 16, 15): "K = 16, pad = K - 1, CO_T = 2",
    (2, 6, 10, 64, 31, 15): "K = 31",
    (1, 8, 16, 1, 31, 30): "L = 1: every output is mostly padding",
    (2, 8, 16, 90, 9, 8): "an existing shape, kept for continuity",
    (2, 7, 12, 50, 3, 1): "CO_T = 4",
    (3, 5, 3, 600, 15, 7): "K = 15 but odd C_out; three tiles",
    (2, 12, 20, 255, 15, 7): "Lo = 255",
    (2, 32, 64, 40, 14, 7): "block geometry at K = 14: 16-wide tiles on both sides",
    (2, 32, 36, 100, 15, 7): "generic slabs under a matrix-core input gradient",
}
FWD_ONLY = {   # forward (both epilogues) only: row lengths at the tile edge
    (6, 3, 4, 1, 3, 1): "Lo = 1",
    (2, 5, 2, 256, 3, 1): "Lo = 256: exactly one tile",
    (1, 4, 8, 257, 5, 2): "Lo = 257: one output in the second tile",
}
CASES = list(SPLIT) + list(GENERIC)
FWD_CASES = CASES + list(FWD_ONLY)
FLOAT4_CASES = [c for c in CASES if describe(c)["reduce"] == R_FLOAT4]
ALIGN_CASES = [(9, 12, 16, 513, 15, 7), (3, 9, 5, 257, 2, 1)]     # one split, one generic: every op direct, the reduce grouped

# (Co, Ci, K) of the packing tests.  A: sixteen problems, the K > 15 ones (one plain launch each, a placeholder in the block
# table) in the middle and last; B: the K > 15 problem first
PACK_A = [(17, 33, 15), (16, 16, 15), (5, 7, 3), (40, 24, 15), (3, 2, 1), (1, 1, 1), (33, 16, 15), (6, 17, 16), (2, 3, 15),
          (8, 8, 9), (20, 4, 5), (4, 40, 2), (12, 12, 14), (7, 1, 15), (16, 17, 15), (10, 6, 31)]
PACK_B = [(6, 17, 16), (32, 12, 15)]


def case_id(case):
    return "x".join(map(str, case))


# ---- operands and the float64 restatement ----------------------------------------------------------------------------------------
_cache = {}


def operands(case):
    """{x, w, b, dy} fp32, seeded from the case; the packed weights as the permutation they are DEFINED to be."""
    if ("op", case) not in _cache:
        N, Ci, Co, L, K, pad = case
        rng = np.random.default_rng(sum(case) * 31 + L)
        c = {"x": rng.standard_normal((N, Ci, L)).astype(np.float32),
             "w": (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32),
             "b": rng.standard_normal(Co).astype(np.float32),
             "dy": rng.standard_normal((N, Co, out_len(case))).astype(np.float32)}
        c["w_fwd"], c["w_bwd"] = packs(c["w"])
        _cache[("op", case)] = c
    return _cache[("op", case)]


def packs(w):
    """w [Co][Ci][K] -> (w_fwd [K][Ci][Co], w_bwd [K][Co][Ci] tap-flipped)"""
    return w.transpose(2, 1, 0).copy(), w[:, :, ::-1].transpose(2, 0, 1).copy()       # (copy: C order, fresh strides at any size)


def windows(x, K, pad, extra=0):
    """x [N][C][L] -> float64 [N][C][Lo + extra][K]: the K samples under every output of zero-padded rows"""
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (0, 0), (pad, pad + extra)))
    return sliding_window_view(xp, K, axis=2)


def fwd64(x, w, b, pad, extra=0):
    """extra > 0: `extra` more outputs past the row end, computed as the kernel's lanes past Lo compute them (on zeros)"""
    y = np.einsum("nitk,oik->not", windows(x, w.shape[2], pad, extra), np.asarray(w, np.float64), optimize=True)
    return y if b is None else y + np.asarray(b, np.float64)[None, :, None]


def dgrad64(dy, w, pad):
    K = w.shape[2]
    return fwd64(dy, np.asarray(w)[:, :, ::-1].transpose(1, 0, 2), None, K - 1 - pad)


def wgrad64(dy, x, K, pad):
    dy = np.asarray(dy, np.float64)
    return np.einsum("not,nitk->oik", dy, windows(x, K, pad), optimize=True), dy.sum(axis=(0, 2))


def reference(case):
    """float64 {y (with bias), y0 (without), dx, dw, db} of the case's operands, computed once"""
    if ("ref", case) not in _cache:
        N, Ci, Co, L, K, pad = case
        c = operands(case)
        r = {"y0": fwd64(c["x"], c["w"], None, pad), "dx": dgrad64(c["dy"], c["w"], pad)}
        r["y"] = r["y0"] + c["b"].astype(np.float64)[None, :, None]
        r["dw"], r["db"] = wgrad64(c["dy"], c["x"], K, pad)
        assert r["y"].shape == (N, Co, out_len(case)) and r["dx"].shape == (N, Ci, L) and r["dw"].shape == (Co, Ci, K)
        _cache[("ref", case)] = r
    return _cache[("ref", case)]


def tile_stats(y):
    """y [N][Co][Lo] -> float64 [Co][N * tiles][4]: sum, sum of squares, sum of magnitudes and count of y over t in
    [256 tile, min(Lo, 256 tile + 256)) at position n * tiles + tile, the layout partials[co][n * tiles + tile][2] of
    conv1d_direct_kernel<CO_T, true>."""
    y = np.asarray(y, np.float64)
    N, Co, Lo = y.shape
    tiles = cdiv(Lo, TT)
    out = np.zeros((Co, N * tiles, 4))
    for n in range(N):
        for tile in range(tiles):
            v = y[n, :, TT * tile:TT * tile + TT]
            out[:, n * tiles + tile] = np.stack([v.sum(1), (v * v).sum(1), np.abs(v).sum(1), np.full(Co, v.shape[1])], axis=1)
    return out


def batch_stats64(y, eps=1e-5):
    y = np.asarray(y, np.float64)
    return y.mean(axis=(0, 2)), 1.0 / np.sqrt(y.var(axis=(0, 2)) + eps)


# ---- checkers: functions of numpy arrays; each returns the largest error over its bound and asserts it is <= 1 --------------------
def gamma(m):
    """|fl(sum of m fp32 terms, any order) - sum| <= gamma(m - 1) * sum of magnitudes <= gamma(m) * ..."""
    return m * EPS24 / (1 - m * EPS24)


def _worst(err, bound, what):
    ratio = float(np.max(err / bound))
    i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    assert np.isfinite(ratio) and ratio <= 1.0, f"{what}: error {err[i]:.3e} over bound {np.broadcast_to(bound, err.shape)[i]:.3e} at {i}"
    return ratio


def _err(got, want):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want)
    return np.where(np.isfinite(err), err, np.inf)


def check_fwd(y, ref):
    """test_conv_vs_oracle: atol 2e-5"""
    return _worst(_err(y, ref), 2e-5, "y")


def check_dgrad(dx, ref, mfma=False):
    """direct kernel: atol 5e-5 (test_conv_vs_oracle); matrix-core kernel: rtol 2e-5, atol 6e-5 (test_conv_random_shapes_vs_oracle)"""
    return _worst(_err(dx, ref), 6e-5 + 2e-5 * np.abs(ref) if mfma else 5e-5, "dx")


def check_wgrad(dw, db, ref_dw, ref_db, N, Lo):
    """test_conv_vs_oracle: atol 2e-6 sqrt(N Lo) + 2e-5 on dw and db"""
    tol = 2e-6 * np.sqrt(N * Lo) + 2e-5
    return max(_worst(_err(dw, ref_dw), tol, "dw"), _worst(_err(db, ref_db), tol, "db"))


def check_partials(part, y_stored):
    """part [Co][P][2] against the float64 sums of the STORED y, position by position: gamma(256) sum|v| on the sum,
    gamma(257) sum v^2 on the sum of squares (each square rounded once, then at most 256 terms added in any order)."""
    want = tile_stats(y_stored)
    part = np.asarray(part)
    assert part.shape == want.shape[:2] + (2,), (part.shape, want.shape)
    assert (want[:, :, 3] >= 1).all()
    tiny = 1e-40                                         # an all-zero tile: 0 <= 0
    rs = _worst(_err(part[:, :, 0], want[:, :, 0]), gamma(256) * want[:, :, 2] + tiny, "partial sum")
    rq = _worst(_err(part[:, :, 1], want[:, :, 1]), gamma(257) * want[:, :, 1] + tiny, "partial sum of squares")
    return rs, rq


def check_finalize(mean, invstd, ref_y):
    """test_conv_stats_epilogue_and_finalize: mean atol 2e-6, invstd rtol 2e-5, against the float64 statistics"""
    m, i = batch_stats64(ref_y)
    return _worst(_err(mean, m), 2e-6, "mean"), _worst(_err(invstd, i), 2e-5 * np.abs(i), "invstd")


def check_pack(w_fwd, w_bwd, w):
    """exact: the packed operands ARE these permutations"""
    f, b = packs(w)
    if w_fwd is not None:
        assert np.array_equal(np.asarray(w_fwd).reshape(f.shape), f), "w_fwd is not w.transpose(2, 1, 0)"
    if w_bwd is not None:
        assert np.array_equal(np.asarray(w_bwd).reshape(b.shape), b), "w_bwd is not w[:, :, ::-1].transpose(2, 0, 1)"
