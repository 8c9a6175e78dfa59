"""Host side of the shape-generic convolution tests: no device needed.

The case table of tests/conv_direct_cases.py states, per case, which kernels of csrc/conv1d_direct.hip it takes — a claim
derived from reading the dispatch.  This file ENFORCES the claim: the table covers the classes it says it covers, and the
library's own host queries (pure functions, asked with integers and addresses only, nothing launched) give the same answers
as the table's restatement.  It also holds the float64 restatement the device tests compare with to the CPU oracle
(oracle/ecg_oracle.py, itself held to torch float64 by tests/test_oracle_padding.py), and shows that each checker fails on
an answer with one defect of the kind it is there to catch.  The kernel-level runs are in tests/test_gpu_conv_direct.py."""
import ctypes

import numpy as np
import pytest

import conv_direct_cases as T

A = 1 << 20            # a 16-byte aligned "address"
IDS = T.case_id


@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from ecg_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def _wforms(lib, case, dw=A, db=A, ws=A):
    f = (ctypes.c_int * 6)()
    assert lib.ecg_conv1d_bwd_weight_forms(A, T.out_len(case), dw, db, ws, *case, f) == 0, lib.ecg_last_error().decode()
    return tuple(f)


# ---- the table covers what it claims -------------------------------------------------------------------------------------------
def test_the_table_reaches_every_class_it_names():
    D = {c: T.describe(c) for c in T.CASES}
    for c, d in D.items():
        assert d["fwd_direct"] and d["wgrad_direct"], c
        assert d["wgrad_kernel"] == ("split" if c in T.SPLIT else "generic"), c
    F = [T.describe(c) for c in T.FWD_CASES]
    assert all(d["fwd_direct"] for d in F)
    assert {d["fwd_co_t"] for d in F} == {16, 8, 4, 2, 1}
    assert {d["dgrad_co_t"] for d in D.values() if d["dgrad_direct"]} == {16, 8, 4, 2, 1}
    assert {1, 2, 3} <= {d["fwd_tiles"] for d in F} and {T.out_len(c) for c in T.FWD_CASES} >= {1, 255, 256, 257, 258}
    assert {1, 2, 3} <= {d["dgrad_tiles"] for d in D.values() if d["dgrad_direct"]}
    assert {1, 2, 5, 32} <= {d["fwd_chunks"] for d in F}                 # one short chunk, exactly one, 4 + 1, many
    assert any(c[1] % T.CI_CHUNK == 1 and c[1] > T.CI_CHUNK for c in T.CASES)
    assert {d["G"] for d in D.values()} == {1, 2, 4, 8, 16}
    assert {d["G"] for c, d in D.items() if c in T.SPLIT} == {1, 2, 4, 8, 16}            # on slabs the split kernel wrote
    assert {d["wgrad_kernel"] for d in D.values()} == {"split", "generic"}
    assert all(d["S"] == 1 for c, d in D.items() if c in T.GENERIC)
    split = [(c[0], D[c]["S"]) for c in T.SPLIT]
    assert any(S == 1 and N > 1 for N, S in split) and any(S == N and N > 1 for N, S in split)
    assert any(N % S != 0 for N, S in split)
    assert [b - a for a, b in D[(7, 128, 40, 70, 15, 7)]["slabs"]] == [1, 2, 2, 2]
    # three t tiles inside the split kernel's own loop, and a ragged last one
    assert any(T.cdiv(d["Lo"], T.TT) == 3 and d["Lo"] % T.TT for c, d in D.items() if c in T.SPLIT)
    # both reduce forms standalone (ecg_conv1d_bwd_weight_bias_ld always is; ecg_conv1d_bwd_weight_data_ld where the input
    # gradient is direct) and riding a matrix-core input gradient, on slabs a direct kernel wrote
    assert {(d["reduce"], d["rides"]) for d in D.values()} == {(f, r) for f in (T.R_GROUPED, T.R_FLOAT4) for r in (False, True)}
    assert {d["G"] for d in D.values() if d["rides"]} >= {1, 2, 4}
    assert len(T.FLOAT4_CASES) >= 3 and all(c in T.SPLIT for c in T.FLOAT4_CASES)
    assert {c[4] for c in T.CASES} >= {1, 2, 9, 14, 15, 16, 31}
    assert any(c[5] == 0 for c in T.CASES) and any(c[5] == c[4] - 1 and c[4] > 1 for c in T.CASES)
    assert any(c[5] == 0 for c in T.SPLIT) and any(c[5] == 14 for c in T.SPLIT)
    for c in T.ALIGN_CASES:        # every op direct and one reduce form whatever the addresses: aligned and misaligned runs compare with ==
        d = D[c]
        assert d["dgrad_direct"] and d["reduce"] == T.R_GROUPED and T.reduce_form(c[2] * c[1] * c[4], c[2], d["S"], False)[1] == d["G"]
    assert {D[c]["wgrad_kernel"] for c in T.ALIGN_CASES} == {"split", "generic"}
    # packing: the K > 15 fallback in the middle, last and first; ragged and full 16 x 16 tiles on both paths of the kernel
    ks = [p[2] for p in T.PACK_A]
    assert len(T.PACK_A) == 16 and ks[-1] > 15 and any(k > 15 for k in ks[1:-1]) and ks[0] <= 15
    assert T.PACK_B[0][2] > 15 and T.PACK_B[1][2] <= 15
    assert (16, 16, 15) in T.PACK_A and any(k == 15 and (co % 16 or ci % 16) for co, ci, k in T.PACK_A)


# ---- the library agrees, asked with addresses only ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_library_gives_the_case_its_class(lib, case):
    N, Ci, Co, L, K, pad = case
    d = T.describe(case)
    Lo = d["Lo"]
    assert _wforms(lib, case) == (T.DIRECT, 0, 0, d["S"], d["reduce"], d["G"])
    assert _wforms(lib, case, db=0) == (T.DIRECT, 0, 0, d["S"], d["reduce"], d["G"])          # a null db counts as aligned
    for o in (4, 8):
        for dw, db, ws in ((o, 0, 0), (0, o, 0), (0, 0, o)):
            f = _wforms(lib, case, A + dw, A + db, A + ws)
            if d["reduce"] == T.R_FLOAT4:
                assert f == (T.DIRECT, 0, 0, d["S"], T.R_GROUPED, 1), (case, f)
            else:
                assert f == (T.DIRECT, 0, 0, d["S"], T.R_GROUPED, d["G"]), (case, f)
    assert lib.ecg_conv1d_bwd_weight_ws_floats(*case) == d["S"] * (Co * Ci * K + Co)
    assert lib.ecg_conv1d_fwd_stat_partials(*case) == N * T.cdiv(Lo, T.TT)
    assert lib.ecg_conv1d_dy_row_stride(*case, 1) == Lo and lib.ecg_conv1d_dy_row_stride(*case, 0) == Lo
    mult = lambda op: lib.ecg_conv1d_multiplies_per_output_pair(op, Ci, Co, K, pad)      # noqa: E731
    assert mult(0) == 2 * K and mult(2) == 2 * K and mult(3) == 2 * K
    assert mult(1) == (2 * K if d["dgrad_direct"] else 23)
    assert d["rides"] == (not d["dgrad_direct"])
    # the entry points refuse a padded dY row on these shapes (nothing is launched on a refusal)
    nul = ctypes.c_void_p(None)
    p = ctypes.c_void_p(A)
    assert lib.ecg_conv1d_bwd_weight_bias_ld(p, Lo + 1, p, p, p, p, *case, nul) == 1 and "dense dY rows" in lib.ecg_last_error().decode()
    if d["dgrad_direct"]:
        assert lib.ecg_conv1d_bwd_data_ld(p, Lo + 1, p, p, *case, nul) == 1 and "dense dY rows" in lib.ecg_last_error().decode()


@pytest.mark.parametrize("case", list(T.FWD_ONLY), ids=IDS)
def test_library_gives_the_forward_only_cases_their_partials(lib, case):
    N, Ci, Co, L, K, pad = case
    assert lib.ecg_conv1d_fwd_stat_partials(*case) == N * T.cdiv(T.out_len(case), T.TT)
    assert lib.ecg_conv1d_multiplies_per_output_pair(0, Ci, Co, K, pad) == 2 * K


# ---- the restatement agrees with the oracle ----------------------------------------------------------------------------------
def _rounds_to(got, want64, what):
    """the oracle accumulates in double in its own order and rounds once to fp32: half an ulp of the result, and the
    difference of two double summation orders (far below 1e-10 on sums of magnitude <= 1e3 and <= 1e5 terms)"""
    err = np.abs(got.astype(np.float64) - want64)
    assert np.all(err <= T.EPS24 * np.abs(want64) + 1e-10), (what, float(err.max()))


@pytest.mark.parametrize("case", T.FWD_CASES, ids=IDS)
def test_restatement_agrees_with_the_oracle(oracle, case):
    N, Ci, Co, L, K, pad = case
    c = T.operands(case)
    _rounds_to(oracle.conv1d_fwd(c["x"], c["w"], c["b"], pad), T.fwd64(c["x"], c["w"], c["b"], pad), "y")
    _rounds_to(oracle.conv1d_fwd(c["x"], c["w"], None, pad), T.fwd64(c["x"], c["w"], None, pad), "y without bias")
    if case in T.FWD_ONLY:
        return
    r = T.reference(case)
    _rounds_to(oracle.conv1d_bwd_data(c["dy"], c["w"], L, pad), r["dx"], "dx")
    dw, db = oracle.conv1d_bwd_weight(c["dy"], c["x"], K, pad)
    _rounds_to(dw, r["dw"], "dw")
    _rounds_to(db, r["db"], "db")
    y32 = oracle.conv1d_fwd(c["x"], c["w"], c["b"], pad)
    om, oi = oracle.bn_stats(y32)
    m, i = T.batch_stats64(y32)
    _rounds_to(om, m, "mean")
    _rounds_to(oi, i, "invstd")
    # the per-tile statistics add up to the whole: sum, sum of squares and count
    ts = T.tile_stats(y32).sum(axis=1)
    y64 = y32.astype(np.float64)
    np.testing.assert_allclose(ts[:, 0], y64.sum(axis=(0, 2)), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(ts[:, 1], (y64 * y64).sum(axis=(0, 2)), rtol=1e-12)
    assert np.all(ts[:, 3] == N * T.out_len(case))


def test_operands_and_packs_are_what_the_docstring_says():
    c = T.operands((2, 7, 12, 50, 3, 1))
    assert all(c[k].dtype == np.float32 for k in c)
    assert c["w_fwd"].shape == (3, 7, 12) and c["w_bwd"].shape == (3, 12, 7)
    assert c["w_fwd"][2, 5, 11] == c["w"][11, 5, 2] and c["w_bwd"][0, 11, 5] == c["w"][11, 5, 2]
    assert T.operands((2, 7, 12, 50, 3, 1)) is c and T.reference((2, 7, 12, 50, 3, 1)) is T.reference((2, 7, 12, 50, 3, 1))


# ---- the checkers reject wrong answers ---------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def test_checkers_accept_the_restatement_rounded_to_fp32():
    case = (9, 12, 16, 513, 15, 7)
    c, r = T.operands(case), T.reference(case)
    y = _f32(r["y"])
    # one rounding to fp32: half an ulp of values of magnitude <= 8 is 4.8e-7, 0.024 of the tightest bound
    assert T.check_fwd(y, r["y"]) < 0.03 and T.check_dgrad(_f32(r["dx"]), r["dx"]) < 0.03
    assert T.check_dgrad(_f32(r["dx"]), r["dx"], mfma=True) < 0.03
    assert T.check_wgrad(_f32(r["dw"]), _f32(r["db"]), r["dw"], r["db"], 9, 513) < 0.1
    assert max(T.check_partials(_f32(T.tile_stats(y)[:, :, :2]), y)) <= 0.01
    assert max(T.check_finalize(*map(_f32, T.batch_stats64(y)), r["y"])) < 0.1
    T.check_pack(c["w_fwd"], c["w_bwd"], c["w"])


@pytest.mark.parametrize("case", [(7, 128, 40, 70, 15, 7), (5, 3, 8, 257, 15, 0), (2, 12, 20, 255, 15, 7)], ids=IDS)
def test_weight_gradient_checker_rejects_a_sample_left_out_of_a_slab(case):
    N, Ci, Co, L, K, pad = case
    c, r, d = T.operands(case), T.reference(case), T.describe(case)
    for s, (n0, n1) in enumerate(d["slabs"]):
        n = n1 - 1                               # the last sample of slab s: what an n_end one too small loses
        lost_w, lost_b = T.wgrad64(c["dy"][n:n + 1], c["x"][n:n + 1], K, pad)
        with pytest.raises(AssertionError, match="dw"):
            T.check_wgrad(_f32(r["dw"] - lost_w), _f32(r["db"]), r["dw"], r["db"], N, d["Lo"])
        with pytest.raises(AssertionError, match="db"):
            T.check_wgrad(_f32(r["dw"]), _f32(r["db"] - lost_b), r["dw"], r["db"], N, d["Lo"])


@pytest.mark.parametrize("case", [(9, 12, 16, 513, 15, 7), (2, 1, 1, 300, 1, 0), (2, 6, 10, 64, 31, 15), (1, 4, 8, 257, 5, 2)], ids=IDS)
def test_forward_checker_rejects_a_tap_dropped_at_a_row_end(case):
    N, Ci, Co, L, K, pad = case
    c = T.operands(case)
    ref = T.fwd64(c["x"], c["w"], c["b"], pad)
    Lo = T.out_len(case)
    k = min(K - 1, L - 1 + pad - (Lo - 1))       # the last tap of the last output that still reads a sample: x[L - 1] if pad < K - 1
    s = Lo - 1 + k - pad
    assert 0 <= s < L and (k == K - 1 or s == L - 1)
    y = ref.copy()
    y[:, :, Lo - 1] -= np.einsum("oi,ni->no", c["w"][:, :, k].astype(np.float64), c["x"][:, :, s].astype(np.float64))
    assert T.check_fwd(_f32(ref), ref) < 0.03
    with pytest.raises(AssertionError, match="y"):
        T.check_fwd(_f32(y), ref)
    # and the input gradient, which is the same kernel: dx[0] without the term that reads dy[0] (tap k = pad)
    if case in T.CASES:
        r = T.reference(case)
        dx = r["dx"].copy()
        dx[:, :, 0] -= np.einsum("oi,no->ni", c["w"][:, :, pad].astype(np.float64), c["dy"][:, :, 0].astype(np.float64))
        with pytest.raises(AssertionError, match="dx"):
            T.check_dgrad(_f32(dx), r["dx"])


@pytest.mark.parametrize("case", [(9, 12, 16, 513, 15, 7), (3, 9, 5, 257, 2, 1), (2, 1, 1, 300, 1, 0)], ids=IDS)
def test_statistics_checker_rejects_swapped_and_unmasked_partials(case):
    N, Ci, Co, L, K, pad = case
    c, d = T.operands(case), T.describe(case)
    Lo, tiles = d["Lo"], d["fwd_tiles"]
    y = _f32(T.reference(case)["y"])
    good = _f32(T.tile_stats(y)[:, :, :2])
    assert max(T.check_partials(good, y)) <= 0.01
    # (n, tile) <-> (tile, n): the layout a transposed pidx = tile * N + n would write; the totals are unchanged
    swapped = good.reshape(Co, N, tiles, 2).transpose(0, 2, 1, 3).reshape(Co, N * tiles, 2)
    assert np.array_equal(np.sort(swapped[:, :, 0], axis=1), np.sort(good[:, :, 0], axis=1))
    with pytest.raises(AssertionError, match="partial sum"):
        T.check_partials(swapped, y)
    two = good.copy()                            # just two positions exchanged
    two[:, [0, N * tiles - 1]] = two[:, [N * tiles - 1, 0]]
    with pytest.raises(AssertionError, match="partial sum"):
        T.check_partials(two, y)
    # the sum of squares over the whole 256-wide tile: what the lanes past Lo hold is the convolution continued on zeros
    assert Lo % T.TT
    ext = T.fwd64(c["x"], c["w"], c["b"], pad, extra=tiles * T.TT - Lo)
    assert ext.shape[2] == tiles * T.TT and np.array_equal(_f32(ext[:, :, :Lo]), y)
    unmasked = good.copy()
    unmasked[:, :, 1] = _f32(T.tile_stats(_f32(ext))[:, :, 1])
    full = np.arange(N * tiles) % tiles != tiles - 1
    assert np.array_equal(unmasked[:, full], good[:, full])                  # only the ragged last tile of each row differs
    with pytest.raises(AssertionError, match="partial sum of squares"):
        T.check_partials(unmasked, y)
    with pytest.raises(AssertionError):          # an element nobody wrote
        bad = good.copy()
        bad[Co - 1, N * tiles - 1, 1] = np.nan
        T.check_partials(bad, y)


def test_pack_checker_rejects_a_missing_tap_flip_and_swapped_channel_roles():
    w = T.operands((2, 6, 10, 64, 31, 15))["w"]
    f, b = T.packs(w)
    T.check_pack(f, b, w)
    T.check_pack(f.reshape(-1), None, w)
    with pytest.raises(AssertionError, match="w_bwd"):
        T.check_pack(f, np.ascontiguousarray(w.transpose(2, 0, 1)), w)                   # no tap flip
    with pytest.raises(AssertionError, match="w_fwd"):
        T.check_pack(np.ascontiguousarray(w[:, :, ::-1].transpose(2, 1, 0)), b, w)       # a flip where none belongs
    sq = T.operands((2, 32, 64, 40, 14, 7))["w"][:32]                                    # square: shapes cannot tell the roles apart
    fs, bs = T.packs(sq)
    with pytest.raises(AssertionError, match="w_bwd"):
        T.check_pack(fs, np.ascontiguousarray(bs.transpose(0, 2, 1)), sq)
