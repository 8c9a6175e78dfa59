"""The shape-generic convolution kernels (csrc/conv1d_direct.hip) at every channel tile, slab split, reduce form and tap count,
in guarded buffers, against a float64 restatement.

The cases, their classes, the restatement and the checkers are in tests/conv_direct_cases.py; the class claims there come
from reading the dispatch and are enforced without a device by tests/test_conv_direct_host.py, which also holds the
restatement to the CPU oracle and shows that every checker fails on a wrong answer.  Here each case RUNS: every launch goes
through align_util.run_guarded (operands between NaN / 12345.0 guards, outputs pre-filled with NaN, workspaces of exactly
the queried size, both runs equal bit for bit) with raw pointers through the C ABI, the weight-gradient form is asserted with
ecg_conv1d_bwd_weight_forms on the real pointers, and each test prints its largest error over its bound.

Tolerances are quoted, not re-derived: test_conv_vs_oracle (2e-5 forward, 5e-5 direct input gradient, 2e-6 sqrt(N Lo) + 2e-5
weight / bias gradient), test_conv_random_shapes_vs_oracle (rtol 2e-5, atol 6e-5 where the input gradient is the matrix-core
kernel), test_conv_stats_epilogue_and_finalize (mean 2e-6, invstd rtol 2e-5); each statistics partial is held to the float64
sums of the stored y over its own (n, tile) with the any-order summation bound gamma(256) sum|v|, gamma(257) sum v^2.
The packed weights the kernels read are the permutation written down in numpy, so the convolution tests do not depend on
the pack kernels; those are compared with the same permutation, exactly, in their own test.
"""
import numpy as np
import pytest
import torch

import conv_direct_cases as T
from align_util import run_guarded, same_bits

pytestmark = pytest.mark.gpu
IDS = T.case_id


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return _lib


@pytest.fixture(autouse=True)
def _end_the_session_on_a_device_error():
    """These tests hand raw pointers to kernels.  A failed assertion lets the next test run; an error of the DEVICE does
    not: nothing more is started on a GPU that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, session ended: {e}", returncode=3)


def _ptr(t):
    return None if t is None else t.data_ptr()


def wgrad_forms(L, dy, dw, db, ws, case):
    import ctypes
    f = (ctypes.c_int * 6)()
    L.call("ecg_conv1d_bwd_weight_forms", _ptr(dy), T.out_len(case), _ptr(dw), _ptr(db) or 0, _ptr(ws), *case, f)
    return tuple(f)


# ---- one call of each entry point on operands at the byte offsets off[name] -------------------------------------------------------
def run_forward(L, case, bias, off=None):
    """plain and statistics epilogue in one guarded run -> {y, ys, part [Co][P][2], mean, invstd}"""
    off = off or {}
    N, Ci, Co, Lin, K, pad = case
    c, Lo = T.operands(case), T.out_len(case)
    P = L.query("ecg_conv1d_fwd_stat_partials", *case)
    assert P == N * T.cdiv(Lo, T.TT)

    def body(ar):
        x, wf = ar.put(c["x"], off.get("x", 0)), ar.put(c["w_fwd"], off.get("w", 0))
        b = ar.put(c["b"], off.get("b", 0)) if bias else None
        y, ys = ar.out((N, Co, Lo), off.get("y", 0)), ar.out((N, Co, Lo), off.get("y", 0))
        part = ar.out((Co, P, 2), off.get("part", 0))                  # 8-byte aligned by contract
        mean, inv = ar.out((Co,), off.get("y", 0)), ar.out((Co,), off.get("y", 0))
        L.call("ecg_conv1d_fwd", _ptr(x), _ptr(wf), _ptr(b), _ptr(y), None, *case, L.stream())
        L.call("ecg_conv1d_fwd", _ptr(x), _ptr(wf), _ptr(b), _ptr(ys), _ptr(part), *case, L.stream())
        L.call("ecg_bn_finalize", _ptr(part), P, N * Lo, _ptr(mean), _ptr(inv), None, None, None, Co, 0.1, 1e-5, L.stream())
        return {"y": y, "ys": ys, "part": part, "mean": mean, "invstd": inv}

    return run_guarded(body)


def run_dgrad(L, case, off=None):
    off = off or {}
    N, Ci, Co, Lin, K, pad = case
    c, Lo = T.operands(case), T.out_len(case)

    def body(ar):
        dy, wb, dx = ar.put(c["dy"], off.get("dy", 0)), ar.put(c["w_bwd"], off.get("w", 0)), ar.out((N, Ci, Lin), off.get("dx", 0))
        L.call("ecg_conv1d_bwd_data_ld", _ptr(dy), Lo, _ptr(wb), _ptr(dx), *case, L.stream())
        return {"dx": dx}

    return run_guarded(body)


def run_wgrad(L, case, entry, off=None):
    """entry 'bias': ecg_conv1d_bwd_weight_bias_ld; 'data': ecg_conv1d_bwd_weight_data_ld -> (outputs, forms)"""
    off = off or {}
    N, Ci, Co, Lin, K, pad = case
    c, Lo = T.operands(case), T.out_len(case)
    n_ws = L.query("ecg_conv1d_bwd_weight_ws_floats", *case)
    assert n_ws == T.describe(case)["S"] * (Co * Ci * K + Co)
    forms = []

    def body(ar):
        dy, x = ar.put(c["dy"], off.get("dy", 0)), ar.put(c["x"], off.get("x", 0))
        dw, db = ar.out((Co, Ci, K), off.get("dw", 0)), ar.out((Co,), off.get("db", 0))
        ws = ar.scratch(n_ws, off.get("ws", 0))
        forms.append(wgrad_forms(L, dy, dw, db, ws, case))
        if entry == "bias":
            L.call("ecg_conv1d_bwd_weight_bias_ld", _ptr(dy), Lo, _ptr(x), _ptr(dw), _ptr(db), _ptr(ws), *case, L.stream())
            return {"dw": dw, "db": db}
        wb, dx = ar.put(c["w_bwd"], off.get("w", 0)), ar.out((N, Ci, Lin), off.get("dx", 0))
        L.call("ecg_conv1d_bwd_weight_data_ld", _ptr(dy), Lo, _ptr(x), _ptr(wb), _ptr(dw), _ptr(db), _ptr(dx), _ptr(ws), *case,
               L.stream())
        return {"dw": dw, "db": db, "dx": dx}

    out = run_guarded(body)
    assert forms[0] == forms[1]
    return out, forms[0]


def check_forward(case, bias, r):
    """-> the largest error over its bound of y, the partial sums, the partial sums of squares, mean and invstd"""
    N, Ci, Co, Lin, K, pad = case
    c = T.operands(case)
    ref = T.reference(case)["y" if bias else "y0"] if case in T.CASES else T.fwd64(c["x"], c["w"], c["b"] if bias else None, pad)
    assert same_bits(r["ys"], r["y"]), "the statistics epilogue stores another y than the plain one"
    worst = (T.check_fwd(r["y"], ref),) + T.check_partials(r["part"], r["y"]) + T.check_finalize(r["mean"], r["invstd"], ref)
    print(f"{IDS(case)} bias={int(bias)}: error / bound  y {worst[0]:.3f}  sum {worst[1]:.3f}  sumsq {worst[2]:.3f}  "
          f"mean {worst[3]:.3f}  invstd {worst[4]:.3f}")
    return worst


# ---- forward: plain and statistics epilogues ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", T.FWD_CASES, ids=IDS)
def test_forward_and_each_statistics_partial(L, case, bias):
    assert T.describe(case)["fwd_direct"]
    check_forward(case, bias, run_forward(L, case, bias))


# ---- input gradient where it is the direct kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in T.CASES if T.describe(c)["dgrad_direct"]], ids=IDS)
def test_direct_input_gradient(L, case):
    r = run_dgrad(L, case)
    print(f"{IDS(case)}: error / bound  dx {T.check_dgrad(r['dx'], T.reference(case)['dx']):.3f}")


# ---- weight and bias gradient through both entry points ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_weight_gradient_through_both_entry_points(L, case):
    N, Ci, Co, Lin, K, pad = case
    d, ref = T.describe(case), T.reference(case)
    want = (T.DIRECT, 0, 0, d["S"], d["reduce"], d["G"])
    outs = {}
    for entry in ("bias", "data"):
        outs[entry], form = run_wgrad(L, case, entry)
        assert form == want, (entry, form, want)
    b, f = outs["bias"], outs["data"]
    ratio = T.check_wgrad(b["dw"], b["db"], ref["dw"], ref["db"], N, d["Lo"])
    # standalone reduce or riders of the input gradient: the same slab kernel, the same sums in the same order
    assert same_bits(f["dw"], b["dw"]) and same_bits(f["db"], b["db"])
    rdx = T.check_dgrad(f["dx"], ref["dx"], mfma=d["rides"])
    line = f"{IDS(case)} {d['wgrad_kernel']} S={d['S']} form={d['reduce']} G={d['G']} rides={int(d['rides'])}: error / bound  dw, db {ratio:.3f}  dx {rdx:.3f}"
    if d["reduce"] == T.R_FLOAT4:            # the workspace 4 bytes off: the grouped form on the same slabs, the same bound
        for entry in ("bias", "data"):
            o, form = run_wgrad(L, case, entry, {"ws": 4})
            assert form == (T.DIRECT, 0, 0, d["S"], T.R_GROUPED, 1), (entry, form)
            r4 = T.check_wgrad(o["dw"], o["db"], ref["dw"], ref["db"], N, d["Lo"])
            line += f"  ws+4 {entry} {r4:.3f}"
    print(line)


# ---- DESIGN.md section 13, row "the same on the direct kernel's shapes": packed weights at 4-byte bases ----------------------------
@pytest.mark.parametrize("o", [4, 8])
@pytest.mark.parametrize("case", T.ALIGN_CASES, ids=IDS)
def test_direct_kernels_read_packed_weights_and_operands_at_any_4_byte_base(L, case, o):
    """w_fwd / w_bwd, x, dy, y, dx, dw, db and ws all `o` bytes past a 16-byte boundary (the statistics partials at 8, their
    contract): every direct kernel has one form, so each result equals the aligned run's bit for bit."""
    d = T.describe(case)
    off = {k: o for k in ("x", "w", "b", "y", "dy", "dx", "dw", "db", "ws")}
    off["part"] = 8
    ref = run_forward(L, case, True)
    check_forward(case, True, ref)
    got = run_forward(L, case, True, off)
    assert all(same_bits(got[k], ref[k]) for k in ref)
    assert same_bits(run_dgrad(L, case, off)["dx"], run_dgrad(L, case)["dx"])
    for entry in ("bias", "data"):
        a, fa = run_wgrad(L, case, entry)
        m, fm = run_wgrad(L, case, entry, off)
        assert fa == fm == (T.DIRECT, 0, 0, d["S"], T.R_GROUPED, d["G"])
        assert all(same_bits(m[k], a[k]) for k in a), entry
        r = T.reference(case)
        T.check_wgrad(m["dw"], m["db"], r["dw"], r["db"], case[0], d["Lo"])


# ---- packing against the permutation, exact ----------------------------------------------------------------------------------------
def _pack_sources(table):
    rng = np.random.default_rng(len(table))
    return [rng.standard_normal(s).astype(np.float32) for s in table]


# (table, the problem whose w_bwd is null): a ragged K <= 15 problem, the K > 15 ones in the middle, last and first
PACK_RUNS = [("A", None), ("A", 2), ("A", 7), ("A", 15), ("B", None), ("B", 0), ("B", 1)]


@pytest.mark.parametrize("table,null_bwd", PACK_RUNS, ids=[f"{t}-{'all' if n is None else f'bwd{n}_null'}" for t, n in PACK_RUNS])
def test_grouped_pack_is_the_permutation(L, table, null_bwd):
    """ecg_pack_weights_grouped over a whole table: K <= 15 problems in the tiled kernel (its full-tile and ragged branches),
    K > 15 problems by the plain kernel with a placeholder in the block table — in the middle, last (A) and first (B).
    Every output sits between guards and was pre-filled with NaN: a float written outside, or one left out, fails."""
    shapes = T.PACK_A if table == "A" else T.PACK_B
    ws = _pack_sources(shapes)

    def body(ar):
        srcs = [ar.put(w, 4 * (i % 3)) for i, w in enumerate(ws)]
        gf = [ar.out((K, Ci, Co)) for Co, Ci, K in shapes]
        gb = [None if i == null_bwd else ar.out((K, Co, Ci)) for i, (Co, Ci, K) in enumerate(shapes)]
        L.call("ecg_pack_weights_grouped", L.ptr_table(srcs), L.ptr_table(gf), L.ptr_table(gb), L.int_table([s[0] for s in shapes]),
               L.int_table([s[1] for s in shapes]), L.int_table([s[2] for s in shapes]), len(shapes), L.stream())
        outs = {f"f{i}": t for i, t in enumerate(gf)}
        outs.update({f"b{i}": t for i, t in enumerate(gb)})
        return outs

    out = run_guarded(body)
    for i, w in enumerate(ws):
        T.check_pack(out[f"f{i}"], out.get(f"b{i}"), w)
        assert (f"b{i}" in out) == (i != null_bwd)


@pytest.mark.parametrize("shape", sorted(set(T.PACK_A + T.PACK_B)), ids=lambda s: "x".join(map(str, s)))
def test_single_pack_is_the_permutation(L, shape):
    Co, Ci, K = shape
    w = _pack_sources([shape])[0]

    def body(ar):
        src = ar.put(w, 4)
        f, b, f1, b1 = ar.out((K, Ci, Co)), ar.out((K, Co, Ci)), ar.out((K, Ci, Co), 4), ar.out((K, Co, Ci), 8)
        L.call("ecg_conv1d_pack_weights", _ptr(src), _ptr(f), _ptr(b), Co, Ci, K, L.stream())
        L.call("ecg_conv1d_pack_weights", _ptr(src), _ptr(f1), None, Co, Ci, K, L.stream())          # either output alone
        L.call("ecg_conv1d_pack_weights", _ptr(src), None, _ptr(b1), Co, Ci, K, L.stream())
        return {"f": f, "b": b, "f1": f1, "b1": b1}

    out = run_guarded(body)
    T.check_pack(out["f"], out["b"], w)
    T.check_pack(out["f1"], out["b1"], w)
