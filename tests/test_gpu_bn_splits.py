"""The BatchNorm row passes where a workgroup owns SEVERAL samples.

Every pass of csrc/bn_relu_pool.hip (fp32 rows) and csrc/bn_relu_pool_h.hip (bf16 rows) gives a workgroup one channel and
the samples [N*s/S, N*(s+1)/S); it walks them flat, recovers (sample, pair) by division, keeps four or more loads in flight
and clamps the dead ones; the forward and the dx pass fold in a 256-strided combine of the partials.  Every other test that
holds these passes to an independent reference runs N <= 4, where a split is exactly one sample.  The table of
tests/bn_split_cases.py (checked without a device by tests/test_bn_splits_host.py) reaches ragged and equal multi-sample
splits, single workgroups that own the whole batch, second trips of the flat walk and of the average pass's row loop, and
combines of more than 256 partials.

References: the C oracle (double accumulation, the kernels' own fmaf expression: pooled values and routing compare exactly)
for the fused passes' tensors, tests/bn_ref.py (float64 numpy) for the per-split sums and the unfused backward.  Every
operand sits in a guarded buffer (tests/align_util.py): outputs are pre-filled with NaN, `ws` has exactly the size the
library asks for, every call runs twice (finite and NaN guards) and the two runs must agree bit for bit.

Bounds (none is fitted to what the kernels return):
  * a partial sum, dgamma, dbeta: bn_ref.chain_bound — (ceil(count/256) + 12) 2^-24 sum|terms| per split, summed over the
    splits, plus one fp32 rounding of the result;
  * mean 2e-6 (atol), invstd 2e-5 (rtol), running statistics 1e-6 / 1e-5: test_conv_stats_epilogue_and_finalize's bars;
  * a row mean of the pooled tensor: (ceil(Lp/64) + 8) 2^-24 times the row mean;
  * dY: 2e-5 (atol), test_bn_relu_pool_fwd_bwd's bar at this input scale; bf16 dY: half a bf16 ulp, 2^-8 |ref|, on top;
  * pooled values, zero patterns, pads, folded against standalone forms, dense against padded calls: exact.
"""
import functools

import numpy as np
import pytest
import torch

import bn_ref as R
import bn_split_cases as T
from align_util import run_guarded
from util import bf16_round, dev

pytestmark = pytest.mark.gpu

MOMENTUM, EPS = 0.1, 1e-5
CASES_H = [c for c in T.CASES if c[1][2] >= 2]          # the bf16 passes and the average passes refuse L < 2
_ids = lambda c: c[0]       # noqa: E731


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


def _zero_bits(a):
    return not np.ascontiguousarray(a).view(np.int32).any()


# ---------------------------------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------------------------------
# Tests of one function run case by case (the case is the outermost parameter), so ONE case's tensors are alive at a time:
# they are seeded and rebuilt when the next test function comes back to the case.  What is kept for the whole session is
# small or needed by several tests: the device's statistics, the routing mask and the per-split sums.
_kept = {}


@functools.lru_cache(maxsize=1)
def _operands(name, shape):
    N, C, Lo = shape
    rng = np.random.default_rng(N * 1000003 + C * 1009 + Lo)
    c = {"y": (rng.standard_normal(shape) * 1.5 + 0.3).astype(np.float32),
         "gamma": (1 + 0.2 * rng.standard_normal(C)).astype(np.float32),
         "beta": (0.2 * rng.standard_normal(C)).astype(np.float32),
         "dp": rng.standard_normal((N, C, Lo // 2)).astype(np.float32),
         "dg": rng.standard_normal((N, C)).astype(np.float32),
         "dout": rng.standard_normal(shape).astype(np.float32)}
    c["yh"], c["dph"] = bf16_round(c["y"]), bf16_round(c["dp"])          # the bf16 passes' values, pre-rounded
    return c


def operands(case):
    return _operands(case[0], case[1])


def device_stats(L, case, h=False):
    """(partials [C*S*2], mean, invstd) of y (h: of the bf16-rounded y) as ecg_bn_stat_partials + ecg_bn_finalize give them:
    the statistics the forward and backward tests hand to kernel and reference alike.  test_statistics holds them to the
    float64 reference."""
    key = (case[0], "stats", h)
    if key not in _kept:
        N, C, Lo = case[1]
        S = case[2][0]
        yd = dev(operands(case)["yh" if h else "y"])
        part, mean, inv = torch.empty(C * S * 2, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        L.call("ecg_bn_stat_partials", L.f32(yd), L.f32(part), N, C, Lo, L.stream())
        L.call("ecg_bn_finalize", L.f32(part), S, N * Lo, L.f32(mean), L.f32(inv), None, None, None, C, MOMENTUM, EPS, L.stream())
        _kept[key] = tuple(t.cpu().numpy() for t in (part, mean, inv))
    return _kept[key]


def reference(L, oracle, case, what, h=False):
    """References on the device's own (mean, invstd); the mask and the sums are kept, the tensors computed where used."""
    key = (case[0], what, h)
    if key in _kept:
        return _kept[key]
    c = operands(case)
    N, C, Lo = case[1]
    Lp = Lo // 2
    y, dp = (c["yh"], c["dph"]) if h else (c["y"], c["dp"])
    _, mean, inv = device_stats(L, case, h)
    if what == "pooled":
        return oracle.bn_relu_pool_fwd(y, c["gamma"], c["beta"], mean, inv)
    if what == "dp_gap":                 # the kernels' own product: dg * (1 / Lp), both fp32
        return np.repeat((c["dg"] * np.float32(1.0 / Lp))[:, :, None], Lp, axis=2).astype(np.float32)
    if what[0] == "fused":               # ("fused", gap, train) -> the oracle's (dy, dgamma, dbeta)
        _, gap, train = what
        d = reference(L, oracle, case, "dp_gap", h) if gap else dp
        return oracle.bn_relu_pool_bwd(y, d, c["gamma"], c["beta"], mean, inv, bool(train))
    if what == "mask":
        r = R.routing_mask(oracle, y, c["gamma"], c["beta"], mean, inv)
    elif what[0] == "sums":              # ("sums", gap, S) -> per-split (sum da, sum da xhat, sum |da|, sum |da xhat|)
        _, gap, S = what
        d = reference(L, oracle, case, "dp_gap", h) if gap else dp
        da = R.routed_da(d, reference(L, oracle, case, "mask", h), Lo)
        r = R.grad_split_sums(y, da, mean, inv, S)
    else:
        raise KeyError(what)
    _kept[key] = r
    return r


def assert_grads(got_dgamma, got_dbeta, sums, terms_per_split):
    """dgamma / dbeta within chain_bound of the float64 sums, split by split, plus one fp32 rounding of the result"""
    a, q, aa, qa = sums
    for name, got, s, sa in (("dbeta", got_dbeta, a, aa), ("dgamma", got_dgamma, q, qa)):
        ref = s.sum(axis=1)
        err, bound = np.abs(got.astype(np.float64) - ref), R.grad_bound(sa, terms_per_split, ref)
        k = int(np.argmax(err - bound))
        print(f"{name}: max err {err.max():.3e}, worst channel {k}: err {err[k]:.3e} bound {bound[k]:.3e}")
        assert np.all(err <= bound), (name, k, err[k], bound[k])


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES, ids=_ids)
def test_statistics(L, oracle, case):
    """ecg_bn_stat_partials partial by partial, ecg_bn_finalize, and the combine folded into ecg_bn_stats_relu_pool_fwd."""
    name, (N, C, Lo), (S, _, _, _), _ = case
    Lp = Lo // 2
    assert L.query("ecg_bn_stat_partials_count", N, C, Lo) == S
    c = operands(case)
    modes = (0, 1) if Lo >= 2 else (0,)
    state = []

    def body(ar):
        y, gamma, beta = ar.put(c["y"]), ar.put(c["gamma"], 4), ar.put(c["beta"], 4)
        part = ar.out((C * S * 2,), 8)
        L.call("ecg_bn_stat_partials", _ptr(y), _ptr(part), N, C, Lo, L.stream())
        outs = {"part": part}
        for tag in ("fin",) + modes:
            mean, inv = ar.out((C,), 4), ar.out((C,), 4)
            rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
            nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
            if tag == "fin":
                L.call("ecg_bn_finalize", _ptr(part), S, N * Lo, _ptr(mean), _ptr(inv), _ptr(rm), _ptr(rv), _ptr(nbt), C,
                       MOMENTUM, EPS, L.stream())
            else:
                out = ar.out((N, C), 4) if tag == 1 else ar.out((N, C, Lp)) if Lp else None
                L.call("ecg_bn_stats_relu_pool_fwd", _ptr(part), S, N * Lo, _ptr(rm), _ptr(rv), _ptr(nbt), MOMENTUM, EPS,
                       _ptr(y), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv), _ptr(out), N, C, Lo, tag, L.stream())
            outs.update({f"mean{tag}": mean, f"inv{tag}": inv, f"rm{tag}": rm, f"rv{tag}": rv})
            state.append(nbt)
        return outs
    o = run_guarded(body)
    assert all(int(t.item()) == 1 for t in state), "the batch counter has more than one writer (or none)"

    # every partial against the float64 sums of ITS OWN sample range: the partition, not only the total
    a, q = R.stat_split_sums(c["y"], S)
    aa = R.split_sums(np.abs(c["y"]), S)
    f = R.chain_factor(R.split_counts(N, S) * Lo)[None, :]
    part = o["part"].reshape(C, S, 2).astype(np.float64)
    ea, eq = np.abs(part[:, :, 0] - a), np.abs(part[:, :, 1] - q)
    print(f"partials: sum err/bound {np.max(ea / (f * aa)):.3f}, sum of squares err/bound {np.max(eq / (f * q)):.3f}")
    assert np.all(ea <= f * aa) and np.all(eq <= f * q)

    orm, orv = np.zeros(C, np.float32), np.ones(C, np.float32)
    omean, oinv = oracle.bn_stats(c["y"], orm, orv, np.zeros((), np.int64), MOMENTUM, EPS)
    np.testing.assert_allclose(o["meanfin"], omean, atol=2e-6)
    np.testing.assert_allclose(o["invfin"], oinv, rtol=2e-5)
    np.testing.assert_allclose(o["rmfin"], orm, atol=1e-6)
    np.testing.assert_allclose(o["rvfin"], orv, rtol=1e-5, atol=1e-6)
    for m in modes:                      # the folded combine: the standalone launch's bits
        for k in ("mean", "inv", "rm", "rv"):
            assert np.array_equal(o[f"{k}{m}"], o[f"{k}fin"]), (k, m)
    # and what the other tests of this file take as the device's statistics is what was checked here
    p0, m0, i0 = device_stats(L, case)
    assert np.array_equal(p0, o["part"]) and np.array_equal(m0, o["meanfin"]) and np.array_equal(i0, o["invfin"])


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES, ids=_ids)
def test_forward(L, oracle, case):
    """Pool forward (standalone and with the combine folded in) bit for bit; the average forward within its row bound."""
    name, (N, C, Lo), (S, _, _, _), _ = case
    Lp = Lo // 2
    c = operands(case)
    part0, mean0, inv0 = device_stats(L, case)

    def body(ar):
        y, gamma, beta = ar.put(c["y"]), ar.put(c["gamma"], 4), ar.put(c["beta"], 4)
        mean, inv, part = ar.put(mean0, 4), ar.put(inv0, 4), ar.put(part0, 8)
        outs = {}
        p = ar.out((N, C, Lp)) if Lp else None
        L.call("ecg_bn_relu_pool_fwd", _ptr(y), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv), _ptr(p), N, C, Lo, L.stream())
        outs["p"] = p
        if Lo >= 2:
            g = ar.out((N, C), 4)
            L.call("ecg_bn_relu_pool_gap_fwd", _ptr(y), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv), _ptr(g), N, C, Lo,
                   L.stream())
            outs["g"] = g
        for mode in (0, 1) if Lo >= 2 else (0,):
            out = ar.out((N, C), 4) if mode else ar.out((N, C, Lp)) if Lp else None
            m2, i2 = ar.out((C,), 4), ar.out((C,), 4)
            L.call("ecg_bn_stats_relu_pool_fwd", _ptr(part), S, N * Lo, None, None, None, MOMENTUM, EPS, _ptr(y), _ptr(gamma),
                   _ptr(beta), _ptr(m2), _ptr(i2), _ptr(out), N, C, Lo, mode, L.stream())
            outs[f"out{mode}"] = out
        return outs
    o = run_guarded(body)
    if Lp == 0:
        return                                       # an empty pooled tensor: the launches and the guards were the test
    rp = reference(L, oracle, case, "pooled")
    assert np.array_equal(o["p"], rp), "ecg_bn_relu_pool_fwd"
    assert np.array_equal(o["out0"], rp), "ecg_bn_stats_relu_pool_fwd, mode 0"
    rg = rp.astype(np.float64).mean(axis=2)
    bound = R.gap_row_bound(Lp, rg)
    for k in ("g", "out1"):
        err = np.abs(o[k] - rg)
        print(f"{k}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound), k
    assert np.array_equal(o["g"], o["out1"])         # the folded form runs the same additions


# ---------------------------------------------------------------------------------------------------------------------
# fused backward (fp32 rows)
# ---------------------------------------------------------------------------------------------------------------------
# (the average form refuses L < 2: an empty pooled row has no average)
FUSED = [(c, False) for c in T.CASES] + [(c, True) for c in CASES_H]


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("case,gap", FUSED, ids=[c[0] + ("-gap" if g else "-pool") for c, g in FUSED])
def test_fused_backward(L, oracle, case, gap, train):
    """ecg_bn_relu_pool_bwd_ld / ecg_bn_relu_pool_gap_bwd_ld with dense and 64-padded dY rows."""
    name, (N, C, Lo), (S, _, _, _), _ = case
    Lp = Lo // 2
    c = operands(case)
    _, mean0, inv0 = device_stats(L, case)
    n_ws = L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo)
    strides = (Lo, T.up(Lo, 64))
    fn = "ecg_bn_relu_pool_gap_bwd_ld" if gap else "ecg_bn_relu_pool_bwd_ld"

    def body(ar):
        y, gamma, beta = ar.put(c["y"]), ar.put(c["gamma"], 4), ar.put(c["beta"], 4)
        mean, inv = ar.put(mean0, 4), ar.put(inv0, 4)
        g = ar.put(c["dg"], 4) if gap else ar.put(c["dp"]) if Lp else None
        outs = {}
        for ld in strides:
            dy, dga, dbe, ws = ar.out((N, C, ld)), ar.out((C,), 4), ar.out((C,), 4), ar.scratch(n_ws)
            L.call(fn, _ptr(y), _ptr(g), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv), _ptr(dy), ld, _ptr(dga), _ptr(dbe),
                   _ptr(ws), N, C, Lo, train, L.stream())
            outs.update({f"dy{ld}": dy, f"dgamma{ld}": dga, f"dbeta{ld}": dbe})
        return outs
    o = run_guarded(body)                            # (guards of every ws checked; two runs equal bit for bit)
    dense, padded = o[f"dy{strides[0]}"], o[f"dy{strides[1]}"]
    assert np.array_equal(padded[:, :, :Lo], dense) and _zero_bits(padded[:, :, Lo:])
    assert np.array_equal(o[f"dgamma{strides[0]}"], o[f"dgamma{strides[1]}"])
    assert np.array_equal(o[f"dbeta{strides[0]}"], o[f"dbeta{strides[1]}"])
    rdy, _, _ = reference(L, oracle, case, ("fused", gap, train))
    print(f"dY: max err {np.abs(dense - rdy).max():.3e}")
    np.testing.assert_allclose(dense, rdy, atol=2e-5, rtol=0)
    if not train:
        assert np.array_equal(dense == 0, rdy == 0)
    assert_grads(o[f"dgamma{Lo}"], o[f"dbeta{Lo}"], reference(L, oracle, case, ("sums", gap, S)), R.split_counts(N, S) * Lp)


# ---------------------------------------------------------------------------------------------------------------------
# unfused backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("case", T.CASES, ids=_ids)
def test_unfused_backward(L, oracle, case, train):
    """ecg_bn_bwd against tests/bn_ref.py."""
    name, (N, C, Lo), (S, _, _, _), _ = case
    c = operands(case)
    _, mean0, inv0 = device_stats(L, case)
    n_ws = L.query("ecg_bn_bwd_ws_floats", N, C, Lo)

    def body(ar):
        y, dout, gamma = ar.put(c["y"]), ar.put(c["dout"]), ar.put(c["gamma"], 4)
        mean, inv = ar.put(mean0, 4), ar.put(inv0, 4)
        dy, dga, dbe, ws = ar.out((N, C, Lo)), ar.out((C,), 4), ar.out((C,), 4), ar.scratch(n_ws)
        L.call("ecg_bn_bwd", _ptr(y), _ptr(dout), _ptr(gamma), _ptr(mean), _ptr(inv), _ptr(dy), _ptr(dga), _ptr(dbe), _ptr(ws),
               N, C, Lo, train, L.stream())
        return {"dy": dy, "dgamma": dga, "dbeta": dbe}
    o = run_guarded(body)
    rdy, _, _ = R.bn_bwd(c["y"], c["dout"], c["gamma"], mean0, inv0, bool(train))
    print(f"dY: max err {np.abs(o['dy'] - rdy).max():.3e}")
    np.testing.assert_allclose(o["dy"], rdy, atol=2e-5, rtol=0)
    assert_grads(o["dgamma"], o["dbeta"], R.grad_split_sums(c["y"], c["dout"], mean0, inv0, S), R.split_counts(N, S) * Lo)


# ---------------------------------------------------------------------------------------------------------------------
# bf16 rows: strides rounded up to 8, garbage in the row pads, values pre-rounded to bf16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES_H, ids=_ids)
def test_bf16_forward(L, oracle, case):
    """ecg_bn_stats_relu_pool_fwd_h: the oracle's pooled tensor rounded to bf16, exactly, over a zero pad;
    ecg_bn_stats_relu_pool_gap_fwd_yh: the average forward's bar."""
    name, (N, C, Lo), (S, _, _, Sg), _ = case
    Lp = Lo // 2
    ldy, ldp = T.up(Lo, 8), T.up(Lp, 8)
    c = operands(case)
    part0, mean0, inv0 = device_stats(L, case, h=True)
    state = []

    def body(ar):
        y = ar.put_rows(c["yh"], ldy, "free")
        part, gamma, beta = ar.put(part0, 8), ar.put(c["gamma"], 4), ar.put(c["beta"], 4)
        mean, inv, p = ar.out((C,), 4), ar.out((C,), 4), ar.out_rows((N, C, ldp), Lp, "zeroed")
        nbt, nbt2 = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
        rm, rv, rm2, rv2 = (torch.full((C,), v, device="cuda") for v in (0.0, 1.0, 0.0, 1.0))
        L.call("ecg_bn_stats_relu_pool_fwd_h", _ptr(part), S, N * Lo, _ptr(rm), _ptr(rv), _ptr(nbt), MOMENTUM, EPS, _ptr(y), ldy,
               _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv), _ptr(p), ldp, N, C, Lo, L.stream())
        mean2, inv2, g = ar.out((C,), 4), ar.out((C,), 4), ar.out((N, C), 4)
        L.call("ecg_bn_stats_relu_pool_gap_fwd_yh", _ptr(part), S, N * Lo, _ptr(rm2), _ptr(rv2), _ptr(nbt2), MOMENTUM, EPS, _ptr(y),
               ldy, _ptr(gamma), _ptr(beta), _ptr(mean2), _ptr(inv2), _ptr(g), N, C, Lo, L.stream())
        state.extend((nbt, nbt2))
        return {"p": p, "g": g, "mean": mean, "inv": inv, "mean2": mean2, "inv2": inv2}
    o = run_guarded(body)
    assert all(int(t.item()) == 1 for t in state), "the batch counter has more than one writer (or none)"
    for k in ("mean", "mean2"):
        assert np.array_equal(o[k], mean0), k
    for k in ("inv", "inv2"):
        assert np.array_equal(o[k], inv0), k
    rp = reference(L, oracle, case, "pooled", h=True)
    assert np.array_equal(o["p"][:, :, :Lp], bf16_round(rp))
    rg = rp.astype(np.float64).mean(axis=2)
    err, bound = np.abs(o["g"] - rg), R.gap_row_bound(Lp, rg)
    print(f"g: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["dp_bf16", "dg_f32", "dp_f32"])
@pytest.mark.parametrize("case", CASES_H, ids=_ids)
def test_bf16_backward(L, oracle, case, kind, train):
    """ecg_bn_relu_pool_bwd_h, all three dp kinds: dY within half a bf16 ulp on top of the fp32 bar, zero pad, dgamma /
    dbeta at the fp32 passes' bars with Sw splits."""
    name, (N, C, Lo), (_, Sw, _, _), _ = case
    Lp = Lo // 2
    ldy, ldp = T.up(Lo, 8), T.up(Lp, 8)
    c = operands(case)
    _, mean0, inv0 = device_stats(L, case, h=True)
    n_ws = L.query("ecg_bn_relu_pool_bwd_ws_floats", N, C, Lo)
    assert n_ws == C * Sw * 2 + C * 2

    def body(ar):
        y = ar.put_rows(c["yh"], ldy, "free")
        if kind == 0:
            dp, ld = ar.put_rows(c["dph"], ldp, "free", 8), ldp
        elif kind == 1:
            dp, ld = ar.put(c["dg"], 4), 0
        else:
            dp, ld = ar.put_f32_rows(c["dph"], ldp, 4), ldp
        gamma, beta, mean, inv = ar.put(c["gamma"], 4), ar.put(c["beta"], 4), ar.put(mean0, 4), ar.put(inv0, 4)
        dy = ar.out_rows((N, C, ldy), Lo, "zeroed")
        dga, dbe, ws = ar.out((C,), 4), ar.out((C,), 4), ar.scratch(n_ws)
        L.call("ecg_bn_relu_pool_bwd_h", _ptr(y), ldy, _ptr(dp), kind, ld, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv),
               _ptr(dy), ldy, _ptr(dga), _ptr(dbe), _ptr(ws), N, C, Lo, train, L.stream())
        return {"dy": dy, "dgamma": dga, "dbeta": dbe}
    o = run_guarded(body)
    gap = kind == 1
    rdy, _, _ = reference(L, oracle, case, ("fused", gap, train), h=True)
    got = o["dy"][:, :, :Lo]
    err, bound = np.abs(got - rdy), 2.0 ** -8 * np.abs(rdy) + 2e-5
    print(f"dY: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # the fp32 passes' bar, count = the pairs of the split.  (A thread of the bf16 reduce adds the four pairs of a chunk, so
    # its longest chain is 4 ceil(chunks / 256) terms, up to 3 more than ceil(pairs / 256): the bound's first-order worst
    # case would need every rounding of one sign; it is held as the fp32 passes' and has not been widened.)
    assert_grads(o["dgamma"], o["dbeta"], reference(L, oracle, case, ("sums", gap, Sw), h=True), R.split_counts(N, Sw) * Lp)
