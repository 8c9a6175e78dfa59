"""The fused tail (csrc/tail_fused.hip: ecg_tail_fwd, ecg_tail_bwd_chain, ecg_linear_wgrad_grouped, ecg_transpose) at widths
other than the model defaults, against the float64 composition of tests/tail_ref.py; then the models that reach those
kernels with non-default widths, against oracle/ref_models.py on the CPU.

Tolerance of the kernel tests, per output:
    rel_rms(hip, f64) <= k * rel_rms(cpu fp32, f64) + 2^-22       max|hip - f64| <= k * max|cpu fp32 - f64| + 2^-22 * max|f64|
with k = 8 (32 at the 4 096-term chains of the LDS-limit case).  k does not grade rounding quality — the convolution tests do
that on the hot path — it separates rounding from indexing: the kernels sum in one serial fp32 fma chain of up to 512 terms
where the CPU sums in blocks (2.8-3.9x was measured for such chains of 3 840 terms in the convolutions), and a reduction
that loses one term sits above 3e4x (tests/test_tail_ref_host.py runs that stand-in on the CPU for every case).  The floor
covers outputs the CPU computes exactly (the 1-wide case)."""
import copy
import functools

import numpy as np
import pytest
import torch

import tail_ref as TR
from oracle import ref_models as R
from util import assert_grads_match_a_cpu_run

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib, functional
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return functional


# ---------------------------------------------------------------------------------------------------------------------
# 1. the three kernels through TailFn against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_runs(idx, demo, use_dz):
    """(float64 run, fp32 run) of one case on the CPU: computed once, shared by the forms that need it, never modified."""
    case, seed = (TR.LIMIT_CASE, TR.LIMIT_SEED) if idx < 0 else (TR.CASES[idx], TR.seed_of(idx))
    ops = TR.operands(case, seed)
    return ops, TR.run(ops, torch.float64, demo, use_dz), TR.run(ops, torch.float32, demo, use_dz)


def _hip_tail(hip, ops, demo, use_dz, xd_grad):
    """TailFn forward and backward on the device -> {"logits", "z", gradient of every operand that received one}."""
    t = {k: v.to(DEV).requires_grad_(k not in ("dlogits", "dz_extra") and (k != "xd" or xd_grad)) for k, v in ops.items()}
    if demo:
        logits, z = hip.TailFn.apply(t["g"], t["xd"], *[t[k] for k in TR.PARAMS])
    else:
        logits, z = hip.TailFn.apply(t["g"], None, t["Wp"], t["bp"], None, None, None, None, None, None, t["Wh"], t["bh"])
    if use_dz:
        torch.autograd.backward([logits, z], [t["dlogits"], t["dz_extra"]])
    else:
        logits.backward(t["dlogits"])
    got = {"logits": logits, "z": z}
    got.update({k: t[k].grad for k in ("g", "xd") + TR.PARAMS if k in t and t[k].grad is not None})
    return {k: v.detach().cpu().double().numpy() for k, v in got.items()}


def _compare(what, got, r32, r64, k):
    want = {n for n in r64 if n not in ("relu_margin", "last_unit_live")}
    assert set(got) == want, (what, sorted(set(got) ^ want))       # a gradient nobody asked for stays None, and the others exist
    failed = []
    for name in sorted(want):
        assert got[name].shape == r64[name].shape and np.isfinite(got[name]).all(), (what, name)
        m = TR.measure(got[name], r32[name], r64[name], k)
        TR.report(what, name, m)
        if not m["ok"]:
            failed.append((name, m))
    assert not failed, (what, failed)


@pytest.mark.parametrize("form", TR.FORMS, ids=[f[0] for f in TR.FORMS])
@pytest.mark.parametrize("idx", range(len(TR.CASES)), ids=[f"case{i}" for i in range(len(TR.CASES))])
def test_tail_kernels_vs_float64_at_untested_widths(hip, idx, form):
    """logits, z and every gradient of TailFn at the seven shapes of tail_ref.CASES (each the smallest that reaches a loop of
    the kernels no default-width test reaches), with and without demographics, the extra d z and the x_demo gradient.

    Largest measured ratio rel_rms(hip, f64) / rel_rms(cpu fp32, f64) over all cases and forms, per output family (MI355X;
    in brackets the largest rel-RMS error of the CPU fp32 run in that family, which the ratios are measured against):
        forward outputs    logits 2.09, z 2.02                                    (CPU fp32 3.2e-7, 2.2e-7)
        input gradients    g 1.59, xd 1.78                                        (CPU fp32 3.1e-7, 4.5e-7)
        weight gradients   Wp 1.21, W0 1.70, W2 1.77, Wf 1.75, Wh 1.85            (CPU fp32 at most 5.6e-7)
        bias gradients     bp 1.40, b0 3.67, b2 2.02, bf 1.90, bh 1.09            (CPU fp32 at most 5.5e-7)
    The largest, b0 at case 1, is a sum of M = 3 terms of a 7-wide layer: 5.8e-7 against 1.6e-7, three fp32 roundings
    against one.  Largest ratio of the maximum errors: 3.63 (the same output).  Nothing comes near k = 8."""
    name, demo, use_dz, xd_grad = form
    ops, r64, r32 = _cpu_runs(idx, demo, use_dz)
    if demo and not xd_grad:
        r64, r32 = ({k: v for k, v in r.items() if k != "xd"} for r in (r64, r32))
    got = _hip_tail(hip, ops, demo, use_dz, xd_grad)
    _compare(f"case {idx} {TR.CASES[idx]} {name}", got, r32, r64, TR.K_TOL)


def test_tail_kernels_at_the_lds_limit(hip):
    """Without demographics (2, 4096, 2048, C = 1024) needs 48 KB of LDS forward and 56 KB backward: the widest shape the
    ABI accepts runs and matches, with k = 32 for its 4 096-term chains (the expected error grows with sqrt(n)).
    Measured ratios (MI355X): z 2.08 (CPU fp32 rel-RMS 5.5e-7), Wh 2.07 (5.5e-7: it multiplies z), logits 1.72 (6.9e-7),
    g, Wp, bp, bh 1.00 (9.9e-7, 5.6e-7, 5.7e-7, 2.7e-8); of the maximum errors at most 3.13 (Wh)."""
    ops, r64, r32 = _cpu_runs(-1, False, True)
    got = _hip_tail(hip, ops, False, True, False)
    _compare(f"limit case {TR.LIMIT_CASE}", got, r32, r64, TR.K_TOL_LIMIT)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _zeros(*shape):
    return torch.zeros(*shape, device=DEV)


def _raw_tail_calls(dims, demo):
    """Both tail launches straight through the ABI with operands of exactly the stated sizes and NaN-filled outputs.
    -> [(entry point, return code, ecg_last_error(), outputs)]"""
    from ecg_hip import _lib as L
    M, F0, F, D, H1, H, C = dims
    lib, f32 = L.load(), L.f32
    d = (lambda *s: _zeros(*s)) if demo else (lambda *s: None)
    dn = (lambda *s: _nan(*s)) if demo else (lambda *s: None)
    res = []
    ins = [_zeros(M, F0), d(M, D), _zeros(F0, F), _zeros(F), d(H1, D), d(H1), d(H, H1), d(H), d(H, 2 * F), d(2 * F),
           _zeros(C, F), _zeros(C)]
    outs = [_nan(M, F), dn(M, H1), dn(M, H), dn(M, 2 * F), dn(M, F), _nan(M, C)]
    rc = lib.ecg_tail_fwd(*[f32(t) for t in ins + outs], M, F0, F, D, H1, H, C, L.stream())
    res.append(("ecg_tail_fwd", rc, L.last_error(), outs))
    ins = [_zeros(M, C), None, d(M, F), d(M, H1), d(M, H), d(M, 2 * F), _zeros(F, F0), d(H1, D), d(H, H1), d(2 * F, H),
           _zeros(C, F)]
    outs = [dn(M, F), _nan(M, F), dn(M, 2 * F), dn(M, H), dn(M, H1), _nan(M, F0), dn(M, D)]
    rc = lib.ecg_tail_bwd_chain(*[f32(t) for t in ins + outs], M, F0, F, D, H1, H, C, int(demo), L.stream())
    res.append(("ecg_tail_bwd_chain", rc, L.last_error(), outs))
    return res


# (dims, demographics, what ecg_last_error must name for the forward / the backward launch)
REFUSED = [((2, 4097, 8, 0, 0, 0, 2), False, ("F0=4097", "F0=4097")),
           ((2, 8, 2049, 0, 0, 0, 2), False, (" F=2049", " F=2049")),
           ((2, 8, 8, 0, 0, 0, 1025), False, ("C=1025", "C=1025")),
           # 8 448 floats per sample forward (F0 + D + H1 + H + F), 8 193 backward (C + 3 F + H + H1): more than 8 192
           ((2, 4096, 2048, 256, 1024, 1024, 1), True, ("67584 bytes of LDS", "65544 bytes of LDS"))]


@pytest.mark.parametrize("dims,demo,needles", REFUSED, ids=["F0=4097", "F=2049", "C=1025", "demo-over-64KB"])
def test_tail_refuses_widths_beyond_the_abi_and_the_lds_guard(hip, dims, demo, needles):
    for (entry, rc, msg, outs), needle in zip(_raw_tail_calls(dims, demo), needles):
        assert rc != 0, f"{entry} accepted {dims}"
        assert needle in msg and ("too wide" in msg or "bytes of LDS" in msg), (entry, msg)
        torch.cuda.synchronize()
        for t in outs:
            assert t is None or bool(torch.isnan(t).all()), f"{entry} wrote an output although it refused {dims}"


# ---------------------------------------------------------------------------------------------------------------------
# the grouped weight gradient on its own, through the ABI
# ---------------------------------------------------------------------------------------------------------------------
# (Out, In, with db): eight different pairs from {1, 5, 31, 32, 33, 64, 65, 257}^2, tiles ragged on neither, one or both sides
WG_PROBS = [(1, 257, True), (5, 65, False), (31, 33, True), (32, 31, True), (33, 5, False), (64, 1, True), (65, 64, True),
            (257, 32, True)]
WG_M = [1, 2, 3, 33, 130, 257]


def _wgrad_call(probs, G, X, M, count=None):
    """-> (return code, message, dW list, db list): outputs NaN-filled; a db the problem does not ask for is passed as NULL."""
    from ecg_hip import _lib as L
    dW = [_nan(o, i) for o, i, _ in probs]
    db = [_nan(o) for o, _, _ in probs]
    rc = L.load().ecg_linear_wgrad_grouped(
        L.ptr_table(G), L.ptr_table(X), L.ptr_table(dW), L.ptr_table([b if p[2] else None for b, p in zip(db, probs)]),
        L.int_table([p[0] for p in probs]), L.int_table([p[1] for p in probs]), len(probs) if count is None else count, M,
        L.stream())
    return rc, L.last_error(), dW, db


@pytest.mark.parametrize("M", WG_M)
@pytest.mark.parametrize("count", [1, 8])
def test_grouped_weight_gradient_vs_float64(hip, count, M):
    """dW_p = G_p^T X_p and db_p = sum_m G_p over count 1 and kMaxProb = 8 problems of different ragged shapes, some without
    db, at sample counts that leave waves empty (M <= 6), short (M = 33, 130) and ragged inside a 16-step batch (M = 130:
    17 steps per wave; M = 257: 129 steps).  Same tolerance rule as the tail; and the reduction order is fixed, so a second
    call gives the same bits.  Largest measured ratios (MI355X): dW 1.14 (CPU fp32 rel-RMS at most 2.8e-7), db 1.90
    (1.3e-7); of the maximum errors 2.23."""
    probs = WG_PROBS if count == 8 else [WG_PROBS[WG_M.index(M) + 1]]
    gen = torch.Generator().manual_seed(1000 * count + M)
    Gh = [torch.randn(M, o, generator=gen) for o, _, _ in probs]
    Xh = [torch.randn(M, i, generator=gen) for _, i, _ in probs]
    G, X = [t.to(DEV) for t in Gh], [t.to(DEV) for t in Xh]
    rc, msg, dW, db = _wgrad_call(probs, G, X, M)
    assert rc == 0, msg
    rc, msg, dW2, db2 = _wgrad_call(probs, G, X, M)
    assert rc == 0, msg
    failed = []
    for q, (o, i, with_db) in enumerate(probs):
        r64 = {"dW": (Gh[q].double().t() @ Xh[q].double()).numpy(), "db": Gh[q].double().sum(0).numpy()}
        r32 = {"dW": (Gh[q].t() @ Xh[q]).double().numpy(), "db": Gh[q].sum(0).double().numpy()}
        assert torch.equal(dW[q], dW2[q]), (q, "dW differs between two calls")
        if not with_db:
            assert bool(torch.isnan(db[q]).all()), (q, "a db that was not asked for was written")
        else:
            assert torch.equal(db[q], db2[q]), (q, "db differs between two calls")
        for name, t in (("dW", dW[q]), ("db", db[q])) if with_db else (("dW", dW[q]),):
            got = t.cpu().double().numpy()
            assert np.isfinite(got).all(), (q, name)
            m = TR.measure(got, r32[name], r64[name], TR.K_TOL)
            TR.report(f"wgrad count {count} M {M} problem {q} ({o} x {i})", name, m)
            if not m["ok"]:
                failed.append((q, name, m))
    assert not failed, failed


@pytest.mark.parametrize("count", [0, 9])
def test_grouped_weight_gradient_refuses_a_count_outside_1_to_8(hip, count):
    probs = WG_PROBS + [(5, 5, True)]                   # nine well-formed problems behind the tables, whatever `count` says
    G = [_zeros(3, o) for o, _, _ in probs]
    X = [_zeros(3, i) for _, i, _ in probs]
    rc, msg, dW, db = _wgrad_call(probs, G, X, 3, count=count)
    assert rc != 0 and f"count={count}" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in dW + db)


# ---------------------------------------------------------------------------------------------------------------------
# the transposes
# ---------------------------------------------------------------------------------------------------------------------
def test_transpose_is_exact_at_ragged_shapes(hip):
    from ecg_hip import _lib as L
    gen = torch.Generator().manual_seed(5)
    for rows in (1, 31, 33, 257):
        for cols in (1, 32, 65, 300):
            w = torch.randn(rows, cols, generator=gen).to(DEV)
            wT = _nan(cols, rows)
            L.call("ecg_transpose", L.f32(w), L.f32(wT), rows, cols, L.stream())
            assert torch.equal(wT, w.t().contiguous()), (rows, cols)


@pytest.mark.parametrize("demo", [True, False])
def test_tail_with_packed_transposes_gives_the_bits_of_its_own(hip, demo):
    """TailFn makes the two transposed weights itself (ecg_transpose) unless a WeightPacker hands them in (the grouped pack
    launch): both ways give the same bits, at a shape whose every transpose tile is ragged."""
    idx = 4
    M, F0, F, D, H1, H, C = TR.CASES[idx]
    ops = TR.operands(TR.CASES[idx], TR.seed_of(idx))

    def lin(w, b):
        m = torch.nn.Linear(ops[w].shape[1], ops[w].shape[0])
        with torch.no_grad():
            m.weight.copy_(ops[w]), m.bias.copy_(ops[b])
        return m.to(DEV)
    proj, head = lin("Wp", "bp"), lin("Wh", "bh")
    mlp0, mlp2, film_gen = (lin("W0", "b0"), lin("W2", "b2"), lin("Wf", "bf")) if demo else (None, None, None)
    conv = torch.nn.Conv1d(7, 5, 3, padding=1).to(DEV)
    _, trans = hip.WeightPacker().pack([conv], [proj, film_gen] if demo else [proj], need_bwd=True)
    assert torch.equal(trans[0], proj.weight.detach().t().contiguous())
    mods = [m for m in (proj, head, mlp0, mlp2, film_gen) if m is not None]

    def run(transposed):
        for m in mods:
            m.zero_grad()
        g = ops["g"].to(DEV).requires_grad_(True)
        xd = ops["xd"].to(DEV).requires_grad_(True) if demo else None
        logits, z = hip.tail(g, xd, proj, head, mlp0, mlp2, film_gen, transposed=transposed)
        torch.autograd.backward([logits, z], [ops["dlogits"].to(DEV), ops["dz_extra"].to(DEV)])
        out = [logits.detach(), z.detach(), g.grad] + ([xd.grad] if demo else [])
        return out + [p.grad.clone() for m in mods for p in m.parameters()]
    for a, b in zip(run(None), run(trans)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the models at non-default widths
# ---------------------------------------------------------------------------------------------------------------------
def _model_table():
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    return {"cnn384x71": (ECGCNN, R.RefECGCNN, dict(feat_dim=384, num_labels=71), 0),
            "cnn40x3": (ECGCNN, R.RefECGCNN, dict(feat_dim=40), 0),
            "mm384x23": (ECGMultimodal, R.RefECGMultimodal, dict(feat_dim=384, demo_dim=3, num_labels=23, demo_hidden_dim=48), 3),
            "mm128x5": (ECGMultimodal, R.RefECGMultimodal, dict(ecg_feat_dim=128, demo_hidden_dim=32), 5)}


MODEL_NAMES = ["cnn384x71", "cnn40x3", "mm384x23", "mm128x5"]
B, T = 3, 64            # the smallest window the suite uses; the tail does not see T


@functools.lru_cache(maxsize=None)
def _cpu_model_run(name):
    """The reference model of `name` run once on the CPU in fp32 and float64: one BCE backward in train mode, then an eval
    forward.  Shared by every route; nothing in it is modified afterwards."""
    _, rctor, kw, D = _model_table()[name]
    R.seed_all(7)
    ref = rctor(**kw)
    sd0 = copy.deepcopy(ref.state_dict())
    ref64 = copy.deepcopy(ref).double()
    C = ref.head.out_features
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, 12, T, generator=gen)
    y = (torch.rand(B, C, generator=gen) < 0.3).float()
    inp = (x, torch.rand(B, D, generator=gen)) if D else (x,)
    out = dict(sd0=sd0, ref=ref, ref64=ref64, inp=inp, y=y, C=C)
    ref.train(), ref64.train()
    logits = ref(*inp)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    torch.nn.functional.binary_cross_entropy_with_logits(ref64(*[t.double() for t in inp]), y.double()).backward()
    out.update(train_logits=logits.detach().numpy(), train_loss=loss.item())
    ref.eval()
    with torch.no_grad():
        if D:
            out.update(eval_logits=ref(*inp).numpy(), eval_z=None)
        else:
            lg, z = ref(*inp, return_features=True)
            out.update(eval_logits=lg.numpy(), eval_z=z.numpy())
    return out


def _device_model(name, sd):
    ctor, _, kw, _ = _model_table()[name]
    m = ctor(**kw)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _hook_for(model, route):
    """The hook that sends a model down `route`; None for the fully fused one."""
    bb = model.ecg_backbone if hasattr(model, "ecg_backbone") else model
    if route == "tail":                     # a hooked backbone block: leaves the fused chain, keeps the fused tail
        return bb.backbone[0].register_forward_hook(lambda m, i, o: None)
    if route == "leaves":                   # a hook on proj: every layer of the tail runs as its own leaf
        return bb.proj.register_forward_hook(lambda m, i, o: None)
    return None


@pytest.mark.parametrize("route", ["fused", "tail", "leaves"])
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_models_at_non_default_widths_vs_cpu_reference(hip, name, route):
    """ECGCNN / ECGMultimodal with the widths a user of the reference changes first, through the three routes the code has:
    loss and every parameter gradient after one BCE backward in train mode, logits (and ECGCNN's features) in eval mode,
    at the tolerances of test_ragged_batches_and_lengths_vs_cpu_oracle."""
    from ecg_hip import _lib
    c = _cpu_model_run(name)
    model = _device_model(name, c["sd0"])
    handle = _hook_for(model, route)
    inp, y = [t.to(DEV) for t in c["inp"]], c["y"].to(DEV)
    model.train()
    logits = model(*inp)
    loss = hip.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), c["train_logits"], atol=1e-4)
    assert abs(loss.item() - c["train_loss"]) < 1e-5, (loss.item(), c["train_loss"])
    assert_grads_match_a_cpu_run(
        {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}, c["ref"], c["ref64"],
        lambda k, g: 1e-6 if ".net.0.bias" in k else 1e-4 * max(1.0, float(np.abs(g).max())), what=f"{name} {route}")
    model.eval()
    with torch.no_grad(), _lib.kernel_timing() as kt:
        out = model(*inp) if c["eval_z"] is None else model(*inp, return_features=True)
    names = {k[0] for k in kt.result}
    if route == "leaves":
        assert "ecg_linear_fwd" in names and "ecg_tail_fwd" not in names, names
    else:
        assert "ecg_tail_fwd" in names and "ecg_linear_fwd" not in names, names
        # the fused route gets its transposes from the grouped pack launch, the other from ecg_transpose
        assert ("ecg_transpose" in names) == (route == "tail"), names
    if c["eval_z"] is None:
        np.testing.assert_allclose(out.cpu().numpy(), c["eval_logits"], atol=1e-4)
    else:
        np.testing.assert_allclose(out[0].cpu().numpy(), c["eval_logits"], atol=1e-4)
        np.testing.assert_allclose(out[1].cpu().numpy(), c["eval_z"], atol=1e-4)
    if handle is not None:
        handle.remove()


def test_flat_adamw_step_on_a_parameter_count_that_is_no_multiple_of_4(hip):
    """ECGCNN(feat_dim=384, num_labels=71) has 778 343 parameters (n % 4 = 3).  One FlatAdamW step against torch.optim.AdamW
    on the reference model GIVEN THE SAME GRADIENTS, at the tolerance of test_adamw_flat_step_vs_oracle_and_torch: AdamW
    divides every gradient by its own magnitude, so the gradients themselves are compared where they are computed (above)."""
    from ecg_hip.optim import FlatAdamW
    name = "cnn384x71"
    c = _cpu_model_run(name)
    model = _device_model(name, c["sd0"]).train()
    assert sum(p.numel() for p in model.parameters()) == 778343
    opt = FlatAdamW(model.parameters(), lr=1.5e-3, weight_decay=1e-4)
    opt.zero_grad()
    hip.binary_cross_entropy_with_logits(model(c["inp"][0].to(DEV)), c["y"].to(DEV)).backward()
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    opt.step()
    ref = _model_table()[name][1](**_model_table()[name][2])
    ref.load_state_dict(c["sd0"])
    ropt = torch.optim.AdamW(ref.parameters(), lr=1.5e-3, weight_decay=1e-4)
    for k, p in ref.named_parameters():
        p.grad = grads[k]
    ropt.step()
    for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().numpy(), atol=2e-7, rtol=2e-6, err_msg=k)
        assert not torch.equal(q.detach(), c["sd0"][k]), k         # the step moved it


@pytest.mark.parametrize("name", ["cnn384x71", "mm384x23"])
def test_bf16_inference_logits_of_the_384_wide_models(hip, name):
    """inference_precision("bf16") against the fp32 logits of the same model, within the 1.5e-2 the README states."""
    c = _cpu_model_run(name)
    model = _device_model(name, c["sd0"]).eval()
    inp = [t.to(DEV) for t in c["inp"]]
    with torch.no_grad():
        fp32 = model(*inp)
        with hip.inference_precision("bf16"):
            bf16 = model(*inp)
    err = float((bf16 - fp32).abs().max())
    print(f"{name}: max|bf16 - fp32| logits = {err:.3e}")
    assert bf16.shape == fp32.shape == (B, c["C"]) and bool(torch.isfinite(bf16).all())
    assert err <= 1.5e-2, err
    assert not torch.equal(bf16, fp32)                  # the bf16 blocks ran: T = 64 is inside their envelope


@pytest.mark.parametrize("name", ["cnn384x71", "mm384x23"])
def test_grad_cam_on_the_71_and_23_label_models(hip, name):
    """ecg_hip.grad_cam, fused against the hook path, for class indices 0, last and -1, at the tolerance of
    test_fused_path_against_the_hook_path."""
    from ecg_hip.gradcam import grad_cam
    from test_gpu_gradcam import PARITY_BOUND
    c = _cpu_model_run(name)
    model = _device_model(name, c["sd0"]).eval()
    x = c["inp"][0].to(DEV)
    xd = c["inp"][1].to(DEV) if len(c["inp"]) > 1 else None
    bound = PARITY_BOUND["multimodal" if xd is not None else "baseline"]
    C = c["C"]
    for normalize in ("before", "after"):
        cams = {}
        for k in (0, C - 1, -1, [0, C - 1, -1]):
            fused, lf = grad_cam(model, x, xd, class_idx=k, signal_length=T, normalize=normalize, return_logits=True, fused=True)
            hook, lh = grad_cam(model, x, xd, class_idx=k, signal_length=T, normalize=normalize, return_logits=True, fused=False)
            d = float((fused - hook).abs().max())
            print(f"{name} class {k} {normalize}: max|fused - hook| = {d:.3e} (bound {bound:.3e})")
            assert fused.shape == hook.shape == ((B, 3, T) if isinstance(k, list) else (B, T))
            assert d <= bound, (k, normalize, d)
            assert float((lf - lh).abs().max()) <= 1e-4
            cams[str(k)] = (fused, hook)
        for i in (0, 1):                                            # -1 is the last class, on both paths
            assert torch.equal(cams["-1"][i], cams[str(C - 1)][i])
            assert torch.equal(cams[str([0, C - 1, -1])][i][:, 2], cams[str([0, C - 1, -1])][i][:, 1])
