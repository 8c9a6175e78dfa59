"""The mixed-precision training form (conv_precision("bf16"), ConvBlockFn._fwd_bf16 / _bwd_bf16) as the Python glue composes
it, pinned stage by stage: the backbone is driven block by block with conv_block_chain exactly as fused_forward drives it,
every block's own tensors are read back (p.grad_fn is the block's ctx: saved_tensors = x, w, y, gamma, beta, mean, invstd; a
tensor hook on p sees the gradient handed back), and each stage is compared with the float64 restatement of THAT stage on
THOSE tensors (tests/bf16_block_ref.py).  Decisions are taken from the device's own y, so nothing cascades and the bars are
fp32-level: every one is either fixed by the format / the kernel-level tests or is the fp32 stand-in's figure of
tests/test_bf16_block_ref_host.py times its stated margin — none was taken from a device run.  What each check pins of the
glue: DESIGN.md section 3, "Stage checks of the mixed-precision chain".  The measured device figure of every check is in the
assertion message (all: name figure/bar) and printed per block (pytest -s).  Largest device figure over every chain of this
file on an MI355X, beside its bar:
  y 0.992 / 1      p_ulp 1 / 1      p_neq 8.4e-5 / 1e-2      uncertain 9.6e-6 / 1e-2      x_rows, lin, nbt, p_pad, p_not_bf16 0 / 0
  mean 5.3e-8 / 3.1e-7      invstd 8.7e-8 / 6.4e-6      running_mean 2.1e-8 / 1.2e-7      running_var 5.5e-8 / 3.8e-7
  gap 2.2e-7 / 1.9e-6       dbeta 1.7e-7 / 3.0e-6       dgamma 1.8e-7 / 1.6e-6            db 1 / 4 (bf16 ulps of dY)
  dx 0.45 / 1.96 (dY flips beyond one bf16 ulp)         dx_neq 7.2e-3 / 0.1               dw 9.0e-5 / 5.2e-4"""
import pytest
import torch

import bf16_block_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, H = "ecg_conv1d_fwd", "ecg_conv1d_fwd_bf16_yh"
WG = {F32: "ecg_conv1d_bwd_weight_bias_ld", H: "ecg_conv1d_bwd_weight_bias_bf16_ncl"}


def _perturb(bns, seed):
    """BatchNorm parameters and running statistics off their defaults, so that a missed gamma / beta / update shows."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in bns:
            C = bn.num_features
            bn.weight.copy_(1.0 + 0.2 * torch.randn(C, generator=g)); bn.bias.copy_(0.1 * torch.randn(C, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(C, generator=g)); bn.running_var.copy_(1.0 + 0.5 * torch.rand(C, generator=g))
            bn.num_batches_tracked.fill_(3)


def _model(kind, seed=5):
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    from src.utils.seed import set_seed
    set_seed(seed)
    model = (ECGCNN(num_labels=5) if kind == "cnn" else ECGMultimodal()).to(DEV).train()
    blocks = list((model if kind == "cnn" else model.ecg_backbone).backbone)
    _perturb([b.net[1] for b in blocks], seed + 1)
    return model, [(b.net[0], b.net[1]) for b in blocks]


def _blocks(widths, seed=5):
    from src.models.ecg_cnn import ConvBlock
    from src.utils.seed import set_seed
    set_seed(seed)
    blocks = [ConvBlock(a, b).to(DEV).train() for a, b in zip(widths, widths[1:])]
    _perturb([b.net[1] for b in blocks], seed + 1)
    return [(b.net[0], b.net[1]) for b in blocks]


def _batch(N, Ci, T, seed, labels=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, T, generator=g) + 0.3 * torch.randn(N, Ci, 1, generator=g)
    return x, torch.randn(N, 5, generator=g), (torch.rand(N, labels, generator=g) > 0.5).float()


class Drive:
    """One forward of a chain of (conv, bn) blocks through conv_block_chain as fused_forward calls it (packed=None: every
    block packs its own operands), with a hook on every block output; then `finish(p_last)` -> scalar, and backward passes on
    demand.  The hooks capture the gradient each p receives and, while self.poison is set, REPLACE a bf16 gradient by a copy
    whose pad columns [Lo // 2, ldp) hold NaN (ecg_conv1d_bwd_data_bf16hh leaves that pad "alone or zeroed")."""

    def __init__(self, blocks, x, finish, gap_last=True):
        from ecg_hip import functional as F
        self.blocks, self.x, self.poison, self.cap, self.info = blocks, x, False, {}, []
        carry, h = None, x
        with F.conv_precision("bf16"):
            for i, (conv, bn) in enumerate(blocks):
                last = i == len(blocks) - 1
                before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
                nxt = (None, None) if last else blocks[i + 1]
                p, new = F.conv_block_chain(h, conv, bn, gap=last and gap_last, packed=None, carry=carry, next_conv=nxt[0],
                                            next_bn=nxt[1], next_gap=gap_last and i + 2 == len(blocks))
                ctx = p.grad_fn
                self.info.append(dict(ctx=ctx, mode=ctx.mode, fed=h, p=p, carry_in=carry, carry_out=new, before=before,
                                      after=(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)),
                                      saved=ctx.saved_tensors if ctx.mode == "bf16" else None))
                p.register_hook(self._hook(i, ctx.Lo // 2))
                carry, h = new, p
            self.out = finish(h)

    def _hook(self, i, Lp):
        def hook(g):
            if not self.poison:
                self.cap[i] = g.detach().clone()
            elif g.dtype == torch.bfloat16:
                g = g.clone()
                g[:, :, Lp:] = float("nan")
                return g
        return hook

    def params(self):
        return [q for conv, bn in self.blocks for q in (conv.weight, conv.bias, bn.weight, bn.bias)]

    def backward(self, poison=False, extra=()):
        """-> the gradients of every block parameter (+ `extra` tensors), cloned; the graph is kept."""
        from ecg_hip import functional as F
        ps = self.params() + list(extra)
        for q in ps:
            q.grad = None
        self.poison = poison
        with F.conv_precision("bf16"):
            self.out.backward(retain_graph=True)
        self.poison = False
        return [None if q.grad is None else q.grad.detach().clone() for q in ps]

    def records(self):
        """Per block the record bf16_block_ref.figures reads (host tensors, device dtypes), None for a block that is not bf16."""
        c = lambda t: None if t is None else t.detach().cpu()     # noqa: E731
        recs = []
        for i, (inf, (conv, bn)) in enumerate(zip(self.info, self.blocks)):
            if inf["mode"] != "bf16":
                recs.append(None)
                continue
            ctx = inf["ctx"]
            x, w, y, gamma, beta, mean, invstd = inf["saved"]
            handed = i > 0 and self.info[i - 1]["p"].dtype == torch.bfloat16        # the previous block's bf16 rows as they are
            if handed:      # same storage, or at least equal bits (figures compares the bits)
                assert x.data_ptr() == self.info[i - 1]["p"].data_ptr() or torch.equal(x, self.info[i - 1]["p"])
            dx = self.cap.get(i - 1) if i else self.x.grad
            recs.append(dict(
                Lin=ctx.Lin, Lo=ctx.Lo, pad=ctx.pad, gap=bool(ctx.gap), eps=bn.eps, momentum=bn.momentum, x=c(x),
                x_src=None if handed else c(inf["fed"]), w=c(w), b=c(conv.bias), gamma=c(gamma), beta=c(beta), y=c(y),
                mean=c(mean), invstd=c(invstd), rm0=c(inf["before"][0]), rv0=c(inf["before"][1]), nbt0=inf["before"][2],
                rm1=c(inf["after"][0]), rv1=c(inf["after"][1]), nbt1=inf["after"][2], p=c(inf["p"]), dp=c(self.cap.get(i)),
                dgamma=c(bn.weight.grad), dbeta=c(bn.bias.grad), dw=c(conv.weight.grad), db=c(conv.bias.grad), dx=c(dx),
                x_cast=ctx.x_cast, ldyh=ctx.ldyh, ldp=ctx.ldp))
        return recs


def _check_chain(drive, what, want_modes):
    """Every stage check on every bf16 block of a driven chain, after one clean backward pass."""
    modes = [inf["mode"] for inf in drive.info]
    assert modes == want_modes, (what, modes)
    recs = drive.records()
    for i, rec in enumerate(recs):
        inf = drive.info[i]
        if i:       # the carry: the true pooled length, exactly when bf16 rows are handed on
            prev = drive.info[i - 1]
            assert prev["carry_out"] == (prev["ctx"].Lo // 2 if prev["p"].dtype == torch.bfloat16 else None), (what, i)
            assert inf["ctx"].Lin == prev["ctx"].Lo // 2, (what, i)
        if rec is None:
            assert inf["fed"].dtype == torch.float32, (what, i)        # an fp32 block is fed fp32 rows
            continue
        x = rec["x"]
        # the glue's choices for this block: fp32 read in place only where the kernels can, bf16 strides multiples of 8
        if x.dtype == torch.float32:
            assert not rec["x_cast"] and rec["Lin"] % 8 == 0 and inf["fed"].data_ptr() % 16 == 0 and i == 0, (what, i)
        else:
            assert x.shape[2] == (rec["Lin"] + 7) & ~7 and rec["x_cast"] == (inf["fed"].dtype == torch.float32), (what, i)
        assert rec["ldyh"] == (rec["Lo"] + 7) & ~7 == rec["y"].shape[2], (what, i)
        if rec["p"].dtype == torch.bfloat16:
            assert rec["ldp"] == (rec["Lo"] // 2 + 7) & ~7 == rec["p"].shape[2] and recs[i + 1] is not None, (what, i)
            assert rec["dp"].dtype == torch.bfloat16 and rec["dp"].shape == rec["p"].shape, (what, i)
        else:
            assert rec["ldp"] == 0 and (rec["dp"] is None or rec["dp"].dtype == torch.float32), (what, i)
        prev = recs[i - 1] if i and recs[i - 1] is not None else (dict(p=drive.info[i - 1]["p"].detach().cpu(),
                                                                       Lo=drive.info[i - 1]["ctx"].Lo) if i else None)
        fig = R.figures(rec, prev)
        print(f"figures | {what} block {i} | " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))       # (pytest -s)
        assert fig["uncertain"] <= R.UNCERTAIN_CAP, (what, i, fig["uncertain"])
        R.assert_block(fig, f"{what} block {i}")
    return recs


def _same_bits(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None), (what, i)
        if u is not None:
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), f"{what}: gradient {i} differs, max {float((u - v).abs().max()):.3g}"


def _tail(model, kind, g, xd):
    from ecg_hip import functional as F
    if kind == "cnn":
        return F.tail(g, None, model.proj, model.head)[0]
    enc, bb = model.demo_encoder, model.ecg_backbone
    return F.tail(g, xd.to(DEV), bb.proj, model.head, enc.mlp[0], enc.mlp[2], model.film_gen)[0]


# rows of the four blocks, and what the case is for
T_CASES = {128: "128/64/32/16: all four blocks bf16 at the shortest rows the form takes",
           127: "../15: last block fp32 with the average; block 2 hands over fp32 rows and receives dp_kind 2",
           100: "100/50/25/12: the short-row defect; Lin % 8 != 0 on block 0: x_cast",
           136: "136/68/34/17", 250: "Lo = 125: odd rows, an unpooled tail", 258: "block 1 Lo = 129: ldt = 256 with 127 zero columns",
           1030: "rows past 1024"}


@pytest.mark.parametrize("N", [1, 3, 19])
@pytest.mark.parametrize("T", sorted(T_CASES))
def test_bf16_chain_stage_by_stage(T, N):
    """ECGCNN's backbone block by block, the fused tail, the BCE loss, one backward — every stage of every bf16 block against
    float64 on the device's own tensors (bars: bf16_block_ref.BARS; the device's figures are in the assertion message).  Then
    the backward again with every bf16 gradient's pad poisoned with NaN: every parameter gradient bit-identical.
    T = 100 is the case that raised EcgHipError("conv1d_bwd_weight_bias_bf16_ncl: N=.. L=12") in backward before block_form
    asked ecg_conv1d_bf16_tk_min_len (block 3, Lin = 12 < 16, took the bf16 forward)."""
    from ecg_hip import functional as F
    model, blocks = _model("cnn")
    x, _, y = _batch(N, 12, T, 100 + N + T)
    yd = y.to(DEV)
    drive = Drive(blocks, x.to(DEV), lambda g: F.binary_cross_entropy_with_logits(_tail(model, "cnn", g, None), yd))
    tail_params = [model.proj.weight, model.proj.bias, model.head.weight, model.head.bias]
    clean = drive.backward(extra=tail_params)
    _check_chain(drive, f"N={N} T={T}", ["bf16"] * 3 + ["bf16" if T >> 3 >= 16 else "fp32"])
    poisoned = drive.backward(poison=True, extra=tail_params)
    _same_bits(clean, poisoned, f"N={N} T={T} poisoned pad")
    assert all(torch.isfinite(g).all() for g in clean)


@pytest.mark.parametrize("kind,N,T", [("cnn", 3, 128), ("cnn", 3, 100), ("cnn", 19, 250), ("mm", 3, 258), ("mm", 1, 127)])
def test_model_forward_gives_the_bits_of_the_manual_drive(kind, N, T):
    """model(x) + loss + backward on a fresh, identically seeded model: the same logits, running statistics and gradient
    bits as the block-by-block drive with packed=None — WeightPacker's grouped pack (and its walk of the chain,
    _operand_kinds) against the per-block packs, the tail's transposed weights against its own."""
    from ecg_hip import functional as F
    x, xd, y = _batch(N, 12, T, 7 + N + T)
    m1, blocks = _model(kind)
    got = {}

    def finish(g):
        got["logits"] = _tail(m1, kind, g, xd)
        return F.binary_cross_entropy_with_logits(got["logits"], y.to(DEV))
    drive = Drive(blocks, x.to(DEV), finish)
    with F.conv_precision("bf16"):
        drive.out.backward()
    m2, _ = _model(kind)
    with F.conv_precision("bf16"):
        logits = m2(x.to(DEV)) if kind == "cnn" else m2(x.to(DEV), xd.to(DEV))
        F.binary_cross_entropy_with_logits(logits, y.to(DEV)).backward()
    assert torch.equal(logits, got["logits"]), float((logits - got["logits"]).abs().max())
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), f"{k}: max {float((a.grad - b.grad).abs().max()):.3g}"


@pytest.mark.parametrize("T,want", [(100, [H, H, H, F32]), (128, [H, H, H, H]), (127, [H, H, H, F32])])
def test_short_rows_take_the_fp32_form_and_the_step_completes(T, want, monkeypatch):
    """ECGCNN at T = 100 under conv_precision("bf16"): block 3 has Lin = 12, below the time-on-K weight gradient's bound, and
    runs the fp32 kernels forward AND backward (before: bf16 forward, then EcgHipError from
    ecg_conv1d_bwd_weight_bias_bf16_ncl in backward).  Entry points spied as in test_bf16_mode_runs_the_fp32_kernels_..."""
    from ecg_hip import _lib, functional as F
    model, _ = _model("cnn")
    x, _, y = _batch(6, 12, T, 3)
    names, raw = [], _lib.call

    def spy(name, *args):
        names.append(name)
        raw(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    monkeypatch.setattr(F, "_call", spy)
    with F.conv_precision("bf16"):
        F.binary_cross_entropy_with_logits(model(x.to(DEV)), y.to(DEV)).backward()
    monkeypatch.undo()
    assert [n for n in names if n in (F32, H)] == want, names
    assert [n for n in names if n in WG.values()] == [WG[f] for f in reversed(want)], names
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


# ---- chains built by hand ---------------------------------------------------------------------------------------------------
def _cot(p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(p.shape, generator=g) / p.shape[0]).to(DEV)


def test_input_gradient_through_x_cast_on_a_32_channel_input():
    """32 -> 64 -> 128 with x.requires_grad_(): block 0 owes an input gradient, so it reads an x_cast copy (bf16 rows of the
    fp32 input) and its dx, bf16 rows, is widened back to fp32 [N][32][Lin]; x.grad against the restatement.  The last block
    has no average: its p is fp32 rows and its gradient arrives as fp32 rows (dp_kind 2)."""
    blocks = _blocks((32, 64, 128))
    x = _batch(3, 32, 100, 21)[0].to(DEV).requires_grad_(True)
    drive = Drive(blocks, x, lambda p: (p * _cot(p, 4)).sum(), gap_last=False)
    clean = drive.backward(extra=[x])
    recs = _check_chain(drive, "input gradient", ["bf16", "bf16"])
    assert recs[0]["x_cast"] and x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    assert torch.equal(x.grad, x.grad.to(torch.bfloat16).float())          # widened bf16 rows
    _same_bits(clean, drive.backward(poison=True, extra=[x]), "input gradient, poisoned pad")


def test_unaligned_input_view_values():
    """The `unaligned` view of test_bf16_mode_runs_the_fp32_kernels_wherever_the_mixed_form_does_not_apply (4 bytes into a
    buffer: contiguous, not 16-byte aligned), now with values: block 0 must take the x_cast copy although Lin % 8 == 0."""
    blocks = _blocks((12, 32, 64))
    x0 = _batch(3, 12, 128, 22)[0].to(DEV)
    buf = torch.empty(x0.numel() + 1, device=DEV)
    buf[1:].copy_(x0.reshape(-1))
    x = buf[1:].view_as(x0)
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    drive = Drive(blocks, x, lambda g: (g * _cot(g, 5)).sum())
    clean = drive.backward()
    recs = _check_chain(drive, "unaligned", ["bf16", "bf16"])
    assert recs[0]["x_cast"]
    _same_bits(clean, drive.backward(poison=True), "unaligned, poisoned pad")


def test_frozen_batchnorm_between_two_bf16_blocks():
    """Block 1's BatchNorm frozen in a 3-block chain: bf16 -> fp32 -> bf16 with fp32 tensors across both joints — block 0
    hands over fp32 rows holding bf16 numbers and receives fp32 rows (dp_kind 2); block 2 casts the fp32 activation (x_cast)
    and widens its dx for the fp32 block."""
    blocks = _blocks((12, 32, 64, 128))
    blocks[1][1].eval()
    x = _batch(3, 12, 136, 23)[0].to(DEV)
    drive = Drive(blocks, x, lambda g: (g * _cot(g, 6)).sum())
    drive.backward()
    recs = _check_chain(drive, "frozen", ["bf16", "fp32", "bf16"])
    assert recs[2]["x_cast"] and recs[2]["dx"].dtype == torch.float32 and recs[0]["dp"].dtype == torch.float32
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in drive.params())


def test_output_width_96():
    """12 -> 96 -> 64: an output width that is a multiple of 32 but not of 64 (the 32-row tiles of the weight gradient and of
    the forward), and 96 input channels on the second block's input gradient."""
    blocks = _blocks((12, 96, 64))
    x = _batch(3, 12, 250, 24)[0].to(DEV)
    drive = Drive(blocks, x, lambda g: (g * _cot(g, 7)).sum())
    clean = drive.backward()
    _check_chain(drive, "width 96", ["bf16", "bf16"])
    _same_bits(clean, drive.backward(poison=True), "width 96, poisoned pad")


class _TakeLast(torch.autograd.Function):
    """(a, b, c) -> c; hands None back for a and b, so their producers run backward with an UNDEFINED gradient."""

    @staticmethod
    def forward(ctx, a, b, c):
        return c.view_as(c)

    @staticmethod
    def backward(ctx, g):
        return None, None, g


def test_unused_output_beside_a_used_one():
    """Three blocks on one bf16 activation; only the third one's p feeds the loss, the other two sit in the graph beside it
    and receive no gradient: the `dp is None` branch of _bwd_bf16 under set_materialize_grads(False), once for bf16 rows
    (a consumer was promised) and once for fp32 rows.  Their parameter gradients are exact zeros — not NaN, not stale memory
    — and the shared producer's gradients are those of the used branch alone."""
    from ecg_hip import functional as F
    first, a, b, c = _blocks((12, 32, 64)), _blocks((32, 64, 128), 8), _blocks((32, 64), 9), _blocks((32, 64), 10)
    x = _batch(3, 12, 136, 25)[0].to(DEV)

    def run(with_unused):
        for conv, bn in first + a[:1] + b + c:
            for q in (conv.weight, conv.bias, bn.weight, bn.bias):
                q.grad = None
        with F.conv_precision("bf16"):
            p0, carry = F.conv_block_chain(x, *first[0], next_conv=c[0][0], next_bn=c[0][1])
            assert p0.dtype == torch.bfloat16
            pc, _ = F.conv_block_chain(p0, *c[0], carry=carry)
            if with_unused:
                pa, ca = F.conv_block_chain(p0, *a[0], carry=carry, next_conv=a[1][0], next_bn=a[1][1])      # bf16 rows out
                pb, _ = F.conv_block_chain(p0, *b[0], carry=carry)                                           # fp32 rows out
                assert pa.dtype == torch.bfloat16 and ca == 34 and pb.dtype == torch.float32
                assert pa.grad_fn.mode == pb.grad_fn.mode == "bf16"
                pc = _TakeLast.apply(pa, pb, pc)
            (pc * _cot(pc, 11)).sum().backward()
        return [q.grad.clone() for conv, bn in first[:1] + c for q in (conv.weight, conv.bias, bn.weight, bn.bias)]
    used = run(True)
    for conv, bn in a[:1] + b:
        for q in (conv.weight, conv.bias, bn.weight, bn.bias):
            assert q.grad is not None and not q.grad.any(), "an unused block's gradient must be exactly zero"
    _same_bits(used, run(False), "beside unused outputs")
