"""The kernels that end every training step, through the C ABI, against the float64 restatements of tests/step_end_ref.py:
bce_kernel and sigmoid_kernel (csrc/tail.hip: ecg_bce_logits_fwd, ecg_sigmoid_fwd), adamw_kernel and adamw_graph_kernel
(csrc/optim.hip: ecg_adamw_step, ecg_adamw_step_graph), then FlatAdamW's host side (ecg_hip/optim.py) without a model.

The bounds are those of step_end_ref (at most eight float32 roundings per output, shown on the CPU to lie above float32 noise
and below a dropped element or a lost factor: tests/test_step_end_ref_host.py); they are not tuned to what the device gives.
Every output buffer is 64 elements longer than needed, from an aligned base, the slack holding 12345.0: it must survive each
call, and the inputs must keep their bits.  Each test prints the largest error it saw as a fraction of its bound.

Out of scope: non-finite logits (tests/test_gpu_values.py), |g gscale| < 1e-16 (see step_end_ref), stream capture."""
import numpy as np
import pytest
import torch

import step_end_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLACK, FILL = 64, 12345.0


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return _lib


def guarded(values=None, n=None, dtype=torch.float32):
    """-> (buffer of n + 64 elements whose slack holds 12345.0, its first n elements: what the kernel is handed)."""
    if values is not None:
        values = torch.from_numpy(np.ascontiguousarray(values))
        n, dtype = values.numel(), values.dtype
    buf = torch.full((n + SLACK,), FILL, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    if values is not None:
        buf[:n] = values.to(DEV)
    return buf, buf[:n]


def slack_intact(*bufs):
    return all(bool((b[-SLACK:] == FILL).all()) for b in bufs)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def host(t):
    return t.detach().cpu().numpy()


def ulps(a, b):
    """Largest |a - b| in units of the float32 spacing at b."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b)).astype(np.float64)
    return float(np.nanmax(np.where(a == b, 0.0, d))) if a.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# BCE with logits
# ---------------------------------------------------------------------------------------------------------------------
def _bce(L, x_d, t_d, n, with_dx=True, running=None, weight=1.0):
    """One ecg_bce_logits_fwd launch into fresh guarded buffers -> (loss buffer, dx buffer or None)."""
    loss_b, loss = guarded(n=1)
    dx_b, dx = guarded(n=n) if with_dx else (None, None)
    L.call("ecg_bce_logits_fwd", L.f32(x_d), L.f32(t_d), L.f32(loss), L.f32(dx), n, L.ptr(running), float(weight), L.stream())
    torch.cuda.synchronize()
    return loss_b, dx_b


@pytest.mark.parametrize("kind", SR.TARGET_KINDS)
@pytest.mark.parametrize("n", SR.NUMEL)
def test_bce_loss_and_gradient_vs_float64(L, n, kind):
    """One workgroup walks numel in strides of 2048: one trip (n <= 1024, 2048), a second half-trip (1025 ... 2047), a second
    trip with and without its second half (2049, 3072, 4097), nine trips with a partial last one (18 176 = 256 x 71)."""
    x, t = SR.logits(n, n), SR.targets(n, kind, n)
    x_d, t_d = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    loss_ref, dx_ref, _ = SR.bce(x, t)
    b_loss, b_dx = SR.bce_bounds(x, t)
    loss_b, dx_b = _bce(L, x_d, t_d, n)
    f_loss = abs(float(loss_b[0]) - loss_ref) / b_loss
    f_dx = SR.worst(host(dx_b[:n]), dx_ref, b_dx)
    print(f"bce n={n} {kind}: loss error {f_loss:.3f} of its bound, dx {f_dx:.3f}")
    assert f_loss <= 1.0, (float(loss_b[0]), loss_ref, b_loss)
    assert f_dx <= 1.0, f_dx
    assert slack_intact(loss_b, dx_b)
    loss2_b, dx2_b = _bce(L, x_d, t_d, n)                                # the sums are in a fixed order
    assert same_bits(loss2_b, loss_b) and same_bits(dx2_b, dx_b)
    loss3_b, _ = _bce(L, x_d, t_d, n, with_dx=False)                     # dx = NULL: the same loss, nothing else written
    assert same_bits(loss3_b, loss_b)
    assert same_bits(x_d, torch.from_numpy(x).to(DEV)) and same_bits(t_d, torch.from_numpy(t).to(DEV))


@pytest.mark.parametrize("n", SR.ONCE_NUMEL)
def test_bce_counts_every_element_exactly_once(L, n):
    """Every term 9.4e-14 but one of 20 at position k, k at each edge of the 1024-wide half-trips and at the end: the loss is
    20 / n within its bound (9 u relative); a dropped or doubled element would miss it by 1e-3 relative and more."""
    for k in SR.once_positions(n):
        x, t = SR.once_case(n, k)
        x_d, t_d = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
        loss_ref, dx_ref, _ = SR.bce(x, t)
        b_loss, b_dx = SR.bce_bounds(x, t)
        for with_dx in (True, False):
            loss_b, dx_b = _bce(L, x_d, t_d, n, with_dx=with_dx)
            got = float(loss_b[0])
            assert abs(got - 20.0 / n) <= b_loss and abs(got - loss_ref) <= b_loss, (n, k, with_dx, got, 20.0 / n, b_loss)
            assert slack_intact(loss_b)
            if with_dx:
                assert SR.worst(host(dx_b[:n]), dx_ref, b_dx) <= 1.0 and slack_intact(dx_b), (n, k)


def test_bce_running_sum_receives_loss_times_weight(L):
    """running += (double) loss * weight inside the launch: from 0.75, three calls with weights 1, 0.25 and 3 (products that
    are exact in double, fused or not) leave 0.75 + sum of double(loss_k) w_k within 2 ulp; its neighbour is not touched."""
    n = 4097
    running = torch.tensor([0.75, FILL], dtype=torch.float64, device=DEV)
    expected = np.float64(0.75)
    for i, w in enumerate((1.0, 0.25, 3.0)):
        x, t = SR.logits(n, 100 + i), SR.targets(n, "hard", 100 + i)
        loss_b, dx_b = _bce(L, torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), n, running=running, weight=w)
        assert abs(float(loss_b[0]) - SR.bce(x, t)[0]) <= SR.bce_bounds(x, t)[0] and slack_intact(loss_b, dx_b)
        expected = expected + np.float64(host(loss_b)[0]) * np.float64(w)
    got = host(running)
    assert abs(got[0] - expected) <= 2 * np.spacing(expected), (got[0], expected)
    assert got[1] == FILL


def test_bce_through_the_autograd_function_at_256_by_71(L):
    """hip.binary_cross_entropy_with_logits on all 71 PTB-XL statements at B = 256: (loss * 2).backward() gives twice the
    reference gradient within twice the dx bound; a transposed (non-contiguous) view of the logits gives the bits of its
    contiguous copy, loss and gradient."""
    from ecg_hip import functional as hipF
    n = 256 * 71
    x, t = SR.logits(n, 71).reshape(256, 71), SR.targets(n, "hard", 71).reshape(256, 71)
    loss_ref, dx_ref, _ = SR.bce(x, t)
    b_loss, b_dx = SR.bce_bounds(x, t)
    t_d = torch.from_numpy(t).to(DEV)
    xa = torch.from_numpy(x).to(DEV).requires_grad_(True)
    la = hipF.binary_cross_entropy_with_logits(xa, t_d)
    (la * 2).backward()
    assert abs(la.item() - loss_ref) <= b_loss
    f = SR.worst(host(xa.grad), 2 * dx_ref, 2 * b_dx)
    print(f"bce through autograd, 256 x 71: d(2 loss)/dx error {f:.3f} of twice the dx bound")
    assert f <= 1.0, f
    base = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV).requires_grad_(True)          # (71, 256)
    view = base.t()
    assert not view.is_contiguous() and torch.equal(view.detach(), xa.detach())
    lb = hipF.binary_cross_entropy_with_logits(view, t_d)
    (lb * 2).backward()
    assert same_bits(lb.detach().view(1), la.detach().view(1))
    assert same_bits(base.grad.t().contiguous(), xa.grad)


# ---------------------------------------------------------------------------------------------------------------------
# sigmoid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SR.SIGMOID_N)
def test_sigmoid_vs_float64(L, n):
    x = SR.logits(n, 500 + n)
    x_d = torch.from_numpy(x).to(DEV)
    out_b, out = guarded(n=n)
    L.call("ecg_sigmoid_fwd", L.f32(x_d), L.f32(out), n, L.stream())
    torch.cuda.synchronize()
    f = SR.worst(host(out), SR.sigmoid(x), SR.sigmoid_bound(x))
    print(f"sigmoid n={n}: error {f:.3f} of its bound")
    assert f <= 1.0, f
    assert slack_intact(out_b) and same_bits(x_d, torch.from_numpy(x).to(DEV))


def test_sigmoid_of_nothing_writes_nothing(L):
    x_d = torch.zeros(4, device=DEV)
    out_b, out = guarded(n=4)
    L.call("ecg_sigmoid_fwd", L.f32(x_d), L.f32(out), 0, L.stream())
    torch.cuda.synchronize()
    assert bool((out_b == FILL).all())


# ---------------------------------------------------------------------------------------------------------------------
# AdamW through the ABI
# ---------------------------------------------------------------------------------------------------------------------
class Adam:
    """p, m, v of one step_end_ref.AdamCase in guarded device buffers, stepped through either entry point and compared,
    step by step, with the float64 step from the state the device held before it."""

    def __init__(self, L, case, s):
        self.L, self.c, self.s, self.n = L, case, s, case.n
        (self.p_b, self.p), (self.m_b, self.m), (self.v_b, self.v) = (guarded(a) for a in (case.p, case.m, case.v))
        self.worst = np.zeros(3)

    def hyper(self):
        s = self.s
        return (float(s["lr"]), float(s["betas"][0]), float(s["betas"][1]), float(s["eps"]), float(s["wd"]), float(s["gscale"]))

    def state(self):
        return tuple(host(a).copy() for a in (self.p, self.m, self.v))

    def launch(self, g_d, t=None, counter=None):
        L = self.L
        lr, b1, b2, eps, wd, gs = self.hyper()
        if counter is None:
            L.call("ecg_adamw_step", L.f32(self.p), L.f32(g_d), L.f32(self.m), L.f32(self.v), self.n, t, lr, b1, b2, eps, wd,
                   gs, L.stream())
        else:
            L.call("ecg_adamw_step_graph", L.f32(self.p), L.f32(g_d), L.f32(self.m), L.f32(self.v), self.n, L.ptr(counter),
                   lr, b1, b2, eps, wd, gs, L.stream())
        torch.cuda.synchronize()

    def reference(self, before, g, t):
        s = self.s
        *ref, aux = SR.adamw(*before[:1], g, *before[1:], t, s["lr"], *s["betas"], s["eps"], s["wd"], s["gscale"])
        return ref, SR.adamw_bounds(aux)

    def step(self, t, counter=None, g=None):
        """One launch at step t -> the fractions of the bounds reached by (p, m, v)."""
        g = self.c.grad() if g is None else g
        g_b, g_d = guarded(g)
        before = self.state()
        self.launch(g_d, t, counter)
        ref, bounds = self.reference(before, g, t)
        f = np.array([SR.worst(a, r, b) for a, r, b in zip(self.state(), ref, bounds)])
        self.worst = np.maximum(self.worst, f)
        assert slack_intact(self.p_b, self.m_b, self.v_b, g_b), (self.n, self.s, t)
        assert same_bits(g_d, torch.from_numpy(g).to(DEV)), "the gradient was written"
        return f


def _three_steps(L, n, s):
    a = Adam(L, SR.AdamCase(n, s["t0"], s["gscale"]), s)
    for t in range(s["t0"], s["t0"] + 3):
        f = a.step(t)
        assert np.all(f <= 1.0), (n, s, t, dict(zip("pmv", f)))
    return a.worst


@pytest.mark.parametrize("n", SR.ADAMW_N)
def test_adamw_step_at_every_size(L, n):
    """n < 4 (the ragged tail with no full float4), 4, 5, 7, and n around the 1024-element blocks of 256 threads x float4, at
    the default setting from zero state (t0 = 1) and from a running state (t0 = 10): p, exp_avg and exp_avg_sq."""
    worst = np.zeros(3)
    for t0 in (1, 10):
        worst = np.maximum(worst, _three_steps(L, n, dict(SR.DEFAULT, t0=t0)))
    print(f"adamw n={n}: p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f} of their bounds")


@pytest.mark.parametrize("t0", SR.T0)
def test_adamw_step_over_the_hyperparameter_grid(L, t0):
    """lr x weight decay x betas (beta1 = 0 among them) x eps x grad_scale at n = 4099, three consecutive steps from t0 with
    gradients spanning 1e-16 ... 1e16 and every 7th exactly 0: 108 settings per t0."""
    worst = np.zeros(3)
    for s in SR.grid():
        if s["t0"] == t0:
            worst = np.maximum(worst, _three_steps(L, 4099, s))
    print(f"adamw grid t0={t0}: p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f} of their bounds")


def test_adamw_step_where_the_squared_gradient_overflows(L):
    """(1 - beta2) g g is formed left to right, in the kernel as in torch's addcmul: at |g| = 1e20 it is 1e37, finite, and the
    step is an ordinary one; at |g| = 1e21 it is +inf.  There exp_avg_sq = +inf, the update m / inf is 0 and p' = p * decay
    exactly, exp_avg stays finite within its bound — what float32 torch gives.  The other elements do not notice."""
    n, t, s = 1025, 10, dict(SR.DEFAULT, t0=10)
    c = SR.AdamCase(n, t)
    g = c.grad()
    over, big = np.array([1, 500, 1024]), np.array([2, 501, 1023])
    g[over] = np.float32(1e21) * np.array([1, -1, 1], np.float32)
    g[big] = np.float32(1e20) * np.array([-1, 1, 1], np.float32)
    a = Adam(L, c, s)
    before = a.state()
    (p_ref, m_ref, v_ref), (bp, bm, bv) = a.reference(before, g, t)
    g_b, g_d = guarded(g)
    a.launch(g_d, t)
    p, m, v = a.state()
    rest = np.ones(n, bool)
    rest[over] = False
    assert np.all(v_ref[over] > SR.FLT_MAX) and np.all(v_ref[big] < SR.FLT_MAX)
    assert np.all(np.isposinf(v[over])) and np.isfinite(v[rest]).all()
    decay = np.float32(1.0 - SR.f32r(s["lr"]) * SR.f32r(s["wd"]))
    assert np.array_equal(p[over], before[0][over] * decay)
    assert np.isfinite(m).all() and SR.worst(m, m_ref, bm) <= 1.0
    assert SR.worst(p[rest], p_ref[rest], bp[rest]) <= 1.0 and SR.worst(v[rest], v_ref[rest], bv[rest]) <= 1.0
    assert slack_intact(a.p_b, a.m_b, a.v_b, g_b)


@pytest.mark.parametrize("t0", SR.T0)
@pytest.mark.parametrize("n", SR.GRAPH_N)
def test_adamw_graph_entry_point_called_eagerly(L, n, t0):
    """adamw_graph_kernel reads the step from a device counter and computes the bias corrections with device pow: counter
    preset to t0 - 1; three calls track the reference at t0, t0 + 1, t0 + 2 and leave t0 + 2 in the counter; the first differs
    from the host-argument entry point on identical inputs by no more than the two bounds together."""
    s = dict(SR.DEFAULT, t0=t0)
    graph, eager = Adam(L, SR.AdamCase(n, t0), s), Adam(L, SR.AdamCase(n, t0), s)
    counter = torch.tensor([t0 - 1, 777], dtype=torch.int32, device=DEV)
    for i, t in enumerate(range(t0, t0 + 3)):
        g = graph.c.grad()
        before = graph.state()
        f = graph.step(t, counter, g=g)                                  # (t goes to the reference only: the kernel counts itself)
        assert host(counter).tolist() == [t, 777]
        assert np.all(f <= 1.0), (n, t, dict(zip("pmv", f)))
        if i == 0:
            eager.step(t, g=g)
            _, bounds = graph.reference(before, g, t)
            d = [SR.worst(a, b, 2 * bd) for a, b, bd in zip(graph.state(), eager.state(), bounds)]
            u = [ulps(a, b) for a, b in zip(graph.state(), eager.state())]
            assert max(d) <= 1.0, f"graph against host-argument entry point: (p, m, v) differ by {u} ulp at most"
            print(f"adamw graph n={n} t0={t0}: against the host-argument entry point (p, m, v) differ by {u} ulp at most")
    print(f"adamw graph n={n} t0={t0}: p {graph.worst[0]:.3f}, m {graph.worst[1]:.3f}, v {graph.worst[2]:.3f} of their bounds")


def test_adamw_refusals_launch_nothing(L):
    """step = 0, a buffer 4 bytes past an aligned base (each of p, g, m, v; both entry points) and a null counter are refused
    with EcgHipError, and no buffer or counter changes a bit."""
    n = 1025
    c = SR.AdamCase(n, 10)
    bufs = [guarded(np.concatenate([a, a[:1]]))[0] for a in (c.p, c.grad(), c.m, c.v)]           # n + 1 values, then slack
    kept = [b.clone() for b in bufs]
    counter = torch.tensor([9, 777], dtype=torch.int32, device=DEV)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0)

    def ptrs(shifted=None):
        return [L.f32(b[1:n + 1] if i == shifted else b[:n]) for i, b in enumerate(bufs)]

    refused = [("ecg_adamw_step", (*ptrs(), n, 0, *hyper, L.stream())),
               ("ecg_adamw_step_graph", (*ptrs(), n, None, *hyper, L.stream()))]
    for i in range(4):
        refused.append(("ecg_adamw_step", (*ptrs(i), n, 10, *hyper, L.stream())))
        refused.append(("ecg_adamw_step_graph", (*ptrs(i), n, L.ptr(counter), *hyper, L.stream())))
    for name, args in refused:
        with pytest.raises(L.EcgHipError):
            L.call(name, *args)
    torch.cuda.synchronize()
    assert all(same_bits(b, k) for b, k in zip(bufs, kept)) and host(counter).tolist() == [9, 777]
    L.call("ecg_adamw_step", *ptrs(), n, 10, *hyper, L.stream())          # the same call, aligned and with a step: accepted
    torch.cuda.synchronize()
    assert not same_bits(bufs[0], kept[0]) and same_bits(bufs[1], kept[1])


# ---------------------------------------------------------------------------------------------------------------------
# FlatAdamW's host side, without a model
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(3,), (5, 7), (1024,), (7,)]
OFFS = np.cumsum([0] + [int(np.prod(s)) for s in SHAPES])
N_FLAT = int(OFFS[-1])
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-2, gscale=1.0)


def _flat_adamw(L, case, p0=None, lr=1e-3, capturable=False):
    from ecg_hip.optim import FlatAdamW
    p0 = case.p if p0 is None else p0
    params = [torch.nn.Parameter(torch.from_numpy(p0[a:b].copy()).view(s).to(DEV)) for a, b, s in zip(OFFS, OFFS[1:], SHAPES)]
    opt = FlatAdamW(params, lr=lr, weight_decay=1e-2)
    assert opt.flat_param.numel() == N_FLAT == 1069 and np.array_equal(host(opt.flat_param), p0)
    return (opt.make_capturable() if capturable else opt), params


def _feed(opt, params, g, kinds):
    """Hand the flat gradient g to the parameters: "plain" (a tensor of its own), "placed" (the parameter's slice of
    opt.flat_grad, filled in place, as the backward kernels leave it) or "none".  -> what opt.flat_grad must hold."""
    want = g.copy()
    opt.flat_grad.fill_(777.0)                   # whatever an earlier step left there
    for p, a, b, kind in zip(params, OFFS, OFFS[1:], kinds):
        val = torch.from_numpy(g[a:b].copy()).view(p.shape).to(DEV)
        if kind == "plain":
            p.grad = val
        elif kind == "placed":
            p.grad = opt.flat_grad[a:b].view(p.shape)
            p.grad.copy_(val)
        else:
            p.grad = None
            want[a:b] = 0.0
    return want


def _flat_state(opt):
    torch.cuda.synchronize()
    return tuple(host(t).copy() for t in (opt.flat_param, opt.flat_m, opt.flat_v))


def _flat_step(opt, params, g, t, kinds=("plain",) * 4, lr=1e-3):
    """feed, step, and compare with the float64 step number t from the state before -> fractions of the (p, m, v) bounds."""
    before = _flat_state(opt)
    want = _feed(opt, params, g, kinds)
    opt.step()
    after = _flat_state(opt)
    assert np.array_equal(host(opt.flat_grad).view(np.int32), want.view(np.int32)), kinds
    *ref, aux = SR.adamw(before[0], want, before[1], before[2], t, lr, *HYPER["betas"], HYPER["eps"], HYPER["wd"])
    for p, a, b in zip(params, OFFS, OFFS[1:]):                            # the parameters are the flat buffer
        assert p.data_ptr() == opt.flat_param.data_ptr() + 4 * a
    return np.array([SR.worst(x, r, bd) for x, r, bd in zip(after, ref, SR.adamw_bounds(aux))])


GATHER = {"none placed": ("plain", "plain", "plain", "plain"), "all placed": ("placed", "placed", "placed", "placed"),
          "mixed": ("placed", "plain", "none", "plain"), "mixed, the large one placed": ("none", "plain", "placed", "placed")}


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("name", list(GATHER))
def test_flat_adamw_gathers_gradients_from_wherever_they_are(L, name, capturable):
    """The three branches of FlatAdamW._gather: after step() the flat gradient is exactly the concatenation (zeros for a
    parameter without a gradient, which is then stepped with a zero gradient) and (p, m, v) follow the reference for it;
    two steps, so that the second finds the first one's gradients in the buffer."""
    c = SR.AdamCase(N_FLAT, 1, seed=3)
    opt, params = _flat_adamw(L, c, capturable=capturable)
    for t in (1, 2):
        f = _flat_step(opt, params, c.grad(), t, GATHER[name])
        assert np.all(f <= 1.0), (name, t, f)
        assert opt.steps_taken == t


def test_flat_adamw_continues_in_capturable_mode_after_eager_steps(L):
    c = SR.AdamCase(N_FLAT, 1, seed=4)
    opt, params = _flat_adamw(L, c)
    for t in (1, 2, 3):
        assert np.all(_flat_step(opt, params, c.grad(), t) <= 1.0), t
    assert opt.make_capturable() is opt and opt.steps_taken == 3
    for t in (4, 5):
        assert np.all(_flat_step(opt, params, c.grad(), t) <= 1.0), t
    assert opt.steps_taken == 5


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_flat_adamw_reads_the_learning_rate_at_every_step(L, capturable):
    """param_groups[0]["lr"] changed from 1e-3 to 1e-2 between steps: the next step is the reference's with 1e-2, and not the
    reference's with 1e-3."""
    c = SR.AdamCase(N_FLAT, 1, seed=5)
    opt, params = _flat_adamw(L, c, capturable=capturable)
    assert np.all(_flat_step(opt, params, c.grad(), 1) <= 1.0)
    opt.param_groups[0]["lr"] = 1e-2
    g = c.grad()
    before = _flat_state(opt)
    assert np.all(_flat_step(opt, params, g, 2, lr=1e-2) <= 1.0)
    p_old, _, _, aux = SR.adamw(before[0], g, before[1], before[2], 2, 1e-3, *HYPER["betas"], HYPER["eps"], HYPER["wd"])
    assert SR.worst(_flat_state(opt)[0], p_old, SR.adamw_bounds(aux)[0]) > 100.0


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_flat_adamw_checkpoint_continues_bit_for_bit(L, capturable):
    """state_dict() after two steps, loaded into a second FlatAdamW over clones of the parameters (constructed with another
    learning rate: the checkpoint's counts): the third step on the same gradient gives identical bits in p, m, v and the same
    steps_taken."""
    c = SR.AdamCase(N_FLAT, 1, seed=6)
    a, pa = _flat_adamw(L, c, capturable=capturable)
    for t in (1, 2):
        assert np.all(_flat_step(a, pa, c.grad(), t) <= 1.0)
    sd = a.state_dict()
    b, pb = _flat_adamw(L, c, p0=_flat_state(a)[0], lr=1.0, capturable=capturable)
    b.load_state_dict(sd)
    assert b.steps_taken == a.steps_taken == 2 and b.param_groups[0]["lr"] == 1e-3
    assert b.flat_m.data_ptr() != a.flat_m.data_ptr()
    g = c.grad()
    fa, fb = _flat_step(a, pa, g, 3), _flat_step(b, pb, g, 3)
    assert np.all(fa <= 1.0) and np.all(fb <= 1.0)
    for x, y in zip(_flat_state(a), _flat_state(b)):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert a.steps_taken == b.steps_taken == 3
