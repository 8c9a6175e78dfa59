"""Host-side checks of ecg_hip.params, the one table of gradient sinks and collectives statements: a record answers for an
address only while its parameter lives there, a sink goes out at most once per backward pass (and again after a pass that
raised), and an owner that goes away withdraws only its own word.  No kernel runs: a three-line autograd.Function asks the
table for its weight gradient's destination exactly as the kernels' wrappers do."""
import gc

import pytest
import torch


@pytest.fixture
def P(monkeypatch):
    from ecg_hip import params
    for name, clean in (("_records", {}), ("_by_ptr", {}), ("_handed", set()), ("_bn_one_launch", True),
                        ("_multi_rank", lambda: False)):
        monkeypatch.setattr(params, name, clean)
    return params


class _Scale(torch.autograd.Function):
    """y = x * w, elementwise."""
    taken = []              # data_ptr of every gradient destination the table gave out

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x)
        ctx.key = w.data_ptr()
        return x * w

    @staticmethod
    def backward(ctx, dy):
        from ecg_hip import functional as F
        (x,) = ctx.saved_tensors
        dw = F._grad_out(ctx.key, dy, *x.shape)
        _Scale.taken.append(dw.data_ptr())
        dw.copy_(dy * x)
        return None, dw


class _Raise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        raise RuntimeError("backward failed")


def _backward(w, x):
    w.grad = None
    _Scale.apply(x, w).sum().backward()
    return w.grad


def _inside(t, flat):
    return flat.data_ptr() <= t.data_ptr() < flat.data_ptr() + 4 * flat.numel()


def test_a_sink_does_not_answer_for_another_parameter_at_the_address_its_own_left(P):
    """The rule for the parameter that moved: no sink at its new address until the table is told (parameters_rehomed, or a
    new registration); from then on the sink follows the parameter object."""
    from ecg_hip import functional as F
    p, flat, x = torch.nn.Parameter(torch.randn(4)), torch.zeros(4), torch.randn(4)
    F.register_grad_sinks([p], [flat])
    assert _backward(p, x).data_ptr() == flat.data_ptr() and torch.equal(flat, x)
    flat.zero_()
    q = torch.nn.Parameter(p.data)                    # another parameter at the address ...
    p.data = torch.randn(4)                           # ... that p has just left
    assert q.data_ptr() != p.data_ptr()
    g = _backward(q, x)
    assert torch.equal(g, x) and not _inside(g, flat) and not flat.any()
    g = _backward(p, x)                               # nobody has told the table where p lives now
    assert torch.equal(g, x) and not _inside(g, flat) and not flat.any()
    F.parameters_rehomed()
    assert _backward(p, x).data_ptr() == flat.data_ptr() and torch.equal(flat, x)
    flat.zero_()
    g = _backward(q, x)
    assert torch.equal(g, x) and not _inside(g, flat) and not flat.any()


def test_a_statement_does_not_answer_for_another_parameter_at_the_address_its_own_left(P):
    from ecg_hip import functional as F
    p = torch.nn.Parameter(torch.zeros(4))
    F.declare_backward_collectives([p], True)
    assert not F.bn_backward_one_launch_allowed(p.data_ptr())
    q = torch.nn.Parameter(p.data)
    p.data = torch.zeros(4)
    assert F.bn_backward_one_launch_allowed(q.data_ptr())          # undeclared, one rank: allowed
    assert F.bn_backward_one_launch_allowed(p.data_ptr())          # p itself counts as undeclared until the table is told
    F.parameters_rehomed()
    assert not F.bn_backward_one_launch_allowed(p.data_ptr()) and F.bn_backward_one_launch_allowed(q.data_ptr())


@pytest.mark.parametrize("kind", ["flat", "adopted"])
def test_a_sink_goes_out_once_per_backward_pass_and_again_after_a_pass_that_raised(P, kind):
    from ecg_hip import functional as F
    from ecg_hip.optim import FlatAdamW, adopt_stock_adamw
    w = torch.nn.Parameter(torch.randn(5))
    opt = FlatAdamW([w], lr=1e-3) if kind == "flat" else adopt_stock_adamw(torch.optim.AdamW([w], lr=1e-3), allow_cpu=True)
    sink, (x1, x2) = opt.flat_grad.data_ptr(), torch.randn(2, 5)
    # used twice in one graph: the sink once, a private tensor for the second gradient, which autograd adds to the first
    _Scale.taken.clear()
    (_Scale.apply(x1, w) + _Scale.apply(x2, w)).sum().backward()
    assert _Scale.taken.count(sink) == 1 and len(_Scale.taken) == 2
    assert torch.equal(w.grad, x1 + x2)
    # the pass ended: the next one gets the sink again without anybody's help
    opt.zero_grad()
    assert _backward(w, x1).data_ptr() == sink

    def fail_a_pass():
        """A backward pass that raises after the sink went out: the engine runs no end-of-pass callback."""
        w.grad = None
        late = _Raise.apply(torch.zeros(5, requires_grad=True))      # (created first: its backward runs after _Scale's)
        with pytest.raises(RuntimeError, match="backward failed"):
            (_Scale.apply(x1, w).sum() + late.sum()).backward()
        assert P._handed
        w.grad = None

    # whatever begins a new step hands the sinks out again: backward_from_loss on its own, zero_grad or step before a
    # plain backward()
    fail_a_pass()
    F.backward_from_loss(_Scale.apply(x2, w).sum())
    assert w.grad.data_ptr() == sink and torch.equal(opt.flat_grad, x2)
    fail_a_pass()
    opt.zero_grad()
    assert _backward(w, x1).data_ptr() == sink
    fail_a_pass()
    w.grad = torch.zeros(5)
    opt.step()
    assert _backward(w, x2).data_ptr() == sink


def test_an_owner_that_goes_away_withdraws_only_what_it_said_itself(P):
    from ecg_hip import functional as F
    from ecg_hip.optim import FlatAdamW

    class Owner:
        pass

    ps, x = [torch.nn.Parameter(torch.randn(3)), torch.nn.Parameter(torch.randn(3))], torch.randn(3)
    first, second = Owner(), Owner()
    flats = [torch.zeros(6), torch.zeros(6)]
    for o, flat, busy in ((first, flats[0], False), (second, flats[1], True)):      # the later word stands
        token = P.owner_token(o)
        F.register_grad_sinks(ps, [flat[:3], flat[3:]], token)
        F.declare_backward_collectives(ps, busy, owner=token)
    del first, o
    gc.collect()
    assert _inside(_backward(ps[1], x), flats[1]) and torch.equal(flats[1][3:], x) and not flats[0].any()
    assert not any(F.bn_backward_one_launch_allowed(p.data_ptr()) for p in ps)
    del second
    gc.collect()
    assert not _inside(_backward(ps[1], x), flats[1])
    assert all(F.bn_backward_one_launch_allowed(p.data_ptr()) for p in ps) and not P._records and not P._by_ptr
    # the same with two optimizers over the same parameters
    oa, ob = FlatAdamW(ps), FlatAdamW(ps)
    del oa
    gc.collect()
    assert _inside(_backward(ps[0], x), ob.flat_grad) and _inside(_backward(ps[1], x), ob.flat_grad)
    del ob
    gc.collect()
    assert not P._records
