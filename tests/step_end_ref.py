"""Float64 restatements of the kernels that end a training step — bce_kernel and sigmoid_kernel (csrc/tail.hip), adamw_kernel
and adamw_graph_kernel (csrc/optim.hip) — with the error bound of each output, the float32 op-by-op restatement the bounds
are checked against without a GPU (tests/test_step_end_ref_host.py), and the seeded case lists both test files share.
Plain numpy, importable without torch or a GPU.

Bounds.  u = 2^-24, one float32 rounding relative to the value rounded.  Each output is a chain of at most eight float32
roundings of quantities no larger than its `scale`: at most 4 u * scale when they add up, doubled as margin for fma contraction
and the device's expf / log1pf.

    loss     u |loss| + 8 u mean(max(x, 0) + |x t| + log1p(exp(-|x|)))      (terms are summed in double; one rounding at the end)
    dx       (8 u max(sigma(x), t) + 1e-37) / numel                         (floor: expf overflows at x < -88, fp32 gives 0)
    sigmoid  4 u sigma(x) + 1e-37
    m'       8 u max(|m|, |g gscale|)
    v'       8 u v'
    p'       8 u (|p| + (lr / bc1) max(|m|, |g gscale|, |m'|) / denom)

Largest error as a fraction of its bound over the case lists below, written down once:
                                   loss    dx      sigmoid  p       m       v
    float32 restatement, CPU       0.09    0.45    0.76     0.52    0.35    0.39     (4.2 u, 2.8 u, 3.1 u * scale for p, m, v)
    the kernels, MI355X            0.05    0.38    0.50     0.52    0.26    0.39     (adamw_graph_kernel: 0.24, 0.12, 0.23)
The first row is asserted (<= 1, figures printed) in tests/test_step_end_ref_host.py, the second in
tests/test_gpu_step_end.py; the bounds come from the count of roundings, not from either row.

The AdamW reference takes every hyperparameter as the float32 value the C ABI receives (ecg_adamw_step takes `float`), widened
back to double: the kernel derives 1 - beta2 and the bias corrections from the float32 beta2, so v / bc2 is unbiased and p is what
a run with double betas gives, while the stored exp_avg_sq sits about 1.3e-5 relative from stock torch's (which multiplies by
float32(1 - 0.999) = 0.001000000047 where the kernel has 1f - 0.999f = 0.00099998713).

Out of scope: |g gscale| below 1e-16, where g^2 (1 - beta2) leaves the normal float32 range and the relative bound on v' has no
meaning.  The gradient lists below stop at 0.5e-16 / 8, whose square times 0.001 is 3.9e-38: still normal.
"""
import numpy as np

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def f32r(x):
    """A Python number as the float32 the ABI receives, widened back to double."""
    return float(np.float32(x))


# ---- BCE with logits, sigmoid ------------------------------------------------------------------------------------------
def sigmoid(x):
    x = _f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce(x, t):
    """-> (loss, dx, terms) in float64 of mean BCE-with-logits; finite logits only."""
    x, t = _f64(x), _f64(t)
    assert x.shape == t.shape and x.size > 0 and np.isfinite(x).all()
    terms = np.maximum(x, 0.0) - x * t + np.log1p(np.exp(-np.abs(x)))
    return float(terms.mean()), (sigmoid(x) - t) / x.size, terms


def bce_bounds(x, t):
    """-> (bound of the loss, bound of each dx element)."""
    x, t = _f64(x), _f64(t)
    loss = bce(x, t)[0]
    scale = np.mean(np.maximum(x, 0.0) + np.abs(x * t) + np.log1p(np.exp(-np.abs(x))))
    return U * abs(loss) + 8 * U * float(scale), (8 * U * np.maximum(sigmoid(x), t) + 1e-37) / x.size


def sigmoid_bound(x):
    return 4 * U * sigmoid(x) + 1e-37


# ---- AdamW -------------------------------------------------------------------------------------------------------------
def adamw(p, g, m, v, t, lr, b1, b2, eps, wd, gscale=1.0):
    """torch.optim.AdamW's single-tensor step number t in float64: decoupled decay, lerp, addcmul,
    denom = sqrt(v') / sqrt(bc2) + eps, step lr / bc1.  State and gradient are widened as they come (the GPU tests hand in the
    device's float32 arrays; float64 state follows a float64 trajectory); every hyperparameter is first rounded to float32.
    -> (p', m', v', aux); aux holds the intermediates of adamw_bounds."""
    lr, b1, b2, eps, wd, gscale = (f32r(h) for h in (lr, b1, b2, eps, wd, gscale))
    p, g, m, v = (_f64(a) for a in (p, g, m, v))
    gs = g * gscale
    decay = 1.0 - lr * wd
    m1 = m + (gs - m) * (1.0 - b1)
    v1 = v * b2 + (1.0 - b2) * gs * gs
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    step = lr / bc1
    p1 = p * decay - step * (m1 / denom)                    # eps > 0: denom > 0 also where the state and gradient are 0
    aux = dict(p0=p, m0=m, gs=gs, m1=m1, v1=v1, denom=denom, step=step, decay=decay)
    return p1, m1, v1, aux


def adamw_bounds(aux):
    """-> (bound of p', of m', of v') per element."""
    in_m = np.maximum(np.abs(aux["m0"]), np.abs(aux["gs"]))
    move = aux["step"] * np.maximum(in_m, np.abs(aux["m1"])) / aux["denom"]
    return 8 * U * (np.abs(aux["p0"]) + move), 8 * U * in_m, 8 * U * aux["v1"]


def worst(got, ref, bound):
    """Largest |got - ref| / bound over the elements (0 / 0 counts as 0, anything / 0 as inf)."""
    err = np.abs(_f64(got) - _f64(ref))
    bound = np.broadcast_to(_f64(bound), err.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ---- the float32 op-by-op restatements (every operation rounded on its own, as the kernels without fma contraction) ------
_F = np.float32


def bce_f32(x, t):
    """bce_kernel in numpy float32: the terms in float32, their sum in double, one rounding of the mean."""
    x, t = np.asarray(x, _F), np.asarray(t, _F)
    with np.errstate(over="ignore", under="ignore"):
        terms = np.maximum(x, _F(0)) - x * t + np.log1p(np.exp(-np.abs(x)))
        inv = _F(1) / _F(x.size)
        dx = (_F(1) / (_F(1) + np.exp(-x)) - t) * inv
    assert terms.dtype == _F and dx.dtype == _F
    return _F(terms.astype(np.float64).sum() / float(x.size)), dx


def sigmoid_f32(x):
    x = np.asarray(x, _F)
    with np.errstate(over="ignore", under="ignore"):
        return _F(1) / (_F(1) + np.exp(-x))


def adamw_f32(p, g, m, v, t, lr, b1, b2, eps, wd, gscale=1.0, torch_beta2=False):
    """adam1 of csrc/optim.hip in numpy float32 with the host-side arguments of ecg_adamw_step (computed in double from the
    float32 hyperparameters, rounded once); 1f - beta formed in float32.  torch_beta2=True is the form stock torch runs on
    float32 tensors with Python-double betas instead: addcmul's value is float32(1 - beta2) and bc2 comes from the double
    beta2 (the multiply by beta2 rounds it to float32 either way)."""
    p, g, m, v = (np.asarray(a, _F).copy() for a in (p, g, m, v))
    b2_double = float(b2)
    lr, b1, b2, eps, wd, gscale = (_F(h) for h in (lr, b1, b2, eps, wd, gscale))
    decay = _F(1.0 - float(lr) * float(wd))
    step = _F(float(lr) / (1.0 - float(b1) ** t))
    one_b2 = _F(1.0 - b2_double) if torch_beta2 else _F(1) - b2
    bc2_sqrt = _F(np.sqrt(1.0 - (b2_double if torch_beta2 else float(b2)) ** t))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        g = g * gscale
        p = p * decay
        m = m + (g - m) * (_F(1) - b1)
        add = (one_b2 * g) * g
        v = (v.astype(np.float64) * float(b2) + add.astype(np.float64)).astype(_F)        # __fmaf_rn
        denom = np.sqrt(v) / bc2_sqrt + eps
        p = p - step * (m / denom)
    assert p.dtype == m.dtype == v.dtype == _F
    return p, m, v


# ---- case lists shared by tests/test_step_end_ref_host.py and tests/test_gpu_step_end.py -----------------------------------
NUMEL = [1, 2, 63, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 4097, 18176]
SIGMOID_N = [1, 255, 256, 257, 18176]
SPECIAL_LOGITS = [40.0, -40.0, 88.0, -88.0, 90.0, -90.0, 103.9, -103.9, 15.0, -15.0, 0.0, 1e-8, -1e-8, 1e-30, -1e-30]
TARGET_KINDS = ["hard", "soft"]


def logits(n, seed):
    """N(0, 3^2) float32 logits with SPECIAL_LOGITS spliced in at seeded positions (as many of them as fit into n)."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal(n)).astype(np.float32)
    k = min(n, len(SPECIAL_LOGITS))
    x[rng.choice(n, size=k, replace=False)] = rng.permutation(np.asarray(SPECIAL_LOGITS, dtype=np.float32))[:k]
    return x


def targets(n, kind, seed):
    rng = np.random.default_rng(seed + 7919)
    if kind == "hard":
        return (rng.random(n) < 0.3).astype(np.float32)
    return rng.uniform(0.0, 0.9, n).astype(np.float32)


ONCE_NUMEL = [2049, 4097, 18176]


def once_positions(n):
    return [0, 1023, 1024, 2047, 2048, n - 1]


def once_case(n, k):
    """Every logit -30 against target 0 (term 9.4e-14) but logit +20 at position k (term 20): the loss is 20 / n when every
    element is counted exactly once, and 1e-3 relative away (at these n, at least 5e-5) when one is dropped or doubled."""
    x = np.full(n, -30.0, dtype=np.float32)
    x[k] = 20.0
    return x, np.zeros(n, dtype=np.float32)


ADAMW_N = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 2047, 2048, 2049, 4099]
GRAPH_N = [3, 1025, 4099]
T0 = [1, 10, 1000, 100000]
DEFAULT = dict(lr=1e-3, wd=1e-2, betas=(0.9, 0.999), eps=1e-8, gscale=1.0)
GRID_LR = [1e-3, 1e-1]
GRID_WD = [0.0, 1e-2, 0.5]
GRID_BETAS = [(0.9, 0.999), (0.5, 0.9), (0.0, 0.5)]
GRID_EPS = [1e-8, 1e-3]
GRID_GSCALE = [1.0, 1.0 / 8.0, 1.0 / 3.0]


def grid():
    """The 432 settings of the N = 4099 sweep as dicts like DEFAULT plus t0."""
    return [dict(lr=lr, wd=wd, betas=b, eps=eps, gscale=gs, t0=t0) for lr in GRID_LR for wd in GRID_WD for b in GRID_BETAS
            for eps in GRID_EPS for gs in GRID_GSCALE for t0 in T0]


class AdamCase:
    """Seeded parameters, state and gradients of one AdamW case of n elements.  Gradients are sign * 10^k * U(0.5, 1.5) with
    k uniform in -16 ... 16 per element (the same k at every step: fresh gradients of the same scale) and every 7th element
    (index 6, 13, ...: none at n < 7, so that the smallest sizes carry live elements) exactly 0.  State: zeros at t0 = 1; otherwise m = g0' U(-1, 1), v = g0'^2 U(0.5, 1.5) with g0' = g0 * gscale, a gradient
    of the same scale as the ones that follow — what the state of a real run looks like."""

    def __init__(self, n, t0, gscale=1.0, seed=0):
        self.n, self.rng = n, np.random.default_rng(1000003 * seed + 31 * n + t0)
        self.k = self.rng.integers(-16, 17, n)
        self.p = self.rng.standard_normal(n).astype(np.float32)
        if t0 == 1:
            self.m, self.v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        else:
            g0 = self.grad().astype(np.float64) * f32r(gscale)
            self.m = (g0 * self.rng.uniform(-1.0, 1.0, n)).astype(np.float32)
            self.v = (g0 * g0 * self.rng.uniform(0.5, 1.5, n)).astype(np.float32)

    def grad(self):
        g = self.rng.choice([-1.0, 1.0], self.n) * 10.0 ** self.k * self.rng.uniform(0.5, 1.5, self.n)
        g[6::7] = 0.0
        return g.astype(np.float32)
