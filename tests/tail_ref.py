"""Reference of the network tail (everything after the global average pool) as a plain torch composition, runnable in a
chosen dtype on the CPU; importable without a GPU.

    z      = g Wp^T + bp
    h1     = relu(xd W0^T + b0)
    h2     = relu(h1 W2^T + b2)
    film   = h2 Wf^T + bf
    zc     = (1 + tanh(film[:, :F])) * z + film[:, F:]          (zc = z without demographics)
    logits = zc Wh^T + bh

Backward is autograd with both output gradients (d logits, and the extra d z of a consumer of the `z` output).
run(..., torch.float64) is the reference of tests/test_gpu_tail_shapes.py; run(..., torch.float32) is the "stock fp32 path"
its tolerances are measured against; run(..., torch.float32, shorten=...) is the mutation stand-in of
tests/test_tail_ref_host.py: the fp32 composition with ONE reduction shortened by its last term — what a kernel that drops
the last element of a remainder loop would compute — which every GPU assertion's tolerance must reject.
"""
import numpy as np
import torch

# (M, F0, F, D, H1, H, C): the smallest shapes that reach each loop of csrc/tail_fused.hip no other test reaches
CASES = [
    (1, 1, 1, 1, 1, 1, 1),              # every loop at its minimum; one live sample in the pair
    (3, 31, 33, 1, 7, 33, 1),           # reductions of 31 (remainder only) and 33 (one batch + 1); odd M; C = 1
    (2, 256, 128, 3, 64, 32, 3),        # ECGMultimodal(ecg_feat_dim=128, demo_hidden_dim=32) with 3 labels
    (5, 256, 384, 5, 64, 48, 71),       # F > 256 with a half-full second pass; H = 48 (batch + 16); 142 (sample, label) pairs
    (33, 300, 257, 9, 64, 65, 23),      # one feature in the second pass; F0 = 9*32 + 12; H = 2*32 + 1; ragged wgrad tiles
    (130, 256, 512, 5, 64, 64, 44),     # 17 steps per wave in the grouped weight gradient; a short last wave; F = 2*256
    (257, 64, 40, 2, 64, 16, 2),        # F < 64 in the head's wave sum; four pairs; H < 32; odd M > 256
]
LIMIT_CASE = (2, 4096, 2048, 0, 0, 0, 1024)    # without demographics: 48 KB of LDS forward, 56 KB backward
LIMIT_SEED = 200

# (name, demographics, extra d z, x_demo.requires_grad)
FORMS = [("demo", True, True, True), ("nodemo", False, True, False), ("demo_nodz", True, False, True),
         ("demo_noxdgrad", True, True, False), ("nodemo_nodz", False, False, False)]

PARAMS = ("Wp", "bp", "W0", "b0", "W2", "b2", "Wf", "bf", "Wh", "bh")
DEMO_ONLY = ("xd", "W0", "b0", "W2", "b2", "Wf", "bf")

K_TOL = 8.0             # separates rounding from indexing: see tests/test_gpu_tail_shapes.py
K_TOL_LIMIT = 32.0      # the 4 096-term chains of LIMIT_CASE
FLOOR = 2.0 ** -22      # for outputs the CPU computes exactly (the 1-wide case)
RELU_MARGIN = 1e-5      # smallest |pre-activation| a case may have: an order above the fp32 error of these O(1) sums


# 100 + case index, raised in steps of 10 until the case meets the two conditions tests/test_tail_ref_host.py asserts: no
# ReLU pre-activation within RELU_MARGIN of zero, and the last unit of h1 and of h2 live in some sample (a reduction's last
# term multiplied by a dead unit is zero, and a kernel that dropped it could not be told from a correct one)
SEEDS = (140, 101, 122, 143, 104, 105, 116)


def seed_of(case_index):
    return SEEDS[case_index]


def operands(case, seed):
    """Seeded fp32 CPU operands of one case: weights randn / sqrt(fan_in), biases 0.1 randn, g randn, x_demo rand,
    d logits randn, extra d z 0.1 randn.  (D, H1, H = 0: no demographic operands.)"""
    M, F0, F, D, H1, H, C = case
    gen = torch.Generator().manual_seed(seed)

    def W(o, i):
        return torch.randn(o, i, generator=gen) / np.sqrt(i)

    def B(o):
        return 0.1 * torch.randn(o, generator=gen)

    t = {"Wp": W(F, F0), "bp": B(F)}
    if D:
        t.update(W0=W(H1, D), b0=B(H1), W2=W(H, H1), b2=B(H), Wf=W(2 * F, H), bf=B(2 * F))
    t.update(Wh=W(C, F), bh=B(C), g=torch.randn(M, F0, generator=gen))
    if D:
        t["xd"] = torch.rand(M, D, generator=gen)
    t["dlogits"] = torch.randn(M, C, generator=gen)
    t["dz_extra"] = 0.1 * torch.randn(M, F, generator=gen)
    return t


def _short(x, w, b, cut):
    """x w^T + b, the reduction without its last term when `cut`."""
    if cut:
        return x[:, :-1] @ w[:, :-1].t() + b
    return x @ w.t() + b


def run(ops, dtype, demo=True, use_dz=True, xd_grad=True, shorten=None):
    """The tail forward and backward in `dtype`.  -> {"logits", "z", gradient of every operand that has one (keyed like
    `operands`)} as float64 numpy, plus "relu_margin": the smallest |pre-activation| of the two ReLUs (inf without them) and
    "last_unit_live": whether the last unit of h1 and of h2 passes its ReLU in some sample.
    shorten: None | "proj" | "head" | "film_gen" | "W2" (that reduction loses its last term, forward and backward alike) |
    "wgrad" (the sample sum of d Wp / d bp loses its last sample)."""
    demo = demo and "xd" in ops
    leaf = {}
    for k, v in ops.items():
        if k in ("dlogits", "dz_extra") or (not demo and k in DEMO_ONLY):
            continue
        leaf[k] = v.to(dtype).clone().requires_grad_(k != "xd" or xd_grad)
    z = _short(leaf["g"], leaf["Wp"], leaf["bp"], shorten == "proj")
    margin, last_live = float("inf"), True
    if demo:
        p1 = leaf["xd"] @ leaf["W0"].t() + leaf["b0"]
        p2 = _short(torch.relu(p1), leaf["W2"], leaf["b2"], shorten == "W2")
        film = _short(torch.relu(p2), leaf["Wf"], leaf["bf"], shorten == "film_gen")
        F = z.shape[1]
        zc = (1.0 + torch.tanh(film[:, :F])) * z + film[:, F:]
        margin = min(p1.detach().abs().min().item(), p2.detach().abs().min().item())
        last_live = bool(p1.detach()[:, -1].max() > 0 and p2.detach()[:, -1].max() > 0)
    else:
        zc = z
    logits = _short(zc, leaf["Wh"], leaf["bh"], shorten == "head")
    if shorten == "wgrad":
        z.retain_grad()
    outs, grads = [logits], [ops["dlogits"].to(dtype)]
    if use_dz:
        outs.append(z)
        grads.append(ops["dz_extra"].to(dtype))
    torch.autograd.backward(outs, grads)
    res = {"logits": logits.detach(), "z": z.detach()}
    for k, v in leaf.items():
        if v.requires_grad:
            res[k] = v.grad
    if shorten == "wgrad":
        res["Wp"] = z.grad[:-1].t() @ leaf["g"].detach()[:-1]
        res["bp"] = z.grad[:-1].sum(0)
    res = {k: v.double().numpy() for k, v in res.items()}
    res["relu_margin"], res["last_unit_live"] = margin, last_live
    return res


# ---- the tolerance rule of the GPU tests -------------------------------------------------------------------------------
def rel_rms(a, r):
    """RMS of (a - r) over the RMS of r; 0 where both vanish, inf where only r does."""
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    num, den = float(np.sqrt(np.mean((a - r) ** 2))), float(np.sqrt(np.mean(r ** 2)))
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def max_err(a, r):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(r, dtype=np.float64)).max())


def bounds(cpu32, ref64, k=K_TOL):
    """(rel-RMS bound, max-error bound) of one output: k times what the CPU fp32 run leaves against float64, plus the floor."""
    return (k * rel_rms(cpu32, ref64) + FLOOR,
            k * max_err(cpu32, ref64) + FLOOR * float(np.abs(np.asarray(ref64)).max()))


def measure(got, cpu32, ref64, k=K_TOL):
    """-> dict(rms, max: the errors of `got`; rms_cpu, max_cpu: those of the CPU fp32 run; rms_bound, max_bound; ok)."""
    b_rms, b_max = bounds(cpu32, ref64, k)
    e_rms, e_max = rel_rms(got, ref64), max_err(got, ref64)
    return dict(rms=e_rms, max=e_max, rms_cpu=rel_rms(cpu32, ref64), max_cpu=max_err(cpu32, ref64), rms_bound=b_rms,
                max_bound=b_max, ok=bool(e_rms <= b_rms and e_max <= b_max))


def report(what, name, m):
    """One printed line per output and case: the measured errors and their ratio to the CPU fp32 run's."""
    ratio = m["rms"] / m["rms_cpu"] if m["rms_cpu"] > 0 else float("nan")
    print(f"{what:44s} {name:7s} rel-RMS {m['rms']:.2e} (cpu fp32 {m['rms_cpu']:.2e}, ratio {ratio:5.2f}, bound {m['rms_bound']:.2e})"
          f"  max {m['max']:.2e} (cpu fp32 {m['max_cpu']:.2e}, bound {m['max_bound']:.2e})")
    return ratio
