"""Pins the CPU oracle's convolution at K = 15 with paddings other than 7 (output length != input length) against
float64 torch.  The golden fixtures (test_oracle_golden.py) only hold 15/7; the GPU tests of the other paddings
(test_gpu_conv_padding.py) lean on the oracle, so the oracle is checked here first.  CPU only.

Bound: 1e-6 absolute.  The oracle accumulates in double, so against float64 torch only the final rounding of the result
to fp32 remains: half an fp32 ulp, 6e-8 for values of order one.  The operands are scaled so that every result IS of
order one (weights by 1/sqrt(Ci K), the cotangent by 1/sqrt(Co K) for dx and by 1/sqrt(N Lo) for dw / db)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

K = 15
PADS = (0, 1, 6, 8, 13, 14)
ATOL = 1e-6
# (N, Ci, Co, L, pads)
SHAPES = [(2, 8, 32, 40, PADS), (1, 4, 32, 1, (14,))]
CASES = [(N, Ci, Co, L, pad) for (N, Ci, Co, L, pads) in SHAPES for pad in pads]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}_{}x{}_L{}_pad{}".format(*c))
def test_oracle_conv_k15_other_paddings_vs_float64_torch(oracle, case):
    N, Ci, Co, L, pad = case
    Lo = L + 2 * pad - K + 1
    assert Lo >= 1
    rng = np.random.default_rng(1000 * L + pad)
    x = rng.standard_normal((N, Ci, L)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    dy = rng.standard_normal((N, Co, Lo)).astype(np.float32)
    dy_x = (dy / np.sqrt(Co * K)).astype(np.float32)          # cotangent for dx: sums of Co*K terms
    dy_w = (dy / np.sqrt(N * Lo)).astype(np.float32)          # cotangent for dw / db: sums of N*Lo terms
    t64 = lambda a: torch.from_numpy(a).double()              # noqa: E731

    y = oracle.conv1d_fwd(x, w, b, pad)
    ry = TF.conv1d(t64(x), t64(w), t64(b), padding=pad).numpy()
    assert y.shape == ry.shape == (N, Co, Lo)
    np.testing.assert_allclose(y, ry, rtol=0, atol=ATOL)

    dx = oracle.conv1d_bwd_data(dy_x, w, L, pad)
    rdx = torch.nn.grad.conv1d_input((N, Ci, L), t64(w), t64(dy_x), padding=pad).numpy()
    assert dx.shape == rdx.shape
    np.testing.assert_allclose(dx, rdx, rtol=0, atol=ATOL)

    dw, db = oracle.conv1d_bwd_weight(dy_w, x, K, pad)
    rdw = torch.nn.grad.conv1d_weight(t64(x), (Co, Ci, K), t64(dy_w), padding=pad).numpy()
    assert dw.shape == rdw.shape
    np.testing.assert_allclose(dw, rdw, rtol=0, atol=ATOL)
    np.testing.assert_allclose(db, dy_w.astype(np.float64).sum(axis=(0, 2)), rtol=0, atol=ATOL)
    # the results are of order one, as the bound assumes (half an fp32 ulp stays below 1e-6 up to |v| < 16)
    assert max(np.abs(ry).max(), np.abs(rdx).max(), np.abs(rdw).max()) < 16
