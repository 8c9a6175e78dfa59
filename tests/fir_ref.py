"""numpy restatement of the zero-phase FIR of the input step (include/ecg_hip.h, ecg_fir_windows) — TEST INFRASTRUCTURE ONLY.

    acc = c[0]*x[n];  for i = 1 .. half ascending:  acc = acc + c[i] * (x[clamp(n-i)] + x[clamp(n+i)]);  y[n] = acc

The folded loop over i, vectorised over n: every output's terms are added in the kernel's order, the symmetric pair first,
each add and each multiply rounded on its own.  dtype=np.float32 is the bit-exact oracle, dtype=np.float64 the accuracy
reference.  physical, windows and zscored are tests/resample_ref.py's: the z-score is NOT restated here either.
"""
import numpy as np

from resample_ref import physical, windows, zscored  # noqa: F401


def fir(x, c, dtype=np.float32):
    """x [Ttot] or [Ttot, leads], c [half+1] one-sided taps -> y of x's shape in `dtype`."""
    x = np.asarray(x, dtype=dtype)
    c = np.asarray(c, dtype=dtype)
    Ttot = x.shape[0]
    n = np.arange(Ttot)
    acc = c[0] * x
    for i in range(1, len(c)):
        pair = x[np.clip(n - i, 0, Ttot - 1)] + x[np.clip(n + i, 0, Ttot - 1)]
        term = c[i] * pair
        acc = acc + term
    assert acc.dtype == dtype
    return acc


def bound(x, c):
    """The recursive-summation bound on |fir(float32) - fir(float64)| for fp32 taps and data: a term passes through at
    most half+2 roundings, so |err[n]| <= gamma_{half+2} * sum_i |c[i]|*(|x[n-i]| + |x[n+i]|), gamma_k = k*u/(1 - k*u)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    c = np.abs(np.asarray(c, dtype=np.float64))
    Ttot = x.shape[0]
    n = np.arange(Ttot)
    mag = c[0] * x
    for i in range(1, len(c)):
        mag = mag + c[i] * (x[np.clip(n - i, 0, Ttot - 1)] + x[np.clip(n + i, 0, Ttot - 1)])
    k, u = len(c) + 1, 2.0 ** -24
    return k * u / (1 - k * u) * mag
