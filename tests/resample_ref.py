"""numpy restatement of the polyphase resampler of the input step (include/ecg_hip.h, ecg_wfdb16_windows_resampled) —
TEST INFRASTRUCTURE ONLY.

    M = n*down + half;  phi = M mod up;  k0 = M div up
    y[n] = sum over i = 0 .. ntap-1 ascending of  g[phi][i] * p[clamp(k0 - i, 0, Ttot-1)],   n in [0, ceil(Ttot*up/down))

Vectorised over n with a Python loop over i: every output's products are added in the kernel's order, each product and each
sum rounded on its own.  dtype=np.float32 is the bit-exact oracle, dtype=np.float64 the accuracy reference.  The z-score is
NOT restated: it is oracle/input_oracle.normalize_per_lead on the view the reference hands it.
"""
import numpy as np

from oracle import input_oracle as io_ref


def physical(d, gain, baseline):
    """d int16 [Ttot, leads] -> the physical samples float32 [Ttot, leads] (wfdb's DAC, -32768 -> NaN, then the cast)."""
    return np.asarray(io_ref.wfdb16_physical(d, gain, baseline), dtype=np.float32)


def table(h, up):
    """FIR h [2*half + 1] -> polyphase table [up, ntap] of the same dtype: g[phi][i] = h[phi + i*up], 0 past the end."""
    ntap = -(-len(h) // up)
    g = np.zeros((up, ntap), dtype=h.dtype)
    for phi in range(up):
        col = h[phi::up]
        g[phi, :len(col)] = col
    return g


def resample(p, g, half, up, down, dtype=np.float32):
    """p [Ttot] or [Ttot, leads], g [up, ntap] -> y [Tout(, leads)] in `dtype`."""
    p = np.asarray(p, dtype=dtype)
    g = np.asarray(g, dtype=dtype)
    Ttot, ntap = p.shape[0], g.shape[1]
    Tout = -(-Ttot * up // down)
    M = np.arange(Tout, dtype=np.int64) * down + half
    phi, k0 = M % up, M // up
    tail = (1,) * (p.ndim - 1)
    acc = np.zeros((Tout,) + p.shape[1:], dtype=dtype)
    for i in range(ntap):
        term = g[phi, i].reshape((Tout,) + tail) * p[np.clip(k0 - i, 0, Ttot - 1)]
        acc = acc + term
    assert acc.dtype == dtype
    return acc


def windows(y, starts, T):
    """y [Tout, leads] -> the physical windows [W, leads, T] cut at `starts` (views transposed as the reference's)."""
    return np.stack([np.ascontiguousarray(y[s:s + T].T) for s in starts])


def zscored(y, starts, T):
    """-> (x [W, leads, T], stats [W*leads, 2]): input_oracle.normalize_per_lead on each window AS THE REFERENCE SEES IT, a
    [leads, T] view of a [T, leads] buffer (numpy then sums left to right per lead).  One lead: the column is doubled, since
    a [T, 1] buffer is contiguous either way and numpy would sum it pairwise."""
    xs, st = [], []
    for s in starts:
        buf = np.ascontiguousarray(y[s:s + T])
        leads = buf.shape[1]
        if leads == 1:
            buf = np.repeat(buf, 2, axis=1)
        v = buf.T
        xs.append(np.ascontiguousarray(io_ref.normalize_per_lead(v))[:leads])
        st.append(np.stack([v.mean(axis=1), v.std(axis=1) + np.float32(1e-6)], axis=1)[:leads])
    return np.stack(xs), np.concatenate(st).astype(np.float32)
