"""Host side of the on-device polyphase resampler (ecg_wfdb16_windows_resampled): the rational ratio of two sampling
rates, the FIR design and its polyphase table.  numpy only.

The filter is scipy.signal.resample_poly's default: for up/down in lowest terms, m = max(up, down), half = 10*m,
    h[j] = (1/m) * sinc((j - half)/m) * kaiser(2*half + 1, beta=5.0)[j],   normalised to sum 1, times up
(scipy: firwin(2*half + 1, 1/m, window=("kaiser", 5.0)) * up), designed in float64.  The kernel reads it as the table
    g[phi][i] = float32(h[phi + i*up]),  phi in [0, up), i in [0, ntap), ntap = ceil((2*half + 1)/up),  0 past the end
and computes  y[n] = sum_i g[phi][i] * p[clamp(k0 - i)]  with  M = n*down + half, phi = M mod up, k0 = M div up.
"""
import math
from fractions import Fraction

import numpy as np

MAX_TERM = 512      # the C ABI's limit on up and down


def rational_ratio(fs_in, fs_out):
    """-> (up, down) with up/down == fs_out/fs_in in lowest terms.  ValueError unless both terms are <= 512 and the
    fraction reproduces the ratio within 1e-9 relative (499.7 Hz -> 500 Hz has no such fraction)."""
    fs_in, fs_out = float(fs_in), float(fs_out)
    if not (fs_in > 0 and fs_out > 0 and math.isfinite(fs_in) and math.isfinite(fs_out)):
        raise ValueError(f"sampling rates must be positive and finite, got {fs_in} -> {fs_out}")
    ratio = Fraction(fs_out) / Fraction(fs_in)
    fr = ratio.limit_denominator(MAX_TERM)
    up, down = fr.numerator, fr.denominator
    if up < 1 or up > MAX_TERM or down > MAX_TERM or abs(fr - ratio) > Fraction(1, 10 ** 9) * ratio:
        raise ValueError(f"{fs_in:g} Hz -> {fs_out:g} Hz is not a ratio up/down with both terms <= {MAX_TERM} "
                         f"(closest: {up}/{down}); resample the recording offline")
    return up, down


def design_filter(up, down):
    """-> (h float64 [2*half + 1], half): the prototype low-pass described in the module docstring."""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"up={up} and down={down} must be >= 1")
    m = max(up, down)
    half = 10 * m
    j = np.arange(2 * half + 1, dtype=np.float64)
    h = (1.0 / m) * np.sinc((j - half) / m) * np.kaiser(2 * half + 1, 5.0)
    h = h / h.sum()
    return h * up, half


def design_taps(up, down):
    """-> (g float32 [up, ntap], half): the polyphase table of design_filter(up, down)."""
    h, half = design_filter(up, down)
    up = int(up)
    ntap = -(-len(h) // up)
    padded = np.zeros(up * ntap, dtype=np.float64)
    padded[:len(h)] = h
    return np.ascontiguousarray(padded.reshape(ntap, up).T.astype(np.float32)), half


def resampled_length(Ttot, up, down):
    """Samples of the resampled recording: ceil(Ttot*up/down) (exact: Python integers)."""
    return -(-int(Ttot) * int(up) // int(down))


_tables = {}        # (up, down, device) -> (table tensor [up, ntap], ntap, half)


def device_taps(up, down, device):
    """The table of design_taps on `device`, uploaded once per (up, down, device) and kept (at most 512 KB each)."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(up), int(down), device)
    ent = _tables.get(key)
    if ent is None:
        g, half = design_taps(up, down)
        ent = _tables[key] = (torch.from_numpy(g).to(device), g.shape[1], half)
    return ent
