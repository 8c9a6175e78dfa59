"""Host side of the on-device zero-phase FIR conditioning (ecg_fir_windows): Kaiser-window designs of the baseline-wander
high-pass, the mains notch and an optional low-pass, their cascade, and the one-sided fp32 form the kernel reads.
numpy only; every design is float64.

    N, beta = kaiserord(atten, width/(fs/2)), N forced odd (N |= 1), half = N // 2
    lowpass   lp[j] = c * sinc(c*(j - half)) * kaiser(N, beta)[j],  c = cutoff/(fs/2),  normalised to sum 1
              (scipy.signal.firwin(N, cutoff, window=("kaiser", beta), fs=fs) to float64 rounding)
    highpass  delta - lowpass                      spectral inversion: DC gain 0 to float64 rounding (about 2e-8 once the
              taps are fp32) — not firwin(pass_zero=False), which scales at Nyquist and leaves a DC gain near 1e-5
    notch     delta - (lowpass(f0 + bw/2) - lowpass(f0 - bw/2))
    cascade   np.convolve of the stages, then (c + c[::-1])/2: symmetric exactly

The kernel computes  y[n] = c[0]*x[n] + sum_{i=1..half} c[i]*(x[n-i] + x[n+i])  with c = one_sided(h), ends edge-held.
A symmetric FIR applied centred has zero phase: no sample of the ECG moves in time.  The price of a 0.5 Hz transition is
length — half = 363 at 100 Hz, 1813 at 500 Hz — and an invalid sample (NaN) poisons every output within `half` samples.
"""
import math
from collections import OrderedDict

import numpy as np

MAX_HALF = 4096     # the C ABI's limit on half


def kaiserord(atten, width):
    """-> (N, beta): scipy.signal.kaiserord restated (Kaiser's empirical formulas); width as a fraction of Nyquist."""
    a = abs(float(atten))
    if a < 8:
        raise ValueError(f"atten={atten} dB is too small for a Kaiser design")
    if not 0 < width < 1:
        raise ValueError(f"transition width {width} (fraction of Nyquist) outside (0, 1)")
    if a > 50:
        beta = 0.1102 * (a - 8.7)
    elif a > 21:
        beta = 0.5842 * (a - 21) ** 0.4 + 0.07886 * (a - 21)
    else:
        beta = 0.0
    return int(math.ceil((a - 7.95) / 2.285 / (np.pi * width) + 1)), beta


def lowpass(fs, cutoff, width, atten=60.0):
    """-> h float64, odd length: low-pass with the -6 dB point at `cutoff` Hz and a transition `width` Hz wide."""
    fs, cutoff, width = float(fs), float(cutoff), float(width)
    nyq = fs / 2
    if not (fs > 0 and 0 < cutoff < nyq):
        raise ValueError(f"cutoff={cutoff:g} Hz outside (0, fs/2={nyq:g})")
    N, beta = kaiserord(atten, width / nyq)
    N |= 1
    half = N // 2
    c = cutoff / nyq
    h = c * np.sinc(c * (np.arange(N, dtype=np.float64) - half)) * np.kaiser(N, beta)
    return h / h.sum()


def _delta_minus(h):
    out = -h
    out[len(h) // 2] += 1.0
    return out


def highpass(fs, cutoff=0.5, width=0.5, atten=60.0):
    """-> h float64, odd length: delta - lowpass(fs, cutoff, width, atten).  The default removes baseline wander."""
    return _delta_minus(lowpass(fs, cutoff, width, atten))


def notch(fs, f0, bandwidth=2.0, width=1.0, atten=60.0):
    """-> h float64, odd length: rejects f0 +- bandwidth/2 Hz (mains hum: f0 = 50 or 60)."""
    fs, f0, bandwidth, width = float(fs), float(f0), float(bandwidth), float(width)
    if f0 + bandwidth / 2 + width / 2 >= fs / 2:
        raise ValueError(f"a {f0:g} Hz notch does not fit below fs/2 = {fs / 2:g} Hz: on this axis the band is already "
                         "gone (the resampler's low-pass has removed it)")
    if f0 - bandwidth / 2 - width / 2 <= 0:
        raise ValueError(f"a {f0:g} Hz notch {bandwidth:g} Hz wide reaches DC: use highpass")
    hi, lo = lowpass(fs, f0 + bandwidth / 2, width, atten), lowpass(fs, f0 - bandwidth / 2, width, atten)
    n = max(len(hi), len(lo))
    band = np.zeros(n, dtype=np.float64)
    for h, sign in ((hi, 1.0), (lo, -1.0)):         # the shorter one zero-padded to the centre
        pad = (n - len(h)) // 2
        band[pad:pad + len(h)] += sign * h
    return _delta_minus(band)


def cascade(*hs):
    """The stages applied one after the other as ONE symmetric FIR (lengths add): convolution, then symmetrised exactly."""
    if not hs:
        raise ValueError("cascade of nothing")
    c = np.asarray(hs[0], dtype=np.float64)
    for h in hs[1:]:
        c = np.convolve(c, np.asarray(h, dtype=np.float64))
    return (c + c[::-1]) / 2


class FilterSpec:
    """What to remove, independent of the sampling rate: taps(fs) designs it for an axis.

    highpass: cutoff in Hz (default 0.5: baseline wander), or None; notch: mains frequency in Hz (50 or 60), or None;
    lowpass: cutoff in Hz, or None.  width: transition width in Hz for every stage; None (default) takes 0.5 Hz for the
    high-pass, 1 Hz for the notch (2 Hz wide) and a fifth of the cutoff for the low-pass.  atten: stop-band attenuation
    and pass-band ripple in dB (Kaiser's formula is approximate: the designs reach about 53 dB at atten=60)."""

    def __init__(self, highpass=0.5, notch=None, lowpass=None, width=None, atten=60.0):
        self.highpass, self.notch, self.lowpass, self.width, self.atten = highpass, notch, lowpass, width, float(atten)
        if highpass is None and notch is None and lowpass is None:
            raise ValueError("FilterSpec with no stage")

    def taps(self, fs):
        """-> h float64 (odd length, symmetric exactly) for an axis sampled at fs Hz."""
        if fs is None:
            raise ValueError("FilterSpec needs the sampling rate of the axis it filters (fs, or model_fs when resampled)")
        w = self.width
        stages = []
        if self.highpass is not None:
            stages.append(highpass(fs, self.highpass, 0.5 if w is None else w, self.atten))
        if self.notch is not None:
            stages.append(notch(fs, self.notch, 2.0, 1.0 if w is None else w, self.atten))
        if self.lowpass is not None:
            stages.append(lowpass(fs, self.lowpass, self.lowpass / 5 if w is None else w, self.atten))
        return cascade(*stages)

    def __repr__(self):
        return (f"FilterSpec(highpass={self.highpass}, notch={self.notch}, lowpass={self.lowpass}, width={self.width}, "
                f"atten={self.atten:g})")


class OneSided(np.ndarray):
    """What one_sided returns: float32 [half+1], marked so that fir_windows does not take it for a full filter."""


def one_sided(h):
    """Full symmetric taps h [2*half+1] -> c float32 [half+1], c[i] = float32(h[half+i]): the kernel's operand.
    ValueError unless the length is odd, the fp32 taps are symmetric exactly, all finite, and half <= MAX_HALF."""
    if isinstance(h, OneSided):
        return h
    h = np.asarray(h)
    if h.ndim != 1 or h.size % 2 == 0:
        raise ValueError(f"a zero-phase FIR has an odd number of taps; got shape {h.shape}")
    half = h.size // 2
    if half > MAX_HALF:
        raise ValueError(f"half={half} exceeds {MAX_HALF} (the filter has {h.size} taps)")
    h32 = h.astype(np.float32)
    if not np.isfinite(h32).all():
        raise ValueError("taps must be finite")
    if not np.array_equal(h32, h32[::-1]):
        raise ValueError("taps are not symmetric: only zero-phase (symmetric) filters are supported")
    return np.ascontiguousarray(h32[half:]).view(OneSided)


_MAX_CACHED = 32
_cache = OrderedDict()      # (taps' bytes, device) -> tensor [half+1]


def device_one_sided(taps, device):
    """-> (c fp32 tensor [half+1] on `device`, half) for full symmetric taps or a one_sided result; uploaded once per
    (taps' bytes, device) and kept (the last 32, at most 16 KB each)."""
    import torch
    c = one_sided(taps)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (c.tobytes(), device)
    t = _cache.get(key)
    if t is None:
        t = _cache[key] = torch.from_numpy(np.array(c, dtype=np.float32)).to(device)
        if len(_cache) > _MAX_CACHED:
            _cache.popitem(last=False)
    else:
        _cache.move_to_end(key)
    return t, c.size - 1
