"""Host side of the on-device zero-phase FIR (ecg_hip/filter.py): the Kaiser designs against scipy, symmetry and the
one-sided form, the frequency response of the defaults, the fp32 restatement (tests/fir_ref.py) against the recursive
summation bound, what is refused, and what the default high-pass does to baseline drift."""
import numpy as np
import pytest

import fir_ref as fr

ATTEN = 60.0
STOP = 3 * 10 ** (-ATTEN / 20)          # 3e-3: the Kaiser formula is approximate, the designs reach 0.0014 .. 0.0022
PASS = 2 * 10 ** (-ATTEN / 20)          # 2e-3: measured deviation <= 0.0012


@pytest.mark.parametrize("fs,cutoff,width", [(100, 0.5, 0.5), (500, 0.5, 0.5), (500, 51.0, 1.0), (250, 40.0, 8.0), (360, 49.0, 1.0)])
def test_lowpass_equals_scipy_firwin(fs, cutoff, width):
    signal = pytest.importorskip("scipy.signal")
    from ecg_hip import filter as flt
    N, beta = signal.kaiserord(ATTEN, width / (fs / 2))
    assert flt.kaiserord(ATTEN, width / (fs / 2)) == (N, beta)
    N |= 1
    h = flt.lowpass(fs, cutoff, width, ATTEN)
    assert h.dtype == np.float64 and len(h) == N
    want = signal.firwin(N, cutoff, window=("kaiser", beta), fs=fs)
    assert np.abs(h - want).max() <= 1e-14
    for a in (30.0, 45.0, 60.0, 80.0):          # the three branches of Kaiser's beta
        assert flt.kaiserord(a, 0.01) == signal.kaiserord(a, 0.01)


def test_lengths_symmetry_cascade_and_one_sided():
    """numpy only: the lengths the issue states, oddness, exact symmetry after cascade, the one-sided fp32 form."""
    from ecg_hip import filter as flt
    assert len(flt.highpass(100)) == 727 and len(flt.highpass(500)) == 3627
    assert abs(flt.highpass(500).sum()) <= 1e-15 and abs(flt.lowpass(500, 0.5, 0.5).sum() - 1) <= 1e-15
    dc32 = abs(float(flt.highpass(500).astype(np.float32).astype(np.float64).sum()))
    print("DC gain of the fp32 500 Hz high-pass:", dc32)
    assert dc32 <= 1e-6
    spec = flt.FilterSpec(notch=50)
    h = spec.taps(500)
    assert len(h) == 2 * 2720 + 1 and h.dtype == np.float64
    assert np.array_equal(h, h[::-1])                                   # exactly, not to rounding
    assert np.array_equal(flt.FilterSpec().taps(100), flt.cascade(flt.highpass(100)))
    assert np.allclose(flt.FilterSpec().taps(100), flt.highpass(100), rtol=0, atol=1e-18)
    both = flt.cascade(flt.highpass(250), flt.notch(250, 50.0), flt.lowpass(250, 100.0, 10.0))
    assert len(both) % 2 == 1 and np.array_equal(both, both[::-1])
    assert len(both) == len(flt.highpass(250)) + len(flt.notch(250, 50.0)) + len(flt.lowpass(250, 100.0, 10.0)) - 2
    assert np.array_equal(flt.FilterSpec(notch=50, lowpass=100.0, width=None).taps(250)[:10],
                          flt.cascade(flt.highpass(250), flt.notch(250, 50.0), flt.lowpass(250, 100.0, 20.0))[:10])
    c = flt.one_sided(h)
    assert c.dtype == np.float32 and c.shape == (2721,) and c.flags.c_contiguous
    assert np.array_equal(c, h[2720:].astype(np.float32))
    assert flt.one_sided(c) is c                                        # marked: not taken for a full filter again
    assert np.array_equal(flt.one_sided([1.0]), np.ones(1, np.float32))
    assert np.array_equal(flt.one_sided(np.array([0.25, 0.5, 0.25])), np.array([0.5, 0.25], np.float32))
    # symmetric in float64 only to rounding, exactly after the fp32 cast: accepted
    assert flt.one_sided(np.array([0.1 + 1e-17, 0.8, 0.1])).shape == (2,)


def test_device_cache_keys_on_the_bytes_not_on_the_object():
    import torch
    from ecg_hip import filter as flt
    h = np.array([0.25, 0.5, 0.25])
    a, half = flt.device_one_sided(h, "cpu")
    b, _ = flt.device_one_sided(h.copy(), torch.device("cpu"))
    assert half == 1 and a is b and a.dtype == torch.float32 and a.tolist() == [0.5, 0.25]
    h[:] = [0.125, 0.75, 0.125]                                         # the same object, other taps
    c, _ = flt.device_one_sided(h, "cpu")
    assert c is not a and c.tolist() == [0.75, 0.125] and a.tolist() == [0.5, 0.25]
    d, _ = flt.device_one_sided(flt.one_sided(h), "cpu")
    assert d is c


def _response(h, fs, nfft=1 << 20):
    H = np.abs(np.fft.rfft(h, nfft))
    return np.arange(len(H)) * (fs / nfft), H


@pytest.mark.parametrize("fs", [100, 250, 500])
def test_frequency_response_of_the_default_highpass(fs):
    """Measured (2^20-point FFT of the float64 taps): stop band (<= 0.25 Hz) 0.00217 / 0.00219 / 0.00221 at
    fs = 100 / 250 / 500; pass band (>= 0.75 Hz) deviates from 1 by at most 0.00110 / 0.00111 / 0.00113."""
    from ecg_hip.filter import FilterSpec
    f, H = _response(FilterSpec().taps(fs), fs)
    stop, dev = H[f <= 0.25].max(), np.abs(H[f >= 0.75] - 1).max()
    print(f"high-pass at {fs} Hz: stop {stop:.5f}, pass deviation {dev:.5f}")
    assert H[0] <= 1e-12
    assert stop <= STOP and dev <= PASS


@pytest.mark.parametrize("fs,f0", [(500, 50), (500, 60), (250, 50)])
def test_frequency_response_of_the_default_notch(fs, f0):
    """Measured: within +-0.5 Hz of f0 at most 0.00135 / 0.00136 / 0.00137 for 500/50, 500/60, 250/50; outside +-1.5 Hz the
    deviation from 1 is at most 0.00109 / 0.00112 / 0.00109."""
    from ecg_hip.filter import notch
    f, H = _response(notch(fs, f0), fs)
    stop, dev = H[np.abs(f - f0) <= 0.5].max(), np.abs(H[np.abs(f - f0) >= 1.5] - 1).max()
    print(f"notch {f0} Hz at {fs} Hz: stop {stop:.5f}, pass deviation {dev:.5f}")
    assert stop <= STOP and dev <= PASS


def _ecg_like(fs, n, seed):
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    x = 2.0 * np.sin(2 * np.pi * 0.05 * t) + 0.4 * np.sin(2 * np.pi * 50.0 * t) + 0.02 * rng.standard_normal(n)
    x += 1.2 * np.exp(-0.5 * (((t * 1.2) % 1.0 - 0.5) / 0.012) ** 2)           # a QRS-like spike 72 times a minute
    return x.astype(np.float32)


@pytest.mark.parametrize("fs,spec", [(100, dict()), (500, dict(notch=50))])
def test_fp32_restatement_within_the_recursive_summation_bound(fs, spec):
    """fp32 against float64 on the SAME fp32 taps and data: a term passes through at most half+2 roundings, so
    |err[n]| <= gamma_{half+2} * sum_i |c[i]|*(|x[n-i]| + |x[n+i]|).  Worst ratio seen: 0.055 of the bound (half 363), 0.015 (half 2720)."""
    from ecg_hip.filter import FilterSpec, one_sided
    c = one_sided(FilterSpec(**spec).taps(fs))
    x = np.stack([_ecg_like(fs, 12 * fs + 7, 1), 3.0 + _ecg_like(fs, 12 * fs + 7, 2)], axis=1)    # [Ttot, 2], one offset
    y32, y64 = fr.fir(x, c, np.float32), fr.fir(x, c, np.float64)
    assert y32.dtype == np.float32 and y32.shape == x.shape
    err, bound = np.abs(y32.astype(np.float64) - y64), fr.bound(x, c)
    print(f"fs {fs}, half {len(c) - 1}: worst err/bound = {(err / bound).max():.4f}")
    assert (err <= bound).all()


def test_restatement_is_the_plain_convolution_with_held_ends():
    """The folded, clamped loop in float64 equals np.convolve of the edge-padded signal with the full taps."""
    from ecg_hip.filter import FilterSpec
    h = FilterSpec(highpass=2.0, width=4.0).taps(100)
    half = len(h) // 2
    x = _ecg_like(100, 301, 3).astype(np.float64)
    want = np.convolve(np.pad(x, half, mode="edge"), h, mode="valid")
    got = fr.fir(x, h[half:], np.float64)
    assert half > 30 and np.abs(got - want).max() <= 1e-13


def test_what_is_refused():
    from ecg_hip import filter as flt
    with pytest.raises(ValueError, match="resampler"):
        flt.notch(100, 50)
    with pytest.raises(ValueError, match="resampler"):
        flt.FilterSpec(notch=50).taps(100)
    assert len(flt.notch(250, 60)) % 2 == 1
    with pytest.raises(ValueError, match="symmetric"):
        flt.one_sided([0.25, 0.5, 0.26])
    with pytest.raises(ValueError, match="odd"):
        flt.one_sided([0.5, 0.5])
    with pytest.raises(ValueError, match="odd"):
        flt.one_sided(np.ones((3, 3)))
    with pytest.raises(ValueError, match="4096"):
        flt.one_sided(np.ones(2 * 4097 + 1))
    assert flt.one_sided(np.ones(2 * 4096 + 1)).shape == (4097,)
    with pytest.raises(ValueError, match="finite"):
        flt.one_sided([np.nan, 1.0, np.nan])
    with pytest.raises(ValueError, match="sampling rate"):
        flt.FilterSpec().taps(None)
    with pytest.raises(ValueError, match="no stage"):
        flt.FilterSpec(highpass=None)
    with pytest.raises(ValueError):
        flt.lowpass(100, 60.0, 1.0)


def test_default_highpass_removes_drift_and_keeps_the_signal():
    """A 2 mV, 0.05 Hz drift on a 1.2 Hz unit sine at 100 Hz: away from the edges (further than half = 363 samples) the
    drift is below 3e-3 of its amplitude and the sine within the pass-band deviation 2e-3.
    Measured: 0.00145 mV of the 2 mV drift is left (0.0007 of it), the sine moves by 0.0004."""
    from ecg_hip.filter import FilterSpec
    fs = 100
    h = FilterSpec().taps(fs)
    half = len(h) // 2
    t = np.arange(40 * fs) / fs
    drift, sine = 2.0 * np.sin(2 * np.pi * 0.05 * t + 0.3), np.sin(2 * np.pi * 1.2 * t)
    inner = slice(half, len(t) - half)
    left = np.abs(fr.fir(drift, h[half:], np.float64)[inner]).max()
    moved = np.abs(fr.fir(sine, h[half:], np.float64) - sine)[inner].max()
    both = np.abs(fr.fir(drift + sine, h[half:], np.float64) - sine)[inner].max()
    print(f"drift left {left:.5f} of 2.0, sine moved {moved:.5f}, together {both:.5f}")
    assert left <= STOP * 2.0 and moved <= PASS and both <= STOP * 2.0 + PASS
