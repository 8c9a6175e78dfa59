"""Host side of the on-device resampler: the rational ratio, the filter design against scipy, the numpy restatement
(tests/resample_ref.py) against scipy.signal.resample_poly, its fp32 form against the derived rounding bound, and the
window plan on the resampled axis."""
import numpy as np
import pytest

import resample_ref as rr

# (fs_in, fs_out): the conversions the filter's quality was recorded for
RATES = [(500, 100), (250, 500), (360, 500), (128, 500), (257, 500), (1000, 100), (360, 100), (250, 100)]


def test_rational_ratio():
    from ecg_hip.resample import rational_ratio
    assert rational_ratio(500, 100) == (1, 5)
    assert rational_ratio(250, 500) == (2, 1)
    assert rational_ratio(360, 500) == (25, 18)
    assert rational_ratio(128, 500) == (125, 32)
    assert rational_ratio(257, 500) == (500, 257)
    assert rational_ratio(500.0, 500) == (1, 1)
    with pytest.raises(ValueError):
        rational_ratio(499.7, 500)
    with pytest.raises(ValueError):
        rational_ratio(1, 1000)             # up = 1000 > 512
    with pytest.raises(ValueError):
        rational_ratio(0, 500)


@pytest.mark.parametrize("rates", RATES)
def test_design_taps_equals_scipy_firwin_and_phase_layout(rates):
    signal = pytest.importorskip("scipy.signal")
    from ecg_hip.resample import design_filter, design_taps, rational_ratio
    up, down = rational_ratio(*rates)
    h, half = design_filter(up, down)
    m = max(up, down)
    assert half == 10 * m and h.dtype == np.float64 and len(h) == 2 * half + 1
    want = signal.firwin(2 * half + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    assert np.abs(h - want).max() <= 1e-14
    g, half2 = design_taps(up, down)
    ntap = -(-(2 * half + 1) // up)
    assert half2 == half and g.dtype == np.float32 and g.shape == (up, ntap) and g.flags.c_contiguous
    for phi in range(up):
        for i in range(ntap):
            j = phi + i * up
            assert g[phi, i] == (np.float32(h[j]) if j < len(h) else 0)
    assert np.array_equal(g, rr.table(h, up).astype(np.float32))


def test_design_taps_layout_without_scipy():
    """The phase layout and the normalisation, on numpy alone (the scipy comparison above is skipped where scipy is absent)."""
    from ecg_hip.resample import design_filter, design_taps
    for up, down in ((1, 5), (25, 18), (500, 257)):
        h, half = design_filter(up, down)
        assert half == 10 * max(up, down) and abs(h.sum() - up) <= 1e-12 and np.array_equal(h, h[::-1])
        g, _ = design_taps(up, down)
        assert g.shape == (up, -(-len(h) // up))
        flat = g.T.reshape(-1)                      # [i][phi] -> j = phi + i*up
        assert np.array_equal(flat[:len(h)], h.astype(np.float32)) and not flat[len(h):].any()


def _signal(fs, seconds=3.0, extra=0):
    """A sum of sines + offset + noise, `seconds` long (+ extra samples, so that the length is no multiple of down)."""
    n = int(seconds * fs) + extra
    t = np.arange(n) / fs
    rng = np.random.default_rng(int(fs))
    return 0.3 + np.sin(2 * np.pi * 1.3 * t) + 0.5 * np.sin(2 * np.pi * 11.0 * t + 0.4) + 0.05 * rng.standard_normal(n)


@pytest.mark.parametrize("rates", RATES)
def test_float64_restatement_equals_scipy_resample_poly(rates):
    signal = pytest.importorskip("scipy.signal")
    from ecg_hip.resample import design_filter, rational_ratio, resampled_length
    up, down = rational_ratio(*rates)
    x = _signal(rates[0], extra=down + 1 if down > 1 else 1)
    assert down == 1 or len(x) % down != 0
    h, half = design_filter(up, down)
    y = rr.resample(x, rr.table(h, up), half, up, down, dtype=np.float64)
    want = signal.resample_poly(x, up, down, padtype="edge")
    assert len(y) == len(want) == resampled_length(len(x), up, down)
    assert np.abs(y - want).max() <= 1e-12


@pytest.mark.parametrize("rates", RATES)
def test_fp32_restatement_within_the_derived_bound(rates):
    """ntap products and ntap sums, each rounded once (relative 2^-24), on top of the taps' own rounding to fp32: against
    the float64 sum over the same fp32 samples the error is at most (ntap + 1) * 2^-24 * max_phi sum_i |g[phi][i]| * max|p|
    to first order."""
    from ecg_hip.resample import design_filter, design_taps, rational_ratio
    up, down = rational_ratio(*rates)
    p = _signal(rates[0], extra=3).astype(np.float32)
    h, half = design_filter(up, down)
    g32, _ = design_taps(up, down)
    y64 = rr.resample(p, rr.table(h, up), half, up, down, dtype=np.float64)
    y32 = rr.resample(p, g32, half, up, down, dtype=np.float32)
    assert y32.dtype == np.float32
    ntap = g32.shape[1]
    bound = (ntap + 1) * 2.0 ** -24 * np.abs(rr.table(h, up)).sum(axis=1).max() * np.abs(p).max()
    err = np.abs(y32.astype(np.float64) - y64).max()
    print(f"{rates}: fp32 - float64 = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_resampled_length_and_window_plan_on_the_resampled_axis():
    from ecg_hip.recording import window_plan
    from ecg_hip.resample import resampled_length
    assert resampled_length(5000, 1, 5) == 1000 and resampled_length(5001, 1, 5) == 1001
    assert resampled_length(1000, 25, 18) == 1389 and resampled_length(7, 2, 1) == 14
    assert resampled_length(2 ** 31 - 1, 500, 257) == -(-(2 ** 31 - 1) * 500 // 257)           # no 32-bit wrap
    Tout = resampled_length(6003, 1, 5)                 # 1201
    first, hop, W, last_start, starts = window_plan(Tout, 200, 101, "shift")
    assert last_start == Tout - 200 and starts[-1] + 200 == Tout and W == len(starts)
    assert all(0 <= s <= Tout - 200 for s in starts)


@pytest.mark.parametrize("rates,f0", [((500, 100), 7.0), ((360, 500), 40.0)])
def test_unit_sine_survives_the_conversion(rates, f0):
    from ecg_hip.resample import design_filter, rational_ratio
    fs_in, fs_out = rates
    up, down = rational_ratio(*rates)
    n = 3 * fs_in + 1
    x = np.sin(2 * np.pi * f0 * np.arange(n) / fs_in)
    h, half = design_filter(up, down)
    y = rr.resample(x, rr.table(h, up), half, up, down, dtype=np.float64)
    want = np.sin(2 * np.pi * f0 * np.arange(len(y)) / fs_out)
    edge = int(np.ceil(half / down)) + 1               # outputs whose filter reaches past an end of the recording
    err = np.abs(y - want)[edge:-edge].max()
    print(f"{rates} at {f0} Hz: {err:.3e}")
    assert err <= 1e-3
