"""Host-side checks of the continuous-recording path: the window rule (ecg_hip.recording.window_plan), the argument
checks of the two entry points behind it (no launch, no device), and the numpy statement of the overlap mean that the
GPU test compares ecg_windows_overlap_mean against."""
import ctypes
import itertools
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from ecg_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# window rule
# ---------------------------------------------------------------------------------------------------------------------
def test_window_plan_properties():
    from ecg_hip.recording import window_plan
    n = 0
    for Ttot, window, hop, tail in itertools.product((1, 63, 100, 700, 1000, 3000, 4100), (1, 63, 100, 256, 1000),
                                                     (1, 7, 100, 250, 333, 1000, 5000), ("shift", "drop")):
        if Ttot < window:
            with pytest.raises(ValueError):
                window_plan(Ttot, window, hop, tail)
            continue
        first, hop_, W, last_start, starts = window_plan(Ttot, window, hop, tail)
        n += 1
        assert hop_ == hop and W == len(starts) >= 1
        assert all(b > a for a, b in zip(starts, starts[1:])), "starts strictly increasing"
        assert all(0 <= s <= Ttot - window for s in starts)
        # the starts are what the C ABI derives from (first, hop, W, last_start)
        rule = [last_start if (last_start >= 0 and w == W - 1) else first + w * hop for w in range(W)]
        assert list(starts) == rule
        exact = (Ttot - window) % hop == 0
        covers_end = starts[-1] + window == Ttot
        if tail == "shift":
            assert covers_end and (last_start >= 0) == (not exact)
        else:
            assert last_start == -1 and covers_end == exact          # the remainder is dropped whole, never cut
            assert W == (Ttot - window) // hop + 1
        if Ttot == window:
            assert W == 1 and starts == (0,)
    assert n > 100
    with pytest.raises(ValueError):
        window_plan(100, 10, 0)
    with pytest.raises(ValueError):
        window_plan(100, 10, 5, tail="pad")


def test_plan_chunks_cover_every_window_once():
    from ecg_hip.recording import plan_chunks, window_plan
    for R, Ttot, window, hop, bs in ((1, 3000, 1000, 500, 4), (3, 700, 256, 100, 4), (5, 700, 256, 100, 13), (2, 1000, 1000, 7, 1),
                                     (1, 3001, 1000, 500, 5), (1, 3001, 1000, 500, 6)):
        plan = window_plan(Ttot, window, hop)
        _, _, W, last_start, starts = plan
        seen = []
        for r0, r1, w0, first, Wc, last in plan_chunks(R, plan, bs):
            assert (r1 - r0) * Wc <= bs and Wc >= 1
            st = [last if (last >= 0 and w == Wc - 1) else first + w * hop for w in range(Wc)]
            seen += [(r, w0 + i, s) for r in range(r0, r1) for i, s in enumerate(st)]
        assert sorted(seen) == [(r, w, starts[w]) for r in range(R) for w in range(W)]


# ---------------------------------------------------------------------------------------------------------------------
# C ABI: rejected on the host, before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_validate_before_launch(lib):
    assert lib.ecg_version() == 100
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)            # a non-null dummy: nothing may dereference it

    def windows(R=1, Ttot=700, leads=12, T=256, first=0, hop=100, W=5, last_start=-1, d=p):
        return lib.ecg_wfdb16_windows(d, p, p, p, p, R, Ttot, leads, T, first, hop, W, last_start, None)

    def overlap(R=1, K=2, T=256, Ttot=700, first=0, hop=100, W=5, last_start=-1, v=p):
        return lib.ecg_windows_overlap_mean(v, p, p, R, K, T, Ttot, first, hop, W, last_start, None)

    for fn in (windows, overlap):
        for bad, text in ((dict(hop=0), b"hop"), (dict(T=701), b"longer than the recording"),
                          (dict(W=6), b"past Ttot-T"),                     # 0 + 5*100 + 256 > 700
                          (dict(W=6, last_start=445), b"last_start"),      # > Ttot - T = 444
                          (dict(W=0), b"W=0"), (dict(first=-1), b"first")):
            assert fn(**bad) == 1, (fn.__name__, bad)                      # ECG_EINVAL
            assert text in lib.ecg_last_error(), (fn.__name__, bad, lib.ecg_last_error())
    assert windows(leads=17) == 1 and b"leads" in lib.ecg_last_error()
    assert windows(leads=0) == 1 and b"leads" in lib.ecg_last_error()
    assert windows(d=None) == 1 and b"null pointer" in lib.ecg_last_error()
    assert overlap(v=None) == 1 and b"null pointer" in lib.ecg_last_error()
    assert overlap(K=0) == 1 and b"K=0" in lib.ecg_last_error()
    assert windows(R=20000, W=5) == 1 and b"grid.y" in lib.ecg_last_error()
    assert overlap(R=40000, K=2) == 1 and b"grid.y" in lib.ecg_last_error()
    # a long window streams per (window, lead) row: the row limit is checked before the first launch too
    assert windows(R=1200, Ttot=8000, T=5000, hop=500, W=5) == 1 and b"rows" in lib.ecg_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the oracle of the overlap mean
# ---------------------------------------------------------------------------------------------------------------------
def overlap_mean_ref(v, starts, Ttot):
    """The definition in include/ecg_hip.h with numpy fp32: windows added in ascending w, one division by the count.
    -> (out [R][K][Ttot], cover [Ttot])."""
    R, W, K, T = v.shape
    acc = np.zeros((R, K, Ttot), np.float32)
    cover = np.zeros(Ttot, np.float32)
    for w, s in enumerate(starts):
        acc[:, :, s:s + T] = acc[:, :, s:s + T] + v[:, w]
        cover[s:s + T] += np.float32(1)
    out = np.zeros_like(acc)
    np.divide(acc, cover[None, None, :], out=out, where=(cover > 0)[None, None, :])
    return out, cover


@pytest.mark.parametrize("case", [(2, 5, 256, 700, 100, "shift"), (1, 1, 100, 900, 250, "drop")])
def test_overlap_mean_reference_matches_brute_force(case):
    from ecg_hip.recording import window_plan
    R, K, T, Ttot, hop, tail = case
    starts = window_plan(Ttot, T, hop, tail)[4]
    rng = np.random.default_rng(Ttot + hop)
    v = rng.standard_normal((R, len(starts), K, T)).astype(np.float32)
    out, cover = overlap_mean_ref(v, starts, Ttot)
    for r, k, t in itertools.product(range(R), range(K), range(Ttot)):
        acc, n = np.float32(0), 0
        for w, s in enumerate(starts):
            if s <= t < s + T:
                acc = np.float32(acc + v[r, w, k, t - s])
                n += 1
        want = np.float32(acc / np.float32(n)) if n else np.float32(0)
        assert out[r, k, t] == want and cover[t] == n, (r, k, t)
    if tail == "drop":
        assert (cover == 0).any() and (out[:, :, cover == 0] == 0).all()       # hop > T leaves gaps
