"""numpy restatement of the beat detector and the rhythm table (include/ecg_hip.h, ecg_wfdb16_beats / ecg_beats_rhythm) —
TEST INFRASTRUCTURE ONLY.

Written from the definitions, not from the kernels: no chunks, no halos, no doubling, no compaction.  It is vectorised
(cumsum for g, a strided window maximum) so that the GPU tests can afford it; tests/test_beats_host.py checks it against
a literal per-sample double loop.  Also the seeded synthetic ECG the detector-quality test and the end-to-end tests use.
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from quality_ref import source_starts

FIELDS = ("n_beats", "first_beat", "last_beat", "sum_rr_sq", "min_rr", "max_rr", "sum_drr_sq", "n_drr_over")
INVALID = -32768


def capacity(Ttot, ref):
    return (Ttot + ref) // (ref + 1)


def feature(v, s, h, lead_mask=None):
    """v int16 [Ttot, leads] of ONE recording -> (f, g) int64 [Ttot]."""
    v = np.asarray(v).astype(np.int64)
    Ttot, leads = v.shape
    take = [l for l in range(leads) if lead_mask is None or (lead_mask >> l) & 1]
    f = np.zeros(Ttot, np.int64)
    if Ttot > 2 * s:
        a, b = v[2 * s:, take], v[:Ttot - 2 * s, take]
        f[s:Ttot - s] = np.where((a != INVALID) & (b != INVALID), np.abs(a - b), 0).sum(1)
    c = np.concatenate([[0], np.cumsum(f)])
    n = np.arange(Ttot)
    g = c[np.minimum(Ttot - 1, n + h) + 1] - c[np.maximum(0, n - h)]
    return f, g


def thresholds(g, blk, num, den, g_min):
    """-> (M, thr): the block maxima and the threshold of every block, Python ints in int64 arrays."""
    Ttot = len(g)
    M = np.maximum.reduceat(g, np.arange(0, Ttot, blk))
    nblk = len(M)
    assert nblk == -(-Ttot // blk)
    thr = np.zeros(nblk, np.int64)
    for b in range(nblk):
        near = sorted(int(x) for x in M[max(0, b - 2):min(nblk, b + 3)])
        thr[b] = max(int(g_min), (num * near[(len(near) - 1) // 2]) // den)
    return M, thr


def beats(v, s, h, ref, blk, num, den, g_min, lead_mask=None):
    """The beat samples of ONE recording v int16 [Ttot, leads], ascending, as an int64 array."""
    _, g = feature(v, s, h, lead_mask)
    _, thr = thresholds(g, blk, num, den, g_min)
    Ttot = len(g)
    pad = np.concatenate([np.full(ref, -1, np.int64), g, np.full(ref, -1, np.int64)])       # out of the recording: below every g
    wmax = sliding_window_view(pad, ref).max(-1)                # wmax[i] = max pad[i : i + ref]
    left, right = wmax[:Ttot], wmax[ref + 1:ref + 1 + Ttot]    # g[n-ref .. n-1] and g[n+1 .. n+ref]
    n = np.arange(Ttot)
    return np.nonzero((g >= thr[n // blk]) & (g > left) & (g >= right))[0]


def detect(d, s, h, ref, blk, num, den, g_min, lead_mask=None):
    """d int16 [R, Ttot, leads], g_min [R] -> (beats int32 [R, cap] with -1 from n_beats[r] on, n_beats int32 [R])."""
    d = np.asarray(d)
    R, Ttot, _ = d.shape
    out, n = np.full((R, capacity(Ttot, ref)), -1, np.int32), np.zeros(R, np.int32)
    for r in range(R):
        x = beats(d[r], s, h, ref, blk, num, den, int(np.asarray(g_min).reshape(-1)[r]), lead_mask)
        out[r, :len(x)], n[r] = x, len(x)
    return out, n


def rhythm_row(x, nn_delta):
    """The eight fields of one window from the beats x inside it (ascending)."""
    x = [int(t) for t in x]
    rr = [x[i + 1] - x[i] for i in range(len(x) - 1)]
    dr = [rr[i + 1] - rr[i] for i in range(len(rr) - 1)]
    return [len(x), x[0] if x else -1, x[-1] if x else -1, sum(t * t for t in rr), min(rr) if rr else 2 ** 31 - 1,
            max(rr) if rr else 0, sum(t * t for t in dr), sum(1 for t in dr if abs(t) > nn_delta)]


def rhythm(beat_table, n_beats, Ttot, T, first, hop, W, last_start=-1, up=1, down=1, nn_delta=0):
    """beat_table [R, cap], n_beats [R] -> int64 [R, W, 8]."""
    a, Tq = source_starts(Ttot, T, first, hop, W, last_start, up, down)
    R = len(n_beats)
    out = np.zeros((R, W, len(FIELDS)), np.int64)
    for r in range(R):
        x = np.asarray(beat_table[r][:int(n_beats[r])], np.int64)
        for w in range(W):
            out[r, w] = rhythm_row(x[(x >= a[w]) & (x < a[w] + Tq)], nn_delta)
    return out


def g_min_of(floor_mv, h, gain, lead_mask=None):
    """max(1, floor(floor_mv * (2h+1) * sum of the gains of the leads taking part)) per recording, float64; gain [R, leads]."""
    gain = np.asarray(gain, np.float64).reshape(-1, np.asarray(gain).shape[-1])
    sel = np.array([1.0 if lead_mask is None or (lead_mask >> l) & 1 else 0.0 for l in range(gain.shape[1])])
    return np.maximum(1, np.floor(floor_mv * (2 * h + 1) * (gain * sel).sum(-1))).astype(np.int64)


def synth(fs, seconds, hr, jitter, noise_mv, seed):
    """A seeded synthetic 12-lead ECG at 1000 counts per mV -> (d int16 [Ttot, 12], planted R-apex samples int64).
    Per beat and lead: a Gaussian R wave of random sign, 0.3-1.5 mV, sigma 12 ms; a small opposite S wave; a T wave of
    0.1-0.4 mV, sigma 50 ms, at +280 ms; a P wave.  On top: 0.5 mV of 0.3 Hz wander, 0.05 mV of 50 Hz hum, white noise of
    noise_mv.  RR intervals are 60/hr * (1 + jitter*u), u uniform in [-1, 1]; no beat within 0.6 s of either end."""
    rng = np.random.default_rng(seed)
    Ttot, leads = int(round(fs * seconds)), 12
    t = np.arange(Ttot) / fs
    times, at = [], 0.6 + 0.2 * rng.random()
    while at < seconds - 0.6:
        times.append(at)
        at += 60.0 / hr * (1.0 + jitter * rng.uniform(-1, 1))
    sign = rng.choice([-1.0, 1.0], size=leads)
    x = np.zeros((Ttot, leads))

    def bump(center, amp, sigma):
        lo, hi = max(0, int((center - 5 * sigma) * fs)), min(Ttot, int((center + 5 * sigma) * fs) + 2)
        x[lo:hi] += amp[None, :] * np.exp(-0.5 * ((t[lo:hi, None] - center) / sigma) ** 2)

    for c in times:
        r_amp = sign * rng.uniform(0.3, 1.5, size=leads)
        bump(c, r_amp, 0.012)
        bump(c + 0.035, -0.2 * r_amp, 0.010)
        bump(c + 0.280, np.abs(sign) * rng.uniform(0.1, 0.4, size=leads), 0.050)
        bump(c - 0.160, np.full(leads, 0.1), 0.025)
    x += 0.5 * np.sin(2 * np.pi * 0.3 * t[:, None] + rng.uniform(0, 2 * np.pi, size=leads)[None, :])
    x += 0.05 * np.sin(2 * np.pi * 50.0 * t[:, None] + rng.uniform(0, 2 * np.pi, size=leads)[None, :])
    x += noise_mv * rng.standard_normal((Ttot, leads))
    d = np.clip(np.round(x * 1000.0), -32767, 32767).astype(np.int16)
    return d, np.round(np.asarray(times) * fs).astype(np.int64)
