"""numpy restatement of the signal-quality indices (include/ecg_hip.h, ecg_wfdb16_quality) — TEST INFRASTRUCTURE ONLY.

Plain loops over recordings, windows, leads and samples, Python ints throughout: every field is written as its definition
reads, not as the kernel computes it (no tiles, no segment summaries, no merging).  Includes the window rule and the
source-span rule a_w = min(floor(s_w*down/up), Ttot - Tq), Tq = min(Ttot, ceil(T*down/up)).
"""
import numpy as np

FIELDS = ("n_invalid", "vmin", "vmax", "sum", "sumsq", "flat_run", "n_rail", "n_pairs", "sum_step", "max_step")
INVALID = -32768


def starts(first, hop, W, last_start):
    """The model-axis start of every window of the shared window rule."""
    return [last_start if (last_start >= 0 and w == W - 1) else first + w * hop for w in range(W)]


def span(T, Ttot, up=1, down=1):
    """Tq: source samples under one model window."""
    return min(Ttot, (T * down + up - 1) // up)


def source_starts(Ttot, T, first, hop, W, last_start, up=1, down=1):
    Tq = span(T, Ttot, up, down)
    return [min(s * down // up, Ttot - Tq) for s in starts(first, hop, W, last_start)], Tq


def row(v, lo=-32767, hi=32767):
    """The ten fields of one lead of one window: v is the sequence of its raw int16 samples."""
    v = [int(x) for x in v]
    valid = [x for x in v if x != INVALID]
    flat = run = 1
    for i in range(1, len(v)):
        run = run + 1 if v[i] == v[i - 1] else 1
        flat = max(flat, run)
    steps = [abs(v[i + 1] - v[i]) for i in range(len(v) - 1) if v[i] != INVALID and v[i + 1] != INVALID]
    return [len(v) - len(valid),
            min(valid) if valid else 32767,
            max(valid) if valid else -32768,
            sum(valid),
            sum(x * x for x in valid),
            flat,
            sum(1 for x in valid if x <= lo or x >= hi),
            len(steps),
            sum(steps),
            max(steps) if steps else 0]


def table(d, T, first, hop, W, last_start=-1, up=1, down=1, rails=None):
    """d int16 [R, Ttot, leads] -> int64 [R, W, leads, 10]; rails: (lo, hi) integer [R, leads], None: (-32767, 32767)."""
    d = np.asarray(d)
    R, Ttot, leads = d.shape
    a, Tq = source_starts(Ttot, T, first, hop, W, last_start, up, down)
    q = np.zeros((R, W, leads, len(FIELDS)), np.int64)
    for r in range(R):
        for w in range(W):
            for c in range(leads):
                lo, hi = (-32767, 32767) if rails is None else (int(rails[0][r][c]), int(rails[1][r][c]))
                q[r, w, c] = row(d[r, a[w]:a[w] + Tq, c], lo, hi)
    return q
