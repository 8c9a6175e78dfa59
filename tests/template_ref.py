"""numpy restatement of the beat-morphology entry points (include/ecg_hip.h: ecg_beats_sum, ecg_beats_match,
ecg_beats_series_mean), of ecg_hip/template.py and of score_recording's template stage — TEST INFRASTRUCTURE ONLY.

Written from the definitions, not from the kernels: no slabs of workgroups, no staging, no atomics.  The gathers are
vectorised per recording (an index array [beats, Lseg] — what the kernels exist to avoid) so that the GPU tests can afford
them; tests/test_template_host.py checks every function against literal per-element loops.  The slab of the series mean's
summation order is an argument: the GPU tests read it from the library query.
"""
import numpy as np

INVALID = -32768
FIELDS = ("n", "sum_v", "sum_vv", "sum_t", "sum_tt", "sum_vt", "sad")


def _round(x):
    return int(np.floor(x + 0.5))


def params(fs, pre_s=0.25, post_s=0.45, match_pre_s=0.08, match_post_s=0.12, max_lag_s=0.03):
    return dict(pre=_round(pre_s * fs), post=_round(post_s * fs), match_pre=_round(match_pre_s * fs),
                match_post=_round(match_post_s * fs), J=max(1, _round(max_lag_s * fs)))


def listed(pos, n, include, r):
    """Indices i of row r with i < n[r], pos >= 0 and include != 0, ascending."""
    pos = np.asarray(pos)
    cap = pos.shape[1]
    i = np.arange(min(max(int(n[r]), 0), cap))
    keep = pos[r, i] >= 0
    if include is not None:
        keep &= np.asarray(include)[r, i] != 0
    return i[keep]


def taking(pos, n, include, r, pre, post, Ttot):
    """The listed entries of row r whose segment [x - pre, x + post] is whole, ascending."""
    i = listed(pos, n, include, r)
    x = np.asarray(pos)[r, i].astype(np.int64)
    return i[(x - pre >= 0) & (x + post < Ttot)]


def sums(d, pos, n, pre, post, include=None):
    """-> (sum int64 [R, Lseg, leads], cnt int32 [R, Lseg, leads])."""
    d = np.asarray(d)
    R, Ttot, leads = d.shape
    L = pre + post + 1
    s, c = np.zeros((R, L, leads), np.int64), np.zeros((R, L, leads), np.int32)
    for r in range(R):
        x = np.asarray(pos)[r, taking(pos, n, include, r, pre, post, Ttot)].astype(np.int64)
        for a in range(0, len(x), 4096):
            seg = d[r][x[a:a + 4096, None] - pre + np.arange(L)[None, :]].astype(np.int64)     # [beats, L, leads]
            valid = seg != INVALID
            s[r] += np.where(valid, seg, 0).sum(0)
            c[r] += valid.sum(0).astype(np.int32)
    return s, c


def fields(v, t):
    """The seven integers of one lead: v, t int64 [Lseg]."""
    both = (v != INVALID) & (t != INVALID)
    v, t = v[both], t[both]
    return [int(both.sum()), int(v.sum()), int((v * v).sum()), int(t.sum()), int((t * t).sum()), int((v * t).sum()),
            int(np.abs(v - t).sum())]


def match(d, pos, n, tmpl, pre, post, J, lead_mask=None, include=None):
    """-> (lag int32 [R, cap], m int64 [R, cap, leads, 7])."""
    d, pos, tmpl = np.asarray(d), np.asarray(pos), np.asarray(tmpl).astype(np.int64)
    R, Ttot, leads = d.shape
    cap, L = pos.shape[1], pre + post + 1
    take = np.array([lead_mask is None or bool((lead_mask >> l) & 1) for l in range(leads)])
    lag, m = np.zeros((R, cap), np.int32), np.zeros((R, cap, leads, 7), np.int64)
    for r in range(R):
        tv = tmpl[r] != INVALID
        for i in listed(pos, n, include, r):
            x = int(pos[r, i])
            best = None
            for j in range(-J, J + 1):
                if x + j - pre < 0 or x + j + post >= Ttot:
                    continue
                seg = d[r, x + j - pre:x + j + post + 1].astype(np.int64)
                score = int(np.where((seg != INVALID) & tv & take[None, :], seg * tmpl[r], 0).sum())
                if best is None or score > best[0]:
                    best = (score, j, seg)
            if best is None:
                continue
            lag[r, i] = best[1]
            for l in range(leads):
                m[r, i, l] = fields(best[2][:, l], tmpl[r][:, l])
    return lag, m


def series_index(s, up, down, Tx):
    return np.minimum(Tx - 1, (np.asarray(s, np.int64) * up) // down)


def series_mean(x, pos, n, Ttot, pre, post, up, down, slab, include=None):
    """x fp32 [R, K, Tx] -> (out fp32 [R, K, Lseg], count int32 [R]); every add a float32 add, in the stated order."""
    x, pos = np.asarray(x, np.float32), np.asarray(pos)
    R, K, Tx = x.shape
    cap, L = pos.shape[1], pre + post + 1
    out, count = np.zeros((R, K, L), np.float32), np.zeros(R, np.int32)
    t = np.arange(L)
    with np.errstate(invalid="ignore"):
        for r in range(R):
            tk = taking(pos, n, include, r, pre, post, Ttot)
            count[r] = len(tk)
            total = np.zeros((K, L), np.float32)
            for b in range(-(-cap // slab)):
                partial = np.zeros((K, L), np.float32)
                for i in tk[(tk >= b * slab) & (tk < (b + 1) * slab)]:
                    partial = partial + x[r][:, series_index(int(pos[r, i]) - pre + t, up, down, Tx)]
                total = total + partial
            if count[r]:
                out[r] = total / np.float32(count[r])
    return out, count


# ---------------------------------------------------------------------------------------------------------------------
# ecg_hip/template.py
# ---------------------------------------------------------------------------------------------------------------------
def mean_template(s, c, centre=False):
    s, c = np.asarray(s, np.int64), np.asarray(c, np.int64)
    have = c > 0
    t = np.where(have, (2 * s + c) // np.where(have, 2 * c, 1), 0)
    if centre:
        k = have.sum(1, keepdims=True)
        t = t - t.sum(1, keepdims=True) // np.where(k > 0, k, 1)
    return np.where(have, np.clip(t, -32767, 32767), INVALID).astype(np.int16)


def correlation(m):
    m = np.asarray(m, np.int64)
    n, sv, svv, st, stt, svt = (m[..., k] for k in range(6))
    num, fv, ft = n * svt - sv * st, n * svv - sv * sv, n * stt - st * st
    good = (n >= 2) & (fv != 0) & (ft != 0)
    den = np.sqrt(np.where(good, fv, 1).astype(np.float64) * np.where(good, ft, 1).astype(np.float64))
    return np.where(good, num.astype(np.float64) / den, np.nan)


def beat_correlation(m, lead_mask=None):
    c = correlation(m)
    out = np.full(c.shape[:-1], np.nan)
    for at in np.ndindex(*c.shape[:-1]):
        v = sorted(x for l, x in enumerate(c[at]) if (lead_mask is None or (lead_mask >> l) & 1) and not np.isnan(x))
        if v:
            out[at] = v[(len(v) - 1) // 2]
    return out


def physical(t, gain, baseline):
    t = np.asarray(t)
    leads = t.shape[-1]
    out = (t.astype(np.float64) - np.asarray(baseline, np.float64).reshape(-1, 1, leads)) / np.asarray(gain, np.float64).reshape(-1, 1, leads)
    return np.where(t == INVALID, np.nan, out)


def stage(d, gain, baseline, beats, n_beats, p, min_corr=0.6, passes=2, lead_mask=None, cam=None, cover=None, up=1, down=1,
          slab=None):
    """score_recording's template stage on the beat list (beats, n_beats): -> dict of its fields as numpy arrays."""
    d, beats = np.asarray(d), np.asarray(beats, np.int32)
    Ttot = d.shape[1]
    pos, ok = beats, None
    for _ in range(passes):
        s, c = sums(d, pos, n_beats, p["match_pre"], p["match_post"], ok)
        tm = mean_template(s, c, centre=True)
        lag, m = match(d, beats, n_beats, tm, p["match_pre"], p["match_post"], p["J"], lead_mask)
        corr = beat_correlation(m, lead_mask)
        with np.errstate(invalid="ignore"):
            pos, ok = beats + lag, corr >= min_corr
    s, c = sums(d, pos, n_beats, p["pre"], p["post"], ok)
    out = dict(beat_pos=pos, beat_lag=lag, beat_ok=ok, beat_corr=corr, template_n=c, match_template=tm,
               template=physical(mean_template(s, c), gain, baseline), template_offsets=tuple(range(-p["pre"], p["post"] + 1)))
    if cam is not None:
        cover = np.asarray(cover)
        Tx = cam.shape[-1]
        inc = ok.copy()
        for r, i in zip(*np.nonzero(ok)):
            # the mapped range: every series sample from the image of x - pre to the image of x + post
            lo = int(series_index(max(0, int(pos[r, i]) - p["pre"]), up, down, Tx))
            hi = int(series_index(max(0, int(pos[r, i]) + p["post"]), up, down, Tx))
            inc[r, i] = not (cover[lo:hi + 1] == 0).any()
        out["cam_include"] = inc
        out["cam_beat"], out["cam_beat_n"] = series_mean(cam, pos, n_beats, Ttot, p["pre"], p["post"], up, down, slab, inc)
    return out
