"""Beat morphology for recordings: the aligned mean beat, how well every beat matches it, and the beat-locked mean of the
stitched CAM.

`functional.beats_sum` (ecg_beats_sum, csrc/beat_template.hip) adds the segments of the raw int16 stream around a list of
positions, `functional.beats_match` (ecg_beats_match) finds every beat's best lag against a template and takes seven exact
integers per (beat, lead) at that lag, named in FIELDS, and `functional.beats_series_mean` (ecg_beats_series_mean) averages
fp32 series that live on a related axis — the stitched Grad-CAM — over the beats.  This module holds what turns those
integers into a template, a correlation and a verdict with plain torch ops, and `score_recording(..., template=)` puts all
of it beside the beat list.  The definitions are in include/ecg_hip.h.

A beat index of ecg_wfdb16_beats is the peak of the integrated slope sum, a few samples from the R apex — at 100 Hz a QRS
is about three samples wide, and averaging or correlating at the raw indices smears the complex away.  So alignment is part
of the stage: every beat is moved by its best lag within +-max_lag_s against a centred mean template, twice.  The aligned
positions are still slope-sum peaks moved onto a common phase of the mean beat, NOT R apices.
"""
from dataclasses import dataclass
from typing import Optional, Sequence

FIELDS = ("n", "sum_v", "sum_vv", "sum_t", "sum_tt", "sum_vt", "sad")
(N, SUM_V, SUM_VV, SUM_T, SUM_TT, SUM_VT, SAD) = range(7)
INVALID = -32768


def slab():
    """List entries per slab of the series mean's summation order (ecg_beats_slab)."""
    from . import _lib as L
    return int(L.query("ecg_beats_slab"))


@dataclass(frozen=True)
class TemplateSpec:
    """The stage's parameters in physical units; `.params(fs)` turns them into the integers of the ABI.
        pre_s, post_s              the displayed mean beat (and the beat-locked CAM) covers [-pre_s, +post_s] around a beat
        match_pre_s, match_post_s  the range the template is matched over: the QRS complex and its flanks
        max_lag_s                  a beat may move by at most this much to its best lag (at least one sample)
        passes                     times the (sum, centre, match) round is run; the second uses the first's lags and verdicts
        min_corr                   a beat is `ok` iff its correlation with the template is at least this
        leads                      indices of the leads taking part in the score and the verdict (None: all)

    The defaults are POLICY, not measurements: a display range that holds P wave to T wave at ordinary rates, a match range
    of 200 ms around the complex, 30 ms of lag and a correlation of 0.6, checked on synthetic recordings only (normal beats
    >= 0.87, planted wide beats <= 0.22 at 100, 250 and 500 Hz: tests/test_template_host.py); no annotated data was available to tune them.  Set them
    for your recordings."""
    pre_s: float = 0.25
    post_s: float = 0.45
    match_pre_s: float = 0.08
    match_post_s: float = 0.12
    max_lag_s: float = 0.03
    passes: int = 2
    min_corr: float = 0.6
    leads: Optional[Sequence[int]] = None

    def lead_mask(self, leads):
        """Bit l set = lead l takes part."""
        if self.leads is None:
            return (1 << int(leads)) - 1
        mask = 0
        for l in self.leads:
            if not 0 <= int(l) < int(leads):
                raise ValueError(f"TemplateSpec.leads: lead {l} outside the stream's {leads} leads")
            mask |= 1 << int(l)
        if not mask:
            raise ValueError("TemplateSpec.leads selects no lead")
        return mask

    def params(self, fs):
        """fs: the SOURCE sampling rate -> dict(pre, post, match_pre, match_post, J): ints, in source samples."""
        from .beats import _round
        return dict(pre=_round(self.pre_s * fs), post=_round(self.post_s * fs), match_pre=_round(self.match_pre_s * fs),
                    match_post=_round(self.match_post_s * fs), J=max(1, _round(self.max_lag_s * fs)))


def mean_template(sum, cnt, centre=False):
    """sum int64, cnt int32 [R, L, leads] (functional.beats_sum) -> the mean beat as int16 [R, L, leads]:
    floor((2*sum + cnt) / (2*cnt)) in int64 — the mean rounded half up — clamped to +-32767, and -32768 ("no value") where
    cnt == 0.  centre=True subtracts from every (recording, lead) the floor-mean of its valid samples (before the clamp):
    a template for matching, whose score must not reward a beat for sitting on the same baseline."""
    import torch
    c = cnt.to(torch.int64)
    have = c > 0
    safe = torch.where(have, c, torch.ones_like(c))
    t = torch.div(2 * sum + c, 2 * safe, rounding_mode="floor")
    t = torch.where(have, t, torch.zeros_like(t))
    if centre:
        k = have.sum(1, keepdim=True)
        mean = torch.div(t.sum(1, keepdim=True), torch.where(k > 0, k, torch.ones_like(k)), rounding_mode="floor")
        t = t - mean
    t = t.clamp(-32767, 32767)
    return torch.where(have, t, torch.full_like(t, INVALID)).to(torch.int16)


def correlation(m):
    """m int64 [..., 7] (functional.beats_match) -> Pearson's r of segment and template per (beat, lead), float64 [...]:
    (N*Svt - Sv*St) / sqrt((N*Svv - Sv^2) * (N*Stt - St^2)), the numerator and both factors taken exactly in int64 (they
    stay below 2^50) before the conversion to float64; NaN where N < 2 or a factor is 0."""
    import torch
    n, sv, svv, st, stt, svt = (m[..., k] for k in (N, SUM_V, SUM_VV, SUM_T, SUM_TT, SUM_VT))
    num, fv, ft = n * svt - sv * st, n * svv - sv * sv, n * stt - st * st
    good = (n >= 2) & (fv != 0) & (ft != 0)
    den = torch.sqrt(torch.where(good, fv, torch.ones_like(fv)).double() * torch.where(good, ft, torch.ones_like(ft)).double())
    return torch.where(good, num.double() / den, torch.full_like(den, float("nan")))


def beat_correlation(m, lead_mask=None):
    """One number per beat, float64 [R, cap]: the LOWER median of correlation(m) over the leads of lead_mask (None: all)
    whose value is not NaN; NaN where there is none."""
    import torch
    c = correlation(m)
    leads = c.shape[-1]
    take = [l for l in range(leads) if lead_mask is None or (int(lead_mask) >> l) & 1]
    if len(take) != leads:
        c = torch.stack([c[..., l] for l in take], -1)      # column by column: no index tensor travels to the device
    return torch.nanmedian(c, dim=-1).values


def physical(template, gain, baseline):
    """An int16 template [R, L, leads] -> mV as float64, (t - baseline) / gain per (recording, lead); NaN where the
    template has no value (-32768).  For a centred template pass baseline=0."""
    import torch
    gain = torch.as_tensor(gain, dtype=torch.float64, device=template.device).reshape(-1, 1, template.shape[-1])
    base = torch.as_tensor(baseline, device=template.device).to(torch.float64)
    base = base.reshape(-1, 1, template.shape[-1]) if base.dim() else base
    out = (template.to(torch.float64) - base) / gain
    return torch.where(template == INVALID, torch.full_like(out, float("nan")), out)
