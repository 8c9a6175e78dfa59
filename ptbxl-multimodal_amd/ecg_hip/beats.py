"""Beat detection for recordings: where the QRS complexes are, and the RR statistics of every window.

`functional.wfdb16_beats` (ecg_wfdb16_beats, csrc/beats.hip) reads the raw int16 stream in place and writes the sorted
list of beat samples of every recording; `functional.beats_rhythm` (ecg_beats_rhythm) turns that list into eight exact
integers per (recording, window), named in FIELDS; `summarize` turns the small table into heart rate, SDNN, RMSSD and pNN
with plain torch ops, and `score_recording(..., beats=)` puts all of it beside the logits.  The detector is stated so that
every sample decides for itself from a bounded neighbourhood, in integers (the definition is in include/ecg_hip.h): a slope
sum over the leads, a moving sum of it, a threshold from the median of block maxima, and a local-maximum rule with a
refractory radius.  Beats are taken from the RAW stream, on the SOURCE axis: before resampling and before `filter=`, for
the same reasons as the quality indices.

A beat index is the peak of the integrated slope sum g, NOT the R apex: it lies within the QRS complex, typically a few
samples from the apex, and it is consistent from beat to beat, which is what RR intervals need.
"""
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

FIELDS = ("n_beats", "first_beat", "last_beat", "sum_rr_sq", "min_rr", "max_rr", "sum_drr_sq", "n_drr_over")
(N_BEATS, FIRST_BEAT, LAST_BEAT, SUM_RR_SQ, MIN_RR, MAX_RR, SUM_DRR_SQ, N_DRR_OVER) = range(8)


def chunk():
    """Samples one workgroup of the detection kernels decides per pass (ecg_wfdb16_beats_chunk)."""
    from . import _lib as L
    return int(L.query("ecg_wfdb16_beats_chunk"))


def capacity(Ttot, ref):
    """Columns of the beat list: beats are more than `ref` samples apart, so at most (Ttot + ref) // (ref + 1) of them."""
    return (int(Ttot) + int(ref)) // (int(ref) + 1)


def _round(x):
    return int(math.floor(x + 0.5))


@dataclass(frozen=True)
class BeatSpec:
    """The detector's parameters in physical units; `.params(fs, gain)` turns them into the integers of the ABI.
        slope_s        half the span of the slope term |v[n+s] - v[n-s]|
        integ_half_s   half the width of the moving sum of the slope sum
        refractory_s   radius inside which a beat must be the (first) maximum: no two beats closer than this
        block_s        length of the blocks whose maxima set the threshold
        frac           (num, den): the threshold is num/den of the lower median of five neighbouring block maxima
        floor_mv       a beat needs a mean slope-sum term of at least this many mV per lead: the threshold never falls
                       under floor_mv * (2h+1) * sum of the gains of the leads taking part
        nn_ms          the successive-difference bound of pNN (pNN50 at 50 ms)
        leads          indices of the leads taking part (None: all)

    The defaults are POLICY, not measurements: ordinary values from the QRS-detection literature (a 120 ms integration
    window, a 250 ms refractory radius, pNN50), checked on synthetic recordings only; no annotated data was available to
    tune them.  Set them for your recordings.  slope_s = 0.01 puts a null of the slope term on 50 Hz at 100 and 500 Hz
    (2s samples are then 20 ms, one mains period, and v[n+s] - v[n-s] cancels it); at rates where slope_s * fs is not an
    integer the null moves off 50 Hz."""
    slope_s: float = 0.01
    integ_half_s: float = 0.06
    refractory_s: float = 0.25
    block_s: float = 2.0
    frac: Tuple[int, int] = (3, 8)
    floor_mv: float = 0.05
    nn_ms: float = 50.0
    leads: Optional[Sequence[int]] = None

    def lead_mask(self, leads):
        """Bit l set = lead l takes part."""
        if self.leads is None:
            return (1 << int(leads)) - 1
        mask = 0
        for l in self.leads:
            if not 0 <= int(l) < int(leads):
                raise ValueError(f"BeatSpec.leads: lead {l} outside the stream's {leads} leads")
            mask |= 1 << int(l)
        if not mask:
            raise ValueError("BeatSpec.leads selects no lead")
        return mask

    def params(self, fs, gain):
        """fs: the SOURCE sampling rate; gain float64 [leads] or [R, leads] in counts per mV -> dict(s, h, ref, blk, num,
        den, nn_delta, lead_mask, g_min): ints, and g_min an int64 tensor [R] on gain's device,
        g_min[r] = max(1, floor(floor_mv * (2h+1) * sum of gain[r, l] over the leads taking part)) in float64."""
        import torch
        gain = torch.as_tensor(gain, dtype=torch.float64)
        if gain.dim() == 1:
            gain = gain[None]
        leads = gain.shape[-1]
        mask = self.lead_mask(leads)
        h = _round(self.integ_half_s * fs)
        if mask == (1 << leads) - 1:
            total = gain.sum(-1)
        else:                                   # column by column: no index tensor has to travel to the device
            total = sum(gain[:, l] for l in range(leads) if (mask >> l) & 1)
        g_min = torch.floor(self.floor_mv * (2 * h + 1) * total).clamp_min(1.0).to(torch.int64)
        return dict(s=max(1, _round(self.slope_s * fs)), h=h, ref=_round(self.refractory_s * fs),
                    blk=_round(self.block_s * fs), num=int(self.frac[0]), den=int(self.frac[1]),
                    nn_delta=_round(self.nn_ms * fs / 1000.0), lead_mask=mask, g_min=g_min)


def heart_rate(rhythm, fs):
    """The heart_rate of summarize alone: float64 [R, W] in bpm, NaN under 2 beats."""
    import torch
    two = rhythm[..., N_BEATS] >= 2
    k, span = rhythm[..., N_BEATS].double(), (rhythm[..., LAST_BEAT] - rhythm[..., FIRST_BEAT]).double()
    return torch.where(two, 60.0 * float(fs) * (k - 1) / torch.where(two, span, torch.ones_like(span)),
                       torch.full_like(span, float("nan")))


def summarize(rhythm, fs):
    """rhythm int64 [R, W, 8] (functional.beats_rhythm), fs the SOURCE rate -> dict of float64 tensors [R, W]:
        heart_rate   bpm, 60 * fs * (k-1) / (last_beat - first_beat)
        sdnn_ms      population standard deviation of the RR intervals, sqrt(sum_rr_sq/(k-1) - mean_rr^2), in ms
        rmssd_ms     sqrt(sum_drr_sq / (k-2)), in ms
        pnn          n_drr_over / (k-2)
    NaN where a window holds fewer than 2 beats (heart_rate, sdnn_ms) or fewer than 3 (rmssd_ms, pnn)."""
    import torch
    if rhythm.dim() != 3 or rhythm.shape[-1] != len(FIELDS):
        raise ValueError(f"summarize: rhythm must be [R, W, {len(FIELDS)}], got {tuple(rhythm.shape)}")
    t = rhythm.double()
    k = t[..., N_BEATS]
    nan = torch.full_like(k, float("nan"))
    two, three = k >= 2, k >= 3
    nrr = torch.where(two, k - 1, torch.ones_like(k))
    ndr = torch.where(three, k - 2, torch.ones_like(k))
    span = torch.where(two, t[..., LAST_BEAT] - t[..., FIRST_BEAT], torch.ones_like(k))
    mean_rr = span / nrr
    var = (t[..., SUM_RR_SQ] / nrr - mean_rr * mean_rr).clamp_min(0.0)
    ms = 1000.0 / float(fs)
    return dict(heart_rate=heart_rate(rhythm, fs),
                sdnn_ms=torch.where(two, var.sqrt() * ms, nan),
                rmssd_ms=torch.where(three, (t[..., SUM_DRR_SQ] / ndr).sqrt() * ms, nan),
                pnn=torch.where(three, t[..., N_DRR_OVER] / ndr, nan))
