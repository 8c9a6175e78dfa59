"""Signal-quality gate for recordings: which windows of a continuous recording can be trusted.

`functional.wfdb16_quality` (ecg_wfdb16_quality, csrc/quality.hip) reads the raw int16 stream in place and writes, for every
(recording, window, lead), the ten exact integers named in FIELDS.  `QualitySpec.judge` turns that small table into
`lead_ok [R, W, leads]` and `usable [R, W]` with plain torch ops, and `score_recording(..., quality=)` keeps the unusable
windows out of prob_max / prob_mean.  The indices are taken from the RAW stream, on the SOURCE axis: before resampling and
before `filter=`, because a filter hides exactly the defects this stage looks for (a high-pass turns a rail into a decaying
transient, a resampler smooths a flat line's ends).
"""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

FIELDS = ("n_invalid", "vmin", "vmax", "sum", "sumsq", "flat_run", "n_rail", "n_pairs", "sum_step", "max_step")
(N_INVALID, VMIN, VMAX, SUM, SUMSQ, FLAT_RUN, N_RAIL, N_PAIRS, SUM_STEP, MAX_STEP) = range(10)


def tile():
    """Source samples per LDS tile of the kernel: a longer window takes more than one pass of its tile loop."""
    from . import _lib as L
    return int(L.query("ecg_wfdb16_quality_tile"))


def source_span(window, Ttot, up=1, down=1):
    """Tq: source samples under one model window of `window` samples, min(Ttot, ceil(window*down/up))."""
    return min(int(Ttot), -((-int(window) * int(down)) // int(up)))


@dataclass(frozen=True)
class QualitySpec:
    """Thresholds that turn the quality table into lead_ok / usable.  A lead of a window is BAD when any of these holds
    (None turns a criterion off):
        flat_s        flat_run >= ceil(flat_s * fs)           a flat line (electrode off) of flat_s seconds or more
        rail_frac     n_rail > rail_frac * Tq                 more than this share of the samples on an ADC rail
        p2p_min_mv    (vmax - vmin) / gain < p2p_min_mv       no signal at all (also a lead with no valid sample)
        p2p_max_mv    (vmax - vmin) / gain > p2p_max_mv       a motion artefact or an amplifier swinging rail to rail
        step_max_mv   max_step / gain > step_max_mv           a jump between neighbouring samples (off by default)
        invalid_frac  n_invalid > invalid_frac * Tq           more than this share of invalid (-32768) samples
    and a window is usable while at most max_bad_leads of its leads are bad.

    The defaults are POLICY, not measurements: they are ordinary values from the signal-quality literature, and no
    labelled data was available to tune them.  Set them for your recordings."""
    flat_s: Optional[float] = 0.5
    rail_frac: Optional[float] = 0.01
    p2p_min_mv: Optional[float] = 0.05
    p2p_max_mv: Optional[float] = 10.0
    step_max_mv: Optional[float] = None
    invalid_frac: Optional[float] = 0.0
    max_bad_leads: int = 0

    def judge(self, q, gain, fs=None, Tq=None):
        """q int64 [R, W, leads, 10] (functional.wfdb16_quality), gain [leads] or [R, leads] in counts per mV, fs the
        SOURCE sampling rate (the indices live on the source axis), Tq the source samples per window (the table does
        not carry it) -> (lead_ok [R, W, leads] bool, usable [R, W] bool), on q's device.
        ValueError when flat_s is set and fs is None, or a share (rail_frac, invalid_frac) is set and Tq is None."""
        import torch
        if q.dim() != 4 or q.shape[-1] != len(FIELDS):
            raise ValueError(f"judge: q must be [R, W, leads, {len(FIELDS)}], got {tuple(q.shape)}")
        if self.flat_s is not None and fs is None:
            raise ValueError("judge: flat_s is in seconds and needs the sampling rate fs of the source stream")
        if (self.rail_frac is not None or self.invalid_frac is not None) and Tq is None:
            raise ValueError("judge: rail_frac / invalid_frac are shares of the window and need its length Tq")
        R, _, leads, _ = q.shape
        g = torch.as_tensor(gain, dtype=torch.float64).to(q.device).reshape(-1, leads).expand(R, leads)[:, None, :]
        bad = torch.zeros(q.shape[:3], dtype=torch.bool, device=q.device)
        if self.flat_s is not None:
            bad |= q[..., FLAT_RUN] >= math.ceil(self.flat_s * fs)
        if self.rail_frac is not None:
            bad |= q[..., N_RAIL].double() > self.rail_frac * Tq
        p2p = (q[..., VMAX] - q[..., VMIN]).double() / g
        if self.p2p_min_mv is not None:
            bad |= p2p < self.p2p_min_mv
        if self.p2p_max_mv is not None:
            bad |= p2p > self.p2p_max_mv
        if self.step_max_mv is not None:
            bad |= q[..., MAX_STEP].double() / g > self.step_max_mv
        if self.invalid_frac is not None:
            bad |= q[..., N_INVALID].double() > self.invalid_frac * Tq
        return ~bad, bad.sum(-1) <= int(self.max_bad_leads)


def rails_from_header(signals):
    """The ADC rails of each signal, (lo, hi) int32 [n], in the decoded int16 domain: a valid sample v counts as railed
    when v <= lo or v >= hi.  signals: the signal dicts of wfdb16.parse_header.  With adc_res > 0 in the header the rails
    are adc_zero - 2^(adc_res-1) and adc_zero + 2^(adc_res-1) - 1; otherwise the range of the storage format: 12 bits for
    212, 8 for 80, 16 for the others."""
    lo, hi = [], []
    for s in signals:
        res, zero = int(s.get("adc_res") or 0), int(s.get("adc_zero") or 0)
        if res <= 0:
            res, zero = {212: 12, 80: 8}.get(int(s["fmt"]), 16), 0
        lo.append(zero - (1 << (res - 1)))
        hi.append(zero + (1 << (res - 1)) - 1)
    i32 = np.iinfo(np.int32)
    return tuple(np.clip(np.asarray(v, np.int64), i32.min, i32.max).astype(np.int32) for v in (lo, hi))
