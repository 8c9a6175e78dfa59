"""Scoring a continuous recording: any WFDB signal longer than one training window (a rhythm strip, a Holter export)
-> per-window logits, record-level probabilities and Grad-CAMs on the recording's own time axis.

The recording stays on the device as the int16 samples of a format-16 .dat file (records stored otherwise — format 212,
skews, several files — are decoded to that form on the device, ecg_hip.wfdbraw).  `ecg_wfdb16_windows` cuts the z-scored windows
straight out of it (no overlapping copy), the windows go through the model's eval forward (or `ecg_hip.grad_cam`) in chunks
of at most `batch_size`, and `ecg_windows_overlap_mean` averages the per-window CAMs where windows overlap.

Window rule (shared with the C ABI): window w starts at sample first + w*hop; with tail="shift" a recording whose length
is not first + k*hop + window gets one more window that ENDS with the recording (start Ttot - window), so that every
sample is scored; tail="drop" leaves the remainder unscored.

A recording sampled at another rate than the model's (`fs` != `model_fs`) is resampled on the device by
`ecg_wfdb16_windows_resampled` (ecg_hip/resample.py) between the DAC conversion and the z-score; the window rule, the
chunks and the stitched CAMs then live on the model-rate axis of resampled_length(Ttot, up, down) samples.

A raw ambulatory recording carries baseline wander and mains hum that the per-window z-score cannot remove (drift of a
few mV dominates the std).  `filter=` conditions it on the device: the physical (or resampled) recording is written once
as fp32 and `ecg_fir_windows` (ecg_hip/filter.py) cuts the windows out of its zero-phase filtered form.

A finite window is not a trustworthy one: a flat line, an amplifier on its rail or a motion artefact z-scores into a
confident number.  `quality=` (ecg_hip/quality.py) takes ten exact integer indices per (recording, window, lead) from the
raw int16 stream in one launch of `ecg_wfdb16_quality` and keeps the windows it judges unusable out of prob_max / prob_mean.

A probability says nothing about where the beats are.  `beats=` (ecg_hip/beats.py) runs an integer QRS detector over the
raw stream (`ecg_wfdb16_beats`) and `ecg_beats_rhythm` gives every window its beat count and RR statistics, on the device.

A beat list says nothing about what the beats look like.  `template=` (ecg_hip/template.py) aligns every beat to a centred
mean template (`ecg_beats_sum`, `ecg_beats_match`: best lag within +-30 ms, two passes), gives every beat its correlation
with that template and a verdict, adds up the mean beat of the beats that pass over a display range, and — with CAMs —
averages the stitched CAM beat-locked (`ecg_beats_series_mean`): where in the beat the model looks.  The aligned positions
are slope-sum peaks moved onto a common phase of the mean beat, NOT R apices; the CAM lives on the model-rate axis, so on a
downsampled recording (down > up) cam_beat is a staircase in source samples — that is the CAM's own resolution; and the
spec's defaults are policy, not measurements.
"""
import torch

from . import _lib as L
from . import functional as hipF


def window_plan(Ttot, window, hop, tail="shift"):
    """-> (first, hop, W, last_start, starts): the arguments of ecg_wfdb16_windows / ecg_windows_overlap_mean for a recording
    of Ttot samples, and the W start samples as a tuple.  last_start is -1 when there is no shifted tail window."""
    Ttot, window, hop = int(Ttot), int(window), int(hop)
    if tail not in ("shift", "drop"):
        raise ValueError(f"tail={tail!r}: 'shift' or 'drop'")
    if window < 1 or hop < 1:
        raise ValueError(f"window={window} and hop={hop} must be >= 1")
    if Ttot < window:
        raise ValueError(f"the recording has {Ttot} samples, fewer than one window of {window}")
    W = (Ttot - window) // hop + 1
    starts = [w * hop for w in range(W)]
    last_start = -1
    if tail == "shift" and (Ttot - window) % hop != 0:
        last_start = Ttot - window
        starts.append(last_start)
        W += 1
    return 0, hop, W, last_start, tuple(starts)


def plan_chunks(R, plan, batch_size):
    """The calls one plan is scored in, as (r0, r1, w0, first, W, last_start): recordings r0..r1 and their windows
    w0..w0+W of the plan, cut by (first, hop, W, last_start).  More windows per recording than batch_size: one recording
    per call, chunked over w, the shifted tail only in the chunk that holds the final window.  Otherwise batch_size // W
    whole recordings per call."""
    first, hop, W, last_start, _ = plan
    if batch_size < 1:
        raise ValueError(f"batch_size={batch_size}")
    if W > batch_size:
        return [(r, r + 1, w0, first + w0 * hop, min(batch_size, W - w0), last_start if w0 + batch_size >= W else -1)
                for r in range(R) for w0 in range(0, W, batch_size)]
    g = batch_size // W
    return [(r0, min(R, r0 + g), 0, first, W, last_start) for r0 in range(0, R, g)]


class RecordingScore:
    """starts (W start samples); logits, prob [R, W, C]; finite [R, W]; prob_max, prob_mean [R, C] over the finite windows
    (NaN where a recording has none); with CAMs: cam [R, K, Ttot], cover [Ttot] (windows over each sample).
    fs: the sampling rate of the axis starts / cam / cover are on (the model's rate where the recording was resampled,
    Ttot then being the resampled length; None when no rate was given); source_len: samples of the recording itself.
    With quality=: quality int64 [R, W, leads, 10] (quality.FIELDS, on the source axis), lead_ok [R, W, leads] and
    usable [R, W]; prob_max / prob_mean are then over the windows that are finite AND usable.  None otherwise.
    With beats=: beats int32 [R, cap] (beat samples on the SOURCE axis, ascending, -1 from n_beats[r] on), n_beats int32
    [R], rhythm int64 [R, W, 8] (beats.FIELDS) and heart_rate float64 [R, W] in bpm (NaN under 2 beats).  None otherwise.
    With template= (all on the SOURCE axis, [R, cap] rows aligned with beats): beat_lag int32, the lag of every beat against
    the centred mean template of the last pass; beat_pos int32 = beats + beat_lag (-1 where beats is); beat_corr float64, the
    lower median over the leads of the beat's correlation with that template (NaN where there is none); beat_ok bool,
    beat_corr >= min_corr; template float64 mV [R, L, leads], the mean of the ok beats over the display range at beat_pos (NaN
    where template_n is 0), template_n int32 [R, L, leads] the samples averaged, template_offsets the L sample offsets
    -pre .. post from beat_pos (a tuple; divide by the source rate for seconds); with CAMs also cam_beat fp32 [R, K, L], the
    mean of cam at those offsets over the ok beats whose range lies on covered samples, and cam_beat_n int32 [R] their
    number.  None otherwise."""
    __slots__ = ("starts", "logits", "prob", "finite", "prob_max", "prob_mean", "cam", "cover", "fs", "source_len",
                 "quality", "lead_ok", "usable", "beats", "n_beats", "rhythm", "heart_rate", "beat_pos", "beat_lag", "beat_ok",
                 "beat_corr", "template", "template_n", "template_offsets", "cam_beat", "cam_beat_n")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


def _record_level(prob, finite):
    """amax / mean of prob [R, W, C] over the windows flagged finite, as torch computes them on those windows."""
    pmax, pmean = prob.amax(1), prob.mean(1)
    for r in torch.nonzero(~finite.all(1)).flatten().tolist():
        sel = prob[r][finite[r]]
        if sel.shape[0]:
            pmax[r], pmean[r] = sel.amax(0), sel.mean(0)
        else:
            pmax[r], pmean[r] = float("nan"), float("nan")
    return pmax, pmean


def _chunk_windows(d, gain, baseline, window, hop, Ttot, ratio, taps):
    """-> windows_of(chunk) = (x [r1-r0, Wc, leads, window], stats) for an entry of plan_chunks, walked in its order.
    Without taps: ONE launch per chunk, wfdb16_windows — or wfdb16_windows_resampled by ratio = (up, down) — on the
    chunk's recordings.  With taps: fir_windows per chunk out of `phys`, the fp32 physical (or resampled) recordings
    [r1-r0, leads, Ttot] of the group in flight, which ONE whole-recording launch (W = 1, not normalised) writes when the
    (r0, r1) group changes — once per group, not once per chunk.  Nothing else knows about phys."""
    def cut(r0, r1, T, first, hop, W, last, normalize):       # -> (x, stats); x alone when not normalised
        if ratio is None:
            return hipF.wfdb16_windows(d[r0:r1], gain[r0:r1], baseline[r0:r1], T, first, hop, W, last, normalize, True)
        return hipF.wfdb16_windows_resampled(d[r0:r1], gain[r0:r1], baseline[r0:r1], T, first, hop, W, last, *ratio,
                                             normalize, True)

    phys = phys_of = None

    def windows_of(chunk):
        nonlocal phys, phys_of
        r0, r1, _, first, Wc, last = chunk
        if taps is None:
            return cut(r0, r1, window, first, hop, Wc, last, True)
        if phys_of != (r0, r1):
            phys, phys_of = cut(r0, r1, Ttot, 0, 1, 1, -1, False)[:, 0], (r0, r1)
        return hipF.fir_windows(phys, taps, window, first, hop, Wc, last, return_stats=True)

    return windows_of


def _quality_gate(quality, d, gain, rails, window, plan, ratio, fs, source_len):
    """-> (quality table, lead_ok, usable) of every window of the plan from ONE wfdb16_quality launch on the raw stream,
    judged at the source rate fs; (None, None, None) and no launch without quality=."""
    if quality is None or quality is False:
        return None, None, None
    from .quality import QualitySpec, source_span
    spec = QualitySpec() if quality is True else quality
    if not isinstance(spec, QualitySpec):
        raise ValueError(f"quality={quality!r}: a QualitySpec, True or None")
    up, down = ratio or (1, 1)
    first, hop, W, last_start, _ = plan
    qtab = hipF.wfdb16_quality(d, window, first, hop, W, last_start, up, down, rails)
    return (qtab, *spec.judge(qtab, gain, fs, source_span(window, source_len, up, down)))


def _beat_stage(beats, d, gain, window, plan, ratio, fs, source_len):
    """-> (beats, n_beats, rhythm, heart_rate) from ONE wfdb16_beats call on the raw stream at the source rate fs and ONE
    beats_rhythm launch on the call's plan and ratio; four Nones and no launch without beats=."""
    if beats is None or beats is False:
        return None, None, None, None
    from .beats import BeatSpec, heart_rate
    spec = BeatSpec() if beats is True else beats
    if not isinstance(spec, BeatSpec):
        raise ValueError(f"beats={beats!r}: a BeatSpec, True or None")
    if fs is None:
        raise ValueError("beats=: the detector's parameters are in seconds and need the sampling rate fs of the source stream")
    p = spec.params(fs, gain)
    up, down = ratio or (1, 1)
    first, hop, W, last_start, _ = plan
    b, n = hipF.wfdb16_beats(d, p["s"], p["h"], p["ref"], p["blk"], p["num"], p["den"], p["g_min"], p["lead_mask"])
    rhythm = hipF.beats_rhythm(b, n, source_len, window, first, hop, W, last_start, up, down, p["nn_delta"])
    return b, n, rhythm, heart_rate(rhythm, fs)        # summarize(rhythm, fs)["heart_rate"]


def _template_spec(template, beats, fs):
    """-> the TemplateSpec of template= (None: no stage); the argument errors of the stage, before anything is launched."""
    if template is None or template is False:
        return None
    from .template import TemplateSpec
    spec = TemplateSpec() if template is True else template
    if not isinstance(spec, TemplateSpec):
        raise ValueError(f"template={template!r}: a TemplateSpec, True or None")
    if beats is None or beats is False:
        raise ValueError("template=: the stage works on the beat list and needs beats=")
    if fs is None:
        raise ValueError("template=: the spec's parameters are in seconds and need the sampling rate fs of the source stream")
    return spec


def _template_stage(spec, d, gain, baseline, beats, n_beats, fs, cam, cover, ratio):
    """-> dict of the RecordingScore fields of template= from the beat list (beats, n_beats) of d.  `passes` rounds of
    beats_sum over the match range at the current positions, the centred mean template, and beats_match at the ORIGINAL
    beats; then beats_sum over the display range at the aligned positions and — with cam [R, K, Tx] and its cover — ONE
    beats_series_mean of the ok beats whose mapped range touches no uncovered sample.  Everything between the launches is
    torch ops on the device."""
    from . import template as T
    p = spec.params(fs)
    R, Ttot, leads = d.shape
    mask = spec.lead_mask(leads)
    pos, ok, lag, corr = beats, None, None, None
    for _ in range(max(1, int(spec.passes))):
        s, c = hipF.beats_sum(d, pos, n_beats, p["match_pre"], p["match_post"], include=ok)
        tm = T.mean_template(s, c, centre=True)
        lag, m = hipF.beats_match(d, beats, n_beats, tm, p["match_pre"], p["match_post"], p["J"], lead_mask=mask)
        corr = T.beat_correlation(m, mask)
        pos, ok = beats + lag, corr >= spec.min_corr
    s, c = hipF.beats_sum(d, pos, n_beats, p["pre"], p["post"], include=ok)
    out = dict(beat_pos=pos, beat_lag=lag, beat_ok=ok, beat_corr=corr, template_n=c,
               template=T.physical(T.mean_template(s, c), gain, baseline),
               template_offsets=tuple(range(-p["pre"], p["post"] + 1)))
    if cam is not None:
        up, down = ratio or (1, 1)
        Tx = cam.shape[-1]
        x = pos.to(torch.int64)
        lo = torch.clamp(torch.clamp(x - p["pre"], min=0) * up // down, max=Tx - 1)
        hi = torch.clamp(torch.clamp(x + p["post"], min=0) * up // down, max=Tx - 1)
        holes = torch.cat([cover.new_zeros(1, dtype=torch.int64), (cover == 0).to(torch.int64).cumsum(0)])
        inc = ok & (holes[hi + 1] == holes[lo])
        out["cam_beat"], out["cam_beat_n"] = hipF.beats_series_mean(cam, pos, n_beats, Ttot, p["pre"], p["post"], up, down,
                                                                    include=inc)
    return out


def _normalize_per_record(cam, cover):
    """cam_normalize="record": min-max of every (recording, class) row of cam [R, K, Ttot] over its covered samples
    (cover > 0), divided only where the maximum is > 0; 0 where nothing covers."""
    covered = (cover > 0)[None, None, :]
    big = torch.finfo(cam.dtype).max
    c = cam - torch.where(covered, cam, cam.new_full((), big)).amin(-1, keepdim=True)
    mx = torch.where(covered, c, cam.new_full((), -big)).amax(-1, keepdim=True)
    c = torch.where(mx > 0, c / torch.where(mx > 0, mx, torch.ones_like(mx)), c)
    return torch.where(covered, c, torch.zeros_like(c))


def score_recording(model, d, gain, baseline, *, window, hop=None, tail="shift", batch_size=256, x_demo=None,
                    cam_classes=None, cam_normalize=None, fs=None, model_fs=None, filter=None, quality=None, rails=None,
                    beats=None, template=None):
    """Score recordings d int16 [Ttot, leads] or [R, Ttot, leads] (on the GPU, the .dat layout) with `model` in eval mode.

    gain float64 / baseline int32 [leads] or [R, leads]; window: samples per model input; hop: default window // 2;
    tail: see window_plan; x_demo [R, D] (ECGMultimodal) is repeated for every window of its recording.
    Windows are produced and consumed in chunks of at most batch_size (plan_chunks), through `model(x)` under the caller's
    inference_precision — or, with cam_classes (a list of class indices), through ecg_hip.grad_cam(class_idx=cam_classes,
    signal_length=window, normalize=None), whose logits are used.  The raw per-window CAMs are stitched by overlap_mean;
    cam_normalize="record" then min-max normalises every (recording, class) row over its covered samples (divided only
    where the maximum is > 0).  The CAM path keeps K x W x window floats per recording until the stitch.

    `finite[r, w]` is False when a logit of the window is not finite or the window holds an invalid sample (-32768, a
    NaN lead).  The kernels hand a NaN on as the stock layers do (pool, ReLU and the eval epilogues included), so the
    logits of such a window are NaN — in its own rows only, the other windows of the batch keep their bits — and it is
    kept out of prob_max / prob_mean; the flag is still taken from the input statistics as well as from the logits.

    fs / model_fs: the sampling rates of the recording and of the model's training data.  When both are given and differ,
    the recording is resampled on the device by up/down = model_fs/fs (resample.rational_ratio; ValueError when the ratio
    needs a term above 512): window, hop, starts, cam and cover are then on the MODEL-RATE axis of
    resample.resampled_length(Ttot, up, down) samples, and model-axis sample t lies at source time t*down/up samples.
    The CAMs are not mapped back to the source axis.  With either None, or both equal, nothing is resampled.

    filter: an ecg_hip.filter.FilterSpec (FilterSpec() is a 0.5 Hz baseline-wander high-pass; notch=50 adds a mains
    notch), or symmetric FIR taps (full, or filter.one_sided's) taken as designed for the axis the windows live on.  A
    spec is designed at that axis' rate — model_fs where the recording is resampled, otherwise fs — and raises ValueError
    when that rate was not given.  The physical (or resampled) fp32 recording of the recordings in flight is then
    written once per recording group of plan_chunks and every chunk comes from functional.fir_windows: zero phase, ends
    edge-held, a filtered sample independent of the window that asks (functional.fir_filter gives the whole conditioned
    signal).  An invalid sample poisons every filtered sample within `half` taps of it on its lead — 363 samples at
    100 Hz, 1813 at 500 Hz for the default high-pass — so a long filter widens the set of windows flagged not finite.
    None (default): no filter, no further launch, today's bits.

    quality: an ecg_hip.quality.QualitySpec, or True for QualitySpec() (its defaults are policy, not measurements).  ONE
    launch of functional.wfdb16_quality for the whole call takes the indices of every window of the plan from the RAW
    int16 stream — before resampling and before filter=, which would hide the defects it looks for; on a resampled
    recording the model-axis windows are mapped onto the source samples they cover by up/down.  rails: (lo, hi) int32
    [leads] or [R, leads], the ADC rails of the stream (quality.rails_from_header; None: -32767 and 32767).  The spec is
    judged at the SOURCE rate fs (ValueError when flat_s is set and fs is None).  The score gains quality, lead_ok and
    usable, and prob_max / prob_mean are taken over finite & usable (NaN where a recording has no such window).  logits,
    prob, finite and the CAMs are untouched: unusable windows are still scored and still stitched.
    None (default): no launch is added and every output keeps today's bits.

    beats: an ecg_hip.beats.BeatSpec, or True for BeatSpec() (its defaults are policy, not measurements).  ONE
    functional.wfdb16_beats call for the whole call detects the beats of every recording on the RAW int16 stream at the
    SOURCE rate fs (ValueError when fs is None) — before resampling and before filter= — and ONE functional.beats_rhythm
    launch takes the table of every window of the plan, mapped onto the source samples by up/down as for quality=.  The
    score gains beats, n_beats (source-axis sample indices; they are not mapped onto the model-rate axis), rhythm and
    heart_rate (beats.summarize).  Every other output is untouched.  None (default): nothing is launched.

    template: an ecg_hip.template.TemplateSpec, or True for TemplateSpec() (its defaults are policy, not measurements);
    needs beats= and fs (ValueError otherwise).  After the beats: `passes` rounds of functional.beats_sum over the match
    range, the centred mean template (template.mean_template) and functional.beats_match at the original beats give every
    beat its lag, its correlation and its verdict; one more beats_sum over the display range gives the mean beat of the
    beats that passed; with cam_classes, functional.beats_series_mean averages the stitched cam (as returned, so after
    cam_normalize) beat-locked, mapped by up/down, over the ok beats whose range [pos - pre, pos + post] maps onto covered
    samples only.  All on the RAW stream and the SOURCE axis, like the beats.  The positions are aligned slope-sum peaks,
    not R apices; on a downsampled recording cam_beat is a staircase in source samples, the CAM's own resolution.  The
    score gains beat_pos, beat_lag, beat_ok, beat_corr, template, template_n, template_offsets, cam_beat and cam_beat_n
    (RecordingScore).  Every other output is untouched.  None (default): nothing is launched.
    -> RecordingScore."""
    if not (torch.is_tensor(d) and d.is_cuda):
        raise L.EcgHipError("score_recording: a CPU tensor reached the HIP input step; d must be on the GPU "
                            "(there is no CPU form of the sliding input step)")
    if model.training:
        raise ValueError("score_recording needs model.eval()")
    if cam_normalize not in (None, "record"):
        raise ValueError(f"cam_normalize={cam_normalize!r}: None or 'record'")
    if d.dim() == 2:
        d = d[None]
    if d.dim() != 3:
        raise L.EcgHipError("score_recording: d must be [Ttot, leads] or [R, Ttot, leads]")
    R, Ttot, leads = d.shape
    dev = d.device
    gain = torch.as_tensor(gain, dtype=torch.float64).to(dev).reshape(-1, leads)
    baseline = torch.as_tensor(baseline, dtype=torch.int32).to(dev).reshape(-1, leads)
    if gain.shape[0] != R or baseline.shape[0] != R:
        raise L.EcgHipError("score_recording: gain/baseline must be [leads] or [R, leads]")
    if x_demo is not None and x_demo.shape[0] != R:
        raise ValueError(f"x_demo has {x_demo.shape[0]} rows for {R} recordings")
    window = int(window)
    source_len, ratio = Ttot, None
    if fs is not None and model_fs is not None and fs != model_fs:
        from .resample import rational_ratio, resampled_length
        ratio = rational_ratio(fs, model_fs)
        if ratio == (1, 1):         # equal within rational_ratio's 1e-9: nothing to resample
            ratio = None
        else:
            Ttot = resampled_length(Ttot, *ratio)
    plan = window_plan(Ttot, window, window // 2 if hop is None else hop, tail)
    _, hop, W, _, starts = plan
    taps = None
    if filter is not None:
        from .filter import FilterSpec, one_sided
        axis_fs = fs if ratio is None else model_fs
        taps = one_sided(filter.taps(axis_fs) if isinstance(filter, FilterSpec) else filter)
    cams = None if cam_classes is None else [int(k) for k in cam_classes]
    tspec = _template_spec(template, beats, fs)
    d = hipF._contig(d)
    qtab, lead_ok, usable = _quality_gate(quality, d, gain, rails, window, plan, ratio, fs, source_len)
    beat_list, n_beats, rhythm, heart_rate = _beat_stage(beats, d, gain, window, plan, ratio, fs, source_len)
    windows_of = _chunk_windows(d, gain, baseline, window, hop, Ttot, ratio, taps)

    logits = v = None
    ok = torch.empty(R, W, dtype=torch.bool, device=dev)
    for chunk in plan_chunks(R, plan, int(batch_size)):
        r0, r1, w0, _, Wc, _ = chunk
        x, stats = windows_of(chunk)
        n = (r1 - r0) * Wc
        x = x.view(n, leads, window)
        xd = None if x_demo is None else x_demo[r0:r1].repeat_interleave(Wc, dim=0)
        if cams is None:
            with torch.no_grad():
                lg = model(x) if xd is None else model(x, xd)
        else:       # (not under no_grad: where the fused path does not apply, grad_cam differentiates the logits)
            from .gradcam import grad_cam
            cam, lg = grad_cam(model, x, xd, class_idx=cams, signal_length=window, normalize=None, return_logits=True)
            if v is None:
                v = hipF._empty(x, R, W, len(cams), window)
            v[r0:r1, w0:w0 + Wc] = cam.reshape(r1 - r0, Wc, len(cams), window)
        if logits is None:
            logits = hipF._empty(x, R, W, lg.shape[1])
        logits[r0:r1, w0:w0 + Wc] = lg.reshape(r1 - r0, Wc, -1)
        ok[r0:r1, w0:w0 + Wc] = torch.isfinite(stats).view(r1 - r0, Wc, -1).all(-1)
    finite = ok & torch.isfinite(logits).all(-1)
    prob = hipF.sigmoid(logits)
    pmax, pmean = _record_level(prob, finite if usable is None else finite & usable)
    cam = cover = None
    if cams is not None:
        cam, cover = hipF.overlap_mean(v, plan, Ttot, return_cover=True)
        if cam_normalize == "record":
            cam = _normalize_per_record(cam, cover)
    morph = {} if tspec is None else _template_stage(tspec, d, gain, baseline, beat_list, n_beats, fs, cam, cover, ratio)
    return RecordingScore(starts=starts, logits=logits, prob=prob, finite=finite, prob_max=pmax, prob_mean=pmean,
                          cam=cam, cover=cover, fs=fs if ratio is None else model_fs, source_len=source_len,
                          quality=qtab, lead_ok=lead_ok, usable=usable, beats=beat_list, n_beats=n_beats, rhythm=rhythm,
                          heart_rate=heart_rate, **morph)


def score_wfdb_record(record_path, model, model_fs=None, leads=None, **kw):
    """score_recording for a WFDB record of any length on disk (record_path without extension), on the device of the model.
    model_fs: the rate the model was trained at; the record is resampled on the device when its header's rate differs.
    None (default): the record is scored at its own rate, whatever the header says.  filter= (score_recording) is passed
    through: a FilterSpec is designed at model_fs when the record is resampled, otherwise at the header's rate.
    quality= is passed through too, with the ADC rails of the selected leads (quality.rails_from_header: adc_res and
    adc_zero of the header, or the storage format's range) unless the caller gives rails= itself.  beats= is passed
    through as well and detects at the header's rate; template= likewise.

    leads: the signals to score, in the model's lead order — names matched against the header's descriptions (e.g.
    wfdbraw.PTBXL_LEADS for a 15-signal PTB Diagnostic record) or signal indices; None: every signal, in header order.
    A plain format-16 record (one .dat file, no skew, no byte offset) with leads=None is read by ecg_hip.wfdb16 and
    uploaded as int16.  Every other record — formats 61, 80, 160 and 212, skews, byte offsets, several files, a lead
    selection — goes through ecg_hip.wfdbraw: the files' bytes are uploaded as they are and ecg_wfdb_decode16 writes the
    int16 stream on the device (the header checksums are verified there)."""
    from .wfdb16 import parse_header, read_record
    dev = next(model.parameters()).device
    with open(record_path + ".hea", "r") as f:
        sigs = parse_header(f.read())["signals"]
    plain = leads is None and len({s["file"] for s in sigs}) == 1 and all(
        s["fmt"] == 16 and s["spf"] == 1 and s["skew"] == 0 and s["offset"] == 0 for s in sigs)
    cols = range(len(sigs))
    if plain:
        rec = read_record(record_path)
        d, gain, baseline, fs = torch.from_numpy(rec.d.astype("int16")).to(dev), rec.gain, rec.baseline, rec.fs
    else:
        from .wfdbraw import read_raw_record, select_leads, to_device
        rec = read_raw_record(record_path)
        d, gain, baseline = to_device(rec, dev, leads)
        fs = rec.fs
        if leads is not None:
            cols = select_leads(rec, leads)
    if kw.get("quality") is not None and "rails" not in kw:
        from .quality import rails_from_header
        kw["rails"] = rails_from_header([sigs[c] for c in cols])
    return score_recording(model, d, torch.from_numpy(gain).to(dev), torch.from_numpy(baseline).to(dev), fs=fs,
                           model_fs=model_fs, **kw)
