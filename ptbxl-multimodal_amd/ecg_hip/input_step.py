"""The input step: the wrappers over the entry points that turn bytes on disk into the model's windows (WFDB decode,
DAC conversion, resampling, zero-phase FIR, window cut, per-lead z-score), the quality indices of those windows, the
beat list, its rhythm table and the beat-morphology reductions, and the overlap mean that brings per-window CAMs back onto
the recording's axis.  None of it takes part in autograd.

`ecg_hip.functional` re-exports every name of this module at its end and stays the place callers reach them through
(`functional.wfdb16_windows`, ...).  A wrapper that is built on another one looks it up there as well, so that a
replacement installed on `functional` holds for every path."""
import torch

from . import _lib as L
from . import functional as _F
from .functional import _call, _contig, _empty, _f32, _st


def _raw_stream(who, d, gain=None, baseline=None, axes=("R", "Ttot")):
    """The one check of a raw int16 stream d [R, Ttot, leads] on the GPU (with its calibration gain float64 / baseline
    int32 [R, leads], when the entry point converts) -> contiguous (d, gain, baseline)."""
    if not (torch.is_tensor(d) and d.is_cuda):
        raise L.EcgHipError(f"{who}: a CPU tensor reached the HIP input step; d must be on the GPU")
    if gain is None:
        if d.dtype != torch.int16:
            raise L.EcgHipError(f"{who}: d must be int16 (the raw stream), got {d.dtype}")
    elif d.dtype != torch.int16 or gain.dtype != torch.float64 or baseline.dtype != torch.int32:
        raise L.EcgHipError(f"{who}: d must be int16, gain float64, baseline int32")
    shape = tuple(d.shape)
    if len(shape) != 3:
        raise L.EcgHipError(f"{who}: d must be [{axes[0]}, {axes[1]}, leads]")
    if gain is None:
        return _contig(d), None, None
    rows = (shape[0], shape[2])
    if tuple(gain.shape) != rows or tuple(baseline.shape) != rows:
        raise L.EcgHipError(f"{who}: gain/baseline must be [{axes[0]}, leads]")
    return _contig(d), _contig(gain), _contig(baseline)


def _windows_out(ref, R, W, leads, window, normalize, return_stats, launch):
    """Allocate out fp32 [R, W, leads, window] (and stats [R*W*leads, 2] when normalising) beside `ref`, run
    launch(out, stats) and -> (out, stats) or out.  An empty plan gets empty tensors: the C side is what refuses it."""
    W = max(int(W), 0)
    out = torch.empty(R, W, leads, max(int(window), 0), dtype=torch.float32, device=ref.device)
    stats = _empty(out, R * W * leads, 2) if normalize else None
    launch(out, stats)
    return (out, stats) if normalize and return_stats else out


def zscore_per_lead(x, out=None, return_stats=False):
    """(x - mean)/(std + 1e-6) per lead row, population std, bit-identical to the reference's float32
    numpy arithmetic (src/datasets/ptbxl.py:122-127).  `out` may alias x (in place)."""
    x = _contig(x)
    T = x.shape[-1]
    rows = x.numel() // T
    if out is None:
        out = torch.empty_like(x)
    stats = _empty(x, rows, 2)
    _call("ecg_zscore_rows", _f32(x), _f32(out), _f32(stats), rows, T, _st())
    return (out, stats) if return_stats else out


def wfdb16_to_windows(d, gain, baseline, normalize=True, return_stats=False):
    """WFDB format-16 samples d int16 [B, T, leads] (time-major, as stored in .dat) + per-(window, lead)
    gain (float64) / baseline (int32) [B, leads]  ->  fp32 windows [B, leads, T], per-lead z-scored:
    `_load_ecg` + `_normalize` of the reference (src/datasets/ptbxl.py:14-41,122-127) on the GPU, one
    launch.  normalize=False stops at the physical signal."""
    d, gain, baseline = _raw_stream("wfdb16_to_windows", d, gain, baseline, axes=("B", "T"))
    B, T, leads = d.shape
    x = torch.empty(B, leads, T, dtype=torch.float32, device=d.device)
    if not normalize:
        _call("ecg_wfdb16_physical", L.ptr(d), L.ptr(gain), L.ptr(baseline), _f32(x), B, T, leads, _st())
        return x
    stats = _empty(x, B * leads, 2)
    _call("ecg_wfdb16_zscore", L.ptr(d), L.ptr(gain), L.ptr(baseline), _f32(x), _f32(stats), B, T, leads, _st())
    return (x, stats) if return_stats else x


def wfdb16_windows(d, gain, baseline, window, first, hop, W, last_start=-1, normalize=True, return_stats=False):
    """Windows read IN PLACE out of continuous recordings d int16 [R, Ttot, leads] (gain float64 / baseline int32
    [R, leads]): window w of every recording starts at sample first + w*hop, the last one at `last_start` when that is
    >= 0.  -> fp32 [R, W, leads, window], each window bit-identical to wfdb16_to_windows on a copy of its slice
    (stats [R*W*leads, 2] likewise).  The raw form under wfdb16_to_windows_sliding, for callers that chunk a plan."""
    d, gain, baseline = _raw_stream("wfdb16_windows", d, gain, baseline)
    R, Ttot, leads = d.shape
    return _windows_out(d, R, W, leads, window, normalize, return_stats, lambda x, stats: _call(
        "ecg_wfdb16_windows", L.ptr(d), L.ptr(gain), L.ptr(baseline), _f32(x), _f32(stats), R, Ttot, leads, int(window),
        int(first), int(hop), int(W), int(last_start), _st()))


def wfdb16_windows_resampled(d, gain, baseline, window, first, hop, W, last_start, up, down, normalize=True,
                             return_stats=False):
    """wfdb16_windows for recordings sampled at another rate than the model's: d int16 [R, Ttot, leads] is resampled by
    up/down on the device (ecg_hip.resample: scipy.signal.resample_poly's default filter, edge-held ends) between the
    DAC conversion and the z-score, and the windows (first, hop, W, last_start — on the RESAMPLED axis of
    resample.resampled_length(Ttot, up, down) samples) are cut out of the result.  -> fp32 [R, W, leads, window]
    (stats [R*W*leads, 2] with return_stats).  A resampled sample depends on its index and the recording only, so
    every window is a bitwise slice of the whole resampled recording.  The raw form, beside wfdb16_windows."""
    from .resample import device_taps
    d, gain, baseline = _raw_stream("wfdb16_windows_resampled", d, gain, baseline)
    up, down = int(up), int(down)
    if not (1 <= up <= 512 and 1 <= down <= 512):
        raise L.EcgHipError(f"wfdb16_windows_resampled: up={up} down={down} outside [1,512]")
    taps, ntap, half = device_taps(up, down, d.device)
    return _F._resampled_call(d, gain, baseline, taps, window, first, hop, W, last_start, up, down, ntap, half, normalize,
                              return_stats)


def _resampled_call(d, gain, baseline, taps, window, first, hop, W, last_start, up, down, ntap, half, normalize=True,
                    return_stats=False):
    """ecg_wfdb16_windows_resampled with a caller-made table taps fp32 [up, ntap] (the ABI's own argument list)."""
    R, Ttot, leads = d.shape
    return _windows_out(d, R, W, leads, window, normalize, return_stats, lambda x, stats: _call(
        "ecg_wfdb16_windows_resampled", L.ptr(d), L.ptr(gain), L.ptr(baseline), _f32(taps), _f32(x), _f32(stats), R, Ttot,
        leads, int(window), int(first), int(hop), int(W), int(last_start), int(up), int(down), int(ntap), int(half), _st()))


def fir_windows(x, taps, window, first, hop, W, last_start=-1, normalize=True, return_stats=False):
    """Zero-phase FIR conditioning of physical recordings x fp32 [R, leads, Ttot] (what wfdb16_windows /
    wfdb16_windows_resampled give for window = the whole recording, W = 1, normalize=False), then the windows of the
    window rule cut out of the filtered recording and z-scored: -> fp32 [R, W, leads, window] (stats [R*W*leads, 2] with
    return_stats; normalize=False stops at the filtered physical windows).  taps: the full symmetric filter
    [2*half + 1] (ecg_hip.filter designs them) or what filter.one_sided returns; half <= 4096.  A filtered sample depends
    on its index and the recording only (ends edge-held), so every window is a bitwise slice of fir_filter's output; a NaN
    sample poisons every output within `half` samples of it on its lead."""
    from .filter import device_one_sided
    if not (torch.is_tensor(x) and x.is_cuda):
        raise L.EcgHipError("fir_windows: a CPU tensor reached the HIP input step; x must be on the GPU")
    if x.dtype != torch.float32:
        raise L.EcgHipError(f"fir_windows: x must be float32 (the physical recording), got {x.dtype}")
    if x.dim() != 3:
        raise L.EcgHipError("fir_windows: x must be [R, leads, Ttot]")
    c, half = device_one_sided(taps, x.device)
    return _F._fir_call(_contig(x), c, window, first, hop, W, last_start, half, normalize, return_stats)


def _fir_call(x, c, window, first, hop, W, last_start, half, normalize=True, return_stats=False):
    """ecg_fir_windows with caller-made one-sided taps c fp32 [half+1] on the device (the ABI's own argument list)."""
    R, leads, Ttot = x.shape
    return _windows_out(x, R, W, leads, window, normalize, return_stats, lambda out, stats: _call(
        "ecg_fir_windows", _f32(x), _f32(c), _f32(out), _f32(stats), R, Ttot, leads, int(window), int(first), int(hop),
        int(W), int(last_start), int(half), _st()))


def fir_filter(x, taps):
    """The whole filtered recording, fp32 [R, leads, Ttot] for x [R, leads, Ttot]: fir_windows with one window that is
    the recording, not z-scored — the signal a CAM of a filtered score_recording is plotted over."""
    if torch.is_tensor(x) and x.dim() == 3:
        return _F.fir_windows(x, taps, x.shape[2], 0, 1, 1, -1, normalize=False)[:, 0]
    return _F.fir_windows(x, taps, 0, 0, 1, 1)     # raises fir_windows' own error for this x


def wfdb16_to_windows_sliding(d, gain, baseline, window, hop, tail="shift", normalize=True, return_stats=False):
    """wfdb16_to_windows for recordings longer than one window: d int16 [R, Ttot, leads] is cut into the windows of
    recording.window_plan(Ttot, window, hop, tail) without an overlapping copy ever existing.
    -> (x [R, W, leads, window], plan), or (x, stats, plan) with return_stats."""
    from .recording import window_plan
    if d.dim() != 3:
        raise L.EcgHipError("wfdb16_to_windows_sliding: d must be [R, Ttot, leads]")
    plan = window_plan(d.shape[1], window, hop, tail)
    first, hop, W, last_start, _ = plan
    out = _F.wfdb16_windows(d, gain, baseline, window, first, hop, W, last_start, normalize, return_stats)
    return (*out, plan) if isinstance(out, tuple) else (out, plan)


def wfdb_decode16(files, layout, n_samp, columns=None):
    """The packed bytes of a WFDB record's .dat files -> the int16 stream [n_samp, len(columns)] the input step reads
    (time-major, as a format-16 file stores it), decoded on the device by ecg_wfdb_decode16: one launch per file.

    files: uint8 CUDA tensors, one per .dat file, holding the file's bytes as they are.  layout: one entry per signal of
    the record (wfdbraw.RawSignal, or anything with these attributes): file (index into files), fmt (16, 61, 80, 160 or
    212), frame (signals interleaved in that file), slot (position inside a frame), skew (frames the signal is stored
    late) and offset (bytes before the file's first sample; honoured by slicing, never by copying).  columns: indices
    into layout, in output order (default: every signal).  The format's invalid code, and every sample a skew or a short
    file puts past the end of the bytes, comes out as -32768 — what the window kernels turn into NaN."""
    layout = list(layout)
    columns = list(range(len(layout))) if columns is None else [int(c) for c in columns]
    n_samp, L_out = int(n_samp), len(columns)
    if not 1 <= L_out <= 16:
        raise L.EcgHipError(f"wfdb_decode16: {L_out} output columns outside [1,16]")
    for f in files:
        if not (torch.is_tensor(f) and f.is_cuda):
            raise L.EcgHipError("wfdb_decode16: a CPU tensor reached the HIP input step; the file bytes must be on the GPU")
        if f.dtype != torch.uint8 or f.dim() != 1:
            raise L.EcgHipError("wfdb_decode16: files must be one-dimensional uint8 tensors (the .dat bytes as they are)")
    by_file = {}
    for j, c in enumerate(columns):
        if not 0 <= c < len(layout):
            raise L.EcgHipError(f"wfdb_decode16: column {c} outside the record's {len(layout)} signals")
        by_file.setdefault(int(layout[c].file), []).append((j, layout[c]))
    out = torch.empty(max(n_samp, 0), L_out, dtype=torch.int16, device=files[0].device if files else None)
    for fi, sel in by_file.items():
        s0 = sel[0][1]
        if any((s.fmt, s.frame, s.offset) != (s0.fmt, s0.frame, s0.offset) for _, s in sel):
            raise L.EcgHipError(f"wfdb_decode16: the signals of file {fi} disagree on format, frame size or byte offset")
        raw = _contig(files[fi])[int(s0.offset):]           # a view: the kernel takes any byte address
        _call("ecg_wfdb_decode16", raw.data_ptr(), raw.numel(),
              int(s0.fmt), int(s0.frame), L.int_table([s.slot for _, s in sel]), L.int_table([s.skew for _, s in sel]),
              L.int_table([j for j, _ in sel]), len(sel), L.ptr(out), n_samp, L_out, _st())
    return out


def wfdb16_quality(d, window, first, hop, W, last_start=-1, up=1, down=1, rails=None):
    """Signal-quality indices of the windows of d int16 [R, Ttot, leads], read in place by ONE launch of
    ecg_wfdb16_quality: -> int64 [R, W, leads, 10], the fields of ecg_hip.quality.FIELDS (exact integers).
    window, first, hop, W, last_start state the windows on the MODEL's axis, as for wfdb16_windows /
    wfdb16_windows_resampled; up/down maps that axis onto the source stream: window w with start s_w covers the source
    samples [a_w, a_w + Tq), a_w = min(s_w*down // up, Ttot - Tq), Tq = quality.source_span(window, Ttot, up, down).
    rails: (lo, hi) int32 [leads] or [R, leads] (quality.rails_from_header), None: -32767 and 32767."""
    from .quality import source_span
    d, _, _ = _raw_stream("wfdb16_quality", d)
    R, Ttot, leads = d.shape
    lo = hi = None
    if rails is not None:
        lo, hi = (_contig(torch.as_tensor(t, dtype=torch.int32).to(d.device).reshape(-1, leads).expand(R, leads))
                  for t in rails)
    q = torch.empty(R, max(int(W), 0), leads, 10, dtype=torch.int64, device=d.device)
    _call("ecg_wfdb16_quality", L.ptr(d), L.ptr(lo), L.ptr(hi), L.ptr(q), R, Ttot, leads, int(window), int(first), int(hop),
          int(W), int(last_start), int(up), int(down), source_span(window, Ttot, up, down), _st())
    return q


def wfdb16_beats(d, s, h, ref, blk, num, den, g_min, lead_mask=None):
    """The beats of d int16 [R, Ttot, leads], read in place by ecg_wfdb16_beats (four launches, no host synchronisation):
    -> (beats int32 [R, cap], n_beats int32 [R]), cap = (Ttot + ref) // (ref + 1); row r holds the beat samples of
    recording r ascending, -1 from n_beats[r] on.  s, h, ref, blk, num, den: the integers of the detector
    (include/ecg_hip.h; beats.BeatSpec.params derives them from physical units); g_min: int64 [R] (or one value), every
    entry >= 1; lead_mask: bit l = lead l takes part (None: every lead).  Allocates the outputs and the workspace."""
    d, _, _ = _raw_stream("wfdb16_beats", d)
    R, Ttot, leads = d.shape
    ref = int(ref)
    g_min = _contig(torch.as_tensor(g_min, dtype=torch.int64).to(d.device).reshape(-1).expand(R))
    mask = (1 << leads) - 1 if lead_mask is None else int(lead_mask)
    cap = (Ttot + ref) // (ref + 1) if ref >= 0 else 0
    beats = torch.empty(R, max(cap, 0), dtype=torch.int32, device=d.device)
    n_beats = torch.empty(R, dtype=torch.int32, device=d.device)
    nbytes = int(L.query("ecg_wfdb16_beats_workspace_bytes", R, Ttot, int(blk)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=d.device)
    _call("ecg_wfdb16_beats", L.ptr(d), L.ptr(g_min), L.ptr(beats), L.ptr(n_beats), L.ptr(ws), R, Ttot, leads, mask, int(s),
          int(h), ref, int(blk), int(num), int(den), _st())
    return beats, n_beats


def beats_rhythm(beats, n_beats, Ttot, window, first, hop, W, last_start=-1, up=1, down=1, nn_delta=0):
    """The rhythm table of a beat list (wfdb16_beats) by ONE launch of ecg_beats_rhythm: -> int64 [R, W, 8], the fields of
    ecg_hip.beats.FIELDS (exact integers).  Ttot: samples of the recordings the beats index (the source axis); window,
    first, hop, W, last_start state the windows on the MODEL's axis and up/down maps them onto the source samples
    [a_w, a_w + Tq) exactly as for wfdb16_quality; nn_delta: the |difference of successive RR| bound of n_drr_over, in
    source samples."""
    from .quality import source_span
    for name, t in (("beats", beats), ("n_beats", n_beats)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise L.EcgHipError(f"beats_rhythm: a CPU tensor reached the HIP input step; {name} must be on the GPU")
        if t.dtype != torch.int32:
            raise L.EcgHipError(f"beats_rhythm: {name} must be int32, got {t.dtype}")
    if beats.dim() != 2 or tuple(n_beats.shape) != (beats.shape[0],):
        raise L.EcgHipError("beats_rhythm: beats must be [R, cap] and n_beats [R]")
    R, cap = beats.shape
    out = torch.empty(R, max(int(W), 0), 8, dtype=torch.int64, device=beats.device)
    _call("ecg_beats_rhythm", L.ptr(_contig(beats)), L.ptr(_contig(n_beats)), L.ptr(out), R, int(Ttot), cap, int(window),
          int(first), int(hop), int(W), int(last_start), int(up), int(down), source_span(window, Ttot, up, down),
          int(nn_delta), _st())
    return out


def _beat_list(who, ref, pos, n, include):
    """The one check of a position list pos int32 [R, cap], n int32 [R], include uint8 / bool [R, cap] or None, all on the
    device of `ref` -> contiguous (pos, n, include as uint8 or None)."""
    for name, t, dt in (("pos", pos, torch.int32), ("n", n, torch.int32)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise L.EcgHipError(f"{who}: a CPU tensor reached the HIP input step; {name} must be on the GPU")
        if t.dtype != dt:
            raise L.EcgHipError(f"{who}: {name} must be int32, got {t.dtype}")
    R = ref.shape[0]
    if pos.dim() != 2 or pos.shape[0] != R or tuple(n.shape) != (R,):
        raise L.EcgHipError(f"{who}: pos must be [R={R}, cap] and n [R]")
    if include is not None:
        if not (torch.is_tensor(include) and include.is_cuda):
            raise L.EcgHipError(f"{who}: a CPU tensor reached the HIP input step; include must be on the GPU")
        if include.dtype == torch.bool:
            include = include.to(torch.uint8)
        if include.dtype != torch.uint8 or tuple(include.shape) != tuple(pos.shape):
            raise L.EcgHipError(f"{who}: include must be uint8 or bool [R, cap] like pos")
        include = _contig(include)
    return _contig(pos), _contig(n), include


def beats_sum(d, pos, n, pre, post, include=None):
    """The ensemble sums of the segments [x - pre, x + post] of d int16 [R, Ttot, leads] at the listed positions x (pos
    int32 [R, cap], the first n[r] of a row, >= 0, include != 0 where given; functional.wfdb16_beats' outputs are such a
    list) by ecg_beats_sum: -> (sum int64 [R, Lseg, leads], cnt int32 [R, Lseg, leads]), over the listed entries whose
    segment lies wholly inside the recording and the samples that are not -32768.  Exact integers."""
    d, _, _ = _raw_stream("beats_sum", d)
    pos, n, include = _beat_list("beats_sum", d, pos, n, include)
    R, Ttot, leads = d.shape
    Lseg = max(int(pre) + int(post) + 1, 0)
    s = torch.empty(R, Lseg, leads, dtype=torch.int64, device=d.device)
    c = torch.empty(R, Lseg, leads, dtype=torch.int32, device=d.device)
    _call("ecg_beats_sum", L.ptr(d), L.ptr(pos), L.ptr(n), L.ptr(include), L.ptr(s), L.ptr(c), R, Ttot, leads, pos.shape[1],
          int(pre), int(post), _st())
    return s, c


def beats_match(d, pos, n, tmpl, pre, post, J, lead_mask=None, include=None):
    """The best lag in [-J, J] of every listed position against tmpl int16 [R, Lseg, leads] (-32768: no value) by
    ecg_beats_match: -> (lag int32 [R, cap], m int64 [R, cap, leads, 7]), the fields of ecg_hip.template.FIELDS at the
    chosen lag for every lead.  The score is the integer dot product over the leads of lead_mask (None: every lead); the
    first of equal maxima wins, scanning from -J.  An entry that is not listed or has no lag with a whole segment gets
    lag 0 and zeros."""
    d, _, _ = _raw_stream("beats_match", d)
    pos, n, include = _beat_list("beats_match", d, pos, n, include)
    R, Ttot, leads = d.shape
    cap = pos.shape[1]
    Lseg = max(int(pre) + int(post) + 1, 0)
    if not (torch.is_tensor(tmpl) and tmpl.is_cuda):
        raise L.EcgHipError("beats_match: a CPU tensor reached the HIP input step; tmpl must be on the GPU")
    if tmpl.dtype != torch.int16 or tuple(tmpl.shape) != (R, Lseg, leads):
        raise L.EcgHipError(f"beats_match: tmpl must be int16 [R, Lseg={Lseg}, leads], got {tmpl.dtype} {tuple(tmpl.shape)}")
    mask = (1 << leads) - 1 if lead_mask is None else int(lead_mask)
    lag = torch.empty(R, cap, dtype=torch.int32, device=d.device)
    m = torch.empty(R, cap, leads, 7, dtype=torch.int64, device=d.device)
    _call("ecg_beats_match", L.ptr(d), L.ptr(pos), L.ptr(n), L.ptr(include), L.ptr(_contig(tmpl)), L.ptr(lag), L.ptr(m), R,
          Ttot, leads, cap, int(pre), int(post), int(J), mask, _st())
    return lag, m


def beats_series_mean(x, pos, n, Ttot, pre, post, up=1, down=1, include=None):
    """The beat-locked mean of the series x fp32 [R, K, Tx] by ecg_beats_series_mean (two launches, no atomics): ->
    (out fp32 [R, K, Lseg], count int32 [R]).  The positions are on the SOURCE axis of Ttot samples; source sample s reads
    series sample min(Tx - 1, s*up // down).  Entries are added in list order inside slabs of template.slab() entries and
    the slab partials ascending, then divided once by the count of listed entries with a whole segment (0 where none).
    Allocates the outputs and the workspace."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise L.EcgHipError("beats_series_mean: a CPU tensor reached the HIP input step; x must be on the GPU")
    if x.dtype != torch.float32 or x.dim() != 3:
        raise L.EcgHipError(f"beats_series_mean: x must be float32 [R, K, Tx], got {x.dtype} {tuple(x.shape)}")
    pos, n, include = _beat_list("beats_series_mean", x, pos, n, include)
    x = _contig(x)
    R, K, Tx = x.shape
    cap = pos.shape[1]
    Lseg = max(int(pre) + int(post) + 1, 0)
    out = _empty(x, R, K, Lseg)
    count = torch.empty(R, dtype=torch.int32, device=x.device)
    nbytes = int(L.query("ecg_beats_series_mean_workspace_bytes", R, K, cap, Lseg))
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=x.device)
    _call("ecg_beats_series_mean", _f32(x), L.ptr(pos), L.ptr(n), L.ptr(include), _f32(out), L.ptr(count), L.ptr(ws), R, K,
          Tx, int(Ttot), cap, int(pre), int(post), int(up), int(down), _st())
    return out, count


def overlap_mean(v, plan, Ttot, return_cover=False):
    """Per-window time series v fp32 [R, W, K, T] (windows placed by `plan`, a window_plan result) -> [R, K, Ttot]: at
    every sample the mean of the windows that cover it, added in ascending window order by the one lane that owns the
    sample (reproducible bit for bit; 0 where nothing covers).  return_cover: also the count per sample, fp32 [Ttot]."""
    first, hop, W, last_start, _ = plan
    if v.dim() != 4 or v.shape[1] != W:
        raise L.EcgHipError(f"overlap_mean: v must be [R, W={W}, K, T], got {tuple(v.shape)}")
    v = _contig(v)
    R, _, K, T = v.shape
    out = _empty(v, R, K, Ttot)
    cover = _empty(v, Ttot) if return_cover else None
    _call("ecg_windows_overlap_mean", _f32(v), _f32(out), _f32(cover), R, K, T, int(Ttot), int(first), int(hop), int(W),
          int(last_start), _st())
    return (out, cover) if return_cover else out
