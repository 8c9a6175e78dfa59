"""WFDB records in any storage format whose samples fit 16 bits — 16, 61, 80, 160 and 212 — with skews, byte offsets, several
.dat files and more signals than the model has leads.  What ecg_hip.wfdb16 refuses, for the recordings the resampler and the
filter were built for: MIT-BIH Arrhythmia (212, 360 Hz), AFDB (212, 250 Hz), LTAFDB (212, 128 Hz), PTB Diagnostic (16,
1000 Hz, 12 + 3 Frank leads).

The host never interprets a sample: `read_raw_record` parses the header (wfdb16.parse_header) and reads every .dat file as
bytes; `to_device` uploads those bytes once and `functional.wfdb_decode16` (ecg_wfdb_decode16, csrc/wfdb_decode.hip) turns
them into the int16 [n_samp, leads] stream `score_recording` and the window entry points read.  The header checksums are
verified on the device, on the decoded tensor.

Layout rules (header(5), signal(5)): the signals of one file are interleaved by time, `frame` samples per time frame, signal
`slot` at that position of every frame; a signal with skew k is stored k frames late, so its sample t is stored sample
(t + k)*frame + slot of the file; `+offset` bytes precede the first sample.  Storage of stored sample s:
    16   little-endian int16 at byte 2s                    invalid sample: -32768
    61   big-endian int16 at byte 2s                       invalid sample: -32768
    160  little-endian uint16 at byte 2s, minus 32768      invalid sample: -32768
    80   byte s, minus 128                                 invalid sample: -128
    212  pair p = s >> 1 in bytes b0 b1 b2 at 3p: even s = b0 | (b1 & 0x0F) << 8, odd s = b2 | (b1 & 0xF0) << 4, sign-
         extended from 12 bits; a file with an odd sample count ends after b1.   invalid sample: -2048
Decoded, the invalid code of every format is -32768 (a NaN lead sample to the kernels), and so is every sample past the end
of the file's bytes: with a skew of k, the last k samples of that signal when the file holds n_samp frames.
"""
import os
from dataclasses import dataclass, field
from typing import List

import numpy as np

from .wfdb16 import WfdbFormatError, parse_header

FORMATS = (16, 61, 80, 160, 212)
INVALID_CODE = {16: -32768, 61: -32768, 160: -32768, 80: -128, 212: -2048}
_VALUE_RANGE = {16: (-32768, 32767), 61: (-32768, 32767), 160: (-32768, 32767), 80: (-128, 127), 212: (-2048, 2047)}
_REFUSED = {8: "first differences, not samples", 24: "24-bit samples do not fit the int16 stream",
            32: "32-bit samples do not fit the int16 stream", 310: "10-bit packing is not implemented",
            311: "10-bit packing is not implemented"}
PTBXL_LEADS = ("I", "II", "III", "AVR", "AVL", "AVF", "V1", "V2", "V3", "V4", "V5", "V6")


@dataclass
class RawSignal:
    file: int               # index into RawRecord.files
    fmt: int
    frame: int              # signals interleaved in that file
    slot: int               # position inside a frame
    skew: int
    offset: int             # bytes before the file's first sample
    gain: float
    baseline: int
    units: str
    description: str
    checksum: object        # int, or None when the header has none
    init_value: object


@dataclass
class RawRecord:
    name: str
    fs: float
    n_samp: int
    signals: List[RawSignal]
    files: List[np.ndarray]                     # uint8, the bytes of each .dat file as they are
    file_names: List[str] = field(default_factory=list)

    @property
    def n_sig(self):
        return len(self.signals)

    @property
    def sig_names(self):
        return [s.description for s in self.signals]


def stored_bytes(fmt, n_stored):
    """Bytes that n_stored samples occupy in a file of this format."""
    return {16: 2 * n_stored, 61: 2 * n_stored, 160: 2 * n_stored, 80: n_stored, 212: (3 * n_stored + 1) // 2}[fmt]


def _stored_samples(fmt, nbytes):
    """Whole samples in nbytes bytes."""
    if fmt == 80:
        return nbytes
    if fmt == 212:
        return (nbytes // 3) * 2 + (1 if nbytes % 3 == 2 else 0)
    return nbytes // 2


def read_raw_record(record_path):
    """record_path without extension -> RawRecord: the parsed header and the bytes of every .dat file, not interpreted."""
    with open(record_path + ".hea", "r") as f:
        hdr = parse_header(f.read())            # (refuses multi-segment records)
    if hdr["n_sig"] < 1:
        raise WfdbFormatError(f"{record_path}: no signals")
    names, per_file = [], {}
    for i, s in enumerate(hdr["signals"]):
        fmt = s["fmt"]
        if fmt not in FORMATS:
            raise WfdbFormatError(f"{record_path}: signal {i} is stored in format {fmt}: "
                                  f"{_REFUSED.get(fmt, 'unknown format')} (supported: {', '.join(map(str, FORMATS))})")
        if s["spf"] != 1:
            raise WfdbFormatError(f"{record_path}: signal {i} has {s['spf']} samples per frame; only 1 is supported")
        if s["file"] not in per_file:
            per_file[s["file"]] = []
            names.append(s["file"])
        per_file[s["file"]].append(i)
    for name, idx in per_file.items():
        first = hdr["signals"][idx[0]]
        for i in idx[1:]:
            s = hdr["signals"][i]
            if s["fmt"] != first["fmt"]:
                raise WfdbFormatError(f"{record_path}: the signals of {name} are stored in different formats "
                                      f"({first['fmt']} and {s['fmt']})")
            if s["offset"] != first["offset"]:
                raise WfdbFormatError(f"{record_path}: the signals of {name} give different byte offsets "
                                      f"({first['offset']} and {s['offset']})")
    folder = os.path.dirname(record_path)
    files = [np.fromfile(os.path.join(folder, name), dtype=np.uint8) for name in names]
    frames = []
    for name, raw in zip(names, files):
        first = hdr["signals"][per_file[name][0]]
        frames.append(_stored_samples(first["fmt"], max(0, raw.size - first["offset"])) // len(per_file[name]))
    n_samp = hdr["n_samp"] if hdr["n_samp"] is not None else min(frames)
    if n_samp < 1:
        raise WfdbFormatError(f"{record_path}: no samples")
    for name, have in zip(names, frames):
        if have < n_samp:
            raise WfdbFormatError(f"{os.path.join(folder, name)}: too short, {have} whole frames on disk and the header "
                                  f"promises {n_samp}")
    signals = []
    for i, s in enumerate(hdr["signals"]):
        idx = per_file[s["file"]]
        signals.append(RawSignal(file=names.index(s["file"]), fmt=s["fmt"], frame=len(idx), slot=idx.index(i),
                                 skew=s["skew"], offset=s["offset"], gain=s["gain"], baseline=s["baseline"],
                                 units=s["units"], description=s["description"], checksum=s["checksum"],
                                 init_value=s["init_value"]))
    return RawRecord(name=hdr["name"], fs=hdr["fs"], n_samp=int(n_samp), signals=signals, files=files, file_names=names)


def _norm(name):
    return "".join(str(name).split()).upper()


def select_leads(rec, leads):
    """Column indices of `leads` in rec, in the order asked: ints are taken as they are, names are matched against the
    header's signal descriptions, case-insensitively and ignoring blanks."""
    have = [_norm(n) for n in rec.sig_names]
    out = []
    for want in leads:
        if isinstance(want, (int, np.integer)):
            if not 0 <= int(want) < rec.n_sig:
                raise WfdbFormatError(f"signal index {int(want)} outside the record's {rec.n_sig} signals")
            out.append(int(want))
            continue
        hits = [i for i, h in enumerate(have) if h == _norm(want)]
        if len(hits) != 1:
            raise WfdbFormatError(f"lead {want!r} is {'missing' if not hits else 'ambiguous (' + str(len(hits)) + ' signals)'}"
                                  f" in record {rec.name}; it has {rec.sig_names}")
        out.append(hits[0])
    return out


def fold16(v):
    """An integer sum as the signed 16-bit value a WFDB header stores."""
    return ((int(v) + 32768) % 65536) - 32768


def to_device(rec, device, leads=None, verify_checksum=True):
    """-> (d int16 [n_samp, L] on `device`, gain float64 [L], baseline int32 [L]) for the selected leads (select_leads;
    default: every signal, in header order).  The files' bytes are uploaded once and decoded by the HIP kernel; only the
    files that hold a selected signal travel.  The header checksums of the selected signals are verified on the device: a
    header checksum is the sum of the STORED values, the decoded tensor holds -32768 where the format's invalid code (or
    nothing: a skewed tail) was stored, so per column  sum(d) + count(d == -32768) * (code + 32768)  folded to 16 bits
    must equal it.  The packed bytes are dropped after decoding."""
    import torch
    from . import functional as hipF
    cols = list(range(rec.n_sig)) if leads is None else select_leads(rec, leads)
    used = {rec.signals[c].file for c in cols}
    files = [torch.from_numpy(f).to(device) if i in used else torch.empty(0, dtype=torch.uint8, device=device)
             for i, f in enumerate(rec.files)]
    d = hipF.wfdb_decode16(files, rec.signals, rec.n_samp, cols)
    del files
    if verify_checksum:
        sums = d.sum(0, dtype=torch.int64)
        invalid = (d == -32768).sum(0, dtype=torch.int64)
        code = torch.tensor([INVALID_CODE[rec.signals[c].fmt] + 32768 for c in cols], dtype=torch.int64, device=d.device)
        got = (sums + invalid * code).tolist()
        for j, c in enumerate(cols):
            want = rec.signals[c].checksum
            if want is not None and fold16(got[j]) != fold16(want):
                raise WfdbFormatError(f"{rec.name}: checksum mismatch on signal {c} ({rec.signals[c].description!r}): "
                                      f"header {want}, data {fold16(got[j])}")
    gain = np.array([rec.signals[c].gain for c in cols], np.float64)
    baseline = np.array([rec.signals[c].baseline for c in cols], np.int32)
    return d, gain, baseline


def encode_samples(v, fmt):
    """Stored values v (a flat integer array, in storage order) -> the bytes of a file of this format."""
    v = np.asarray(v, dtype=np.int64).reshape(-1)
    lo, hi = _VALUE_RANGE[fmt]
    if v.size and (v.min() < lo or v.max() > hi):
        raise ValueError(f"format {fmt} stores [{lo}, {hi}]; got [{v.min()}, {v.max()}]")
    if fmt == 16:
        return v.astype("<i2").view(np.uint8)
    if fmt == 61:
        return v.astype(">i2").view(np.uint8)
    if fmt == 160:
        return (v + 32768).astype("<u2").view(np.uint8)
    if fmt == 80:
        return (v + 128).astype(np.uint8)
    u = (v & 0xFFF).astype(np.uint16)
    even, odd = u[0::2], u[1::2]
    out = np.zeros(3 * even.size, np.uint8)
    out[0::3] = even & 0xFF
    out[1::3] = even >> 8
    out[1:3 * odd.size:3] |= ((odd >> 8) << 4).astype(np.uint8)
    out[2:3 * odd.size:3] = odd & 0xFF
    return out[:stored_bytes(212, v.size)]


def write_raw_record(record_path, d, fs, gain, baseline, fmt=212, skew=None, offset=0, files=None, units=None,
                     sig_names=None, adc_res=16):
    """Write d integer [n_samp, n_sig] (the values as they DECODE; -32768 marks an invalid sample and is stored as the
    format's invalid code) as <record_path>.hea and its .dat files.

    fmt, offset: one value, or one per FILE.  files: for every signal the index of its file (default: all in file 0);
    file k is <name>.dat for one file, else <name>_k.dat.  skew: frames per signal (default 0).
    adc_res: the ADC resolution in bits the signal lines announce (one value).  Every file holds
    n_samp frames: signal sample t is stored in frame t + skew, the first `skew` frames of that slot hold the invalid
    code and the last `skew` samples are NOT stored — they read back as invalid, and the header checksum counts them as
    the invalid code, like the samples that are stored as such.  `offset` bytes of 0xA5 precede the samples."""
    d = np.asarray(d)
    n_samp, n_sig = d.shape
    files = [0] * n_sig if files is None else [int(f) for f in files]
    n_files = max(files) + 1
    fmts = [int(fmt)] * n_files if np.isscalar(fmt) else [int(f) for f in fmt]
    offsets = [int(offset)] * n_files if np.isscalar(offset) else [int(o) for o in offset]
    skew = [0] * n_sig if skew is None else [int(k) for k in skew]
    units = units or ["mV"] * n_sig
    sig_names = sig_names or [f"sig{i}" for i in range(n_sig)]
    name = os.path.basename(record_path)
    folder = os.path.dirname(record_path)
    fnames = [f"{name}.dat" if n_files == 1 else f"{name}_{k}.dat" for k in range(n_files)]
    lines = {}
    for k in range(n_files):
        members = [i for i in range(n_sig) if files[i] == k]
        code = INVALID_CODE[fmts[k]]
        stored = np.full((n_samp, len(members)), code, np.int64)
        for slot, i in enumerate(members):
            v = d[:, i].astype(np.int64)
            v = np.where(v == -32768, code, v)
            keep = max(0, n_samp - skew[i])
            stored[skew[i]:skew[i] + keep, slot] = v[:keep]
            as_read = np.concatenate([v[:keep], np.full(n_samp - keep, code, np.int64)])
            spec = f"{fmts[k]}" + (f":{skew[i]}" if skew[i] else "") + (f"+{offsets[k]}" if offsets[k] else "")
            lines[i] = (f"{fnames[k]} {spec} {float(gain[i])!r}({int(baseline[i])})/{units[i]} {int(adc_res)} 0 "
                        f"{int(as_read[0])} {fold16(as_read.sum())} 0 {sig_names[i]}\n")
        body = encode_samples(stored.reshape(-1), fmts[k])
        np.concatenate([np.full(offsets[k], 0xA5, np.uint8), body]).tofile(os.path.join(folder, fnames[k]))
    with open(record_path + ".hea", "w") as f:
        f.write(f"{name} {n_sig} {fs:g} {n_samp}\n")
        for i in range(n_sig):
            f.write(lines[i])
