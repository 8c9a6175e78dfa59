"""Independent numpy restatement of ecg_wfdb_decode16 (include/ecg_hip.h): one Python loop per output sample over the
storage rules, written from the format descriptions — not the encoder of ecg_hip.wfdbraw run backwards."""
import numpy as np

INVALID = -32768
CODE = {16: -32768, 61: -32768, 160: -32768, 80: -128, 212: -2048}


def stored_sample(raw, fmt, s):
    """Stored sample number s of the bytes `raw` (uint8), or INVALID when its bytes are not all there / it is the
    format's invalid code."""
    if not isinstance(raw, bytes):
        raw = np.asarray(raw, np.uint8).tobytes()
    n = len(raw)

    def byte(i):
        return raw[i]

    if fmt in (16, 61, 160):
        if 2 * s + 2 > n:
            return INVALID
        a, b = byte(2 * s), byte(2 * s + 1)
        if fmt == 61:
            a, b = b, a
        u = a + 256 * b
        v = u - 32768 if fmt == 160 else (u - 65536 if u >= 32768 else u)
    elif fmt == 80:
        if s + 1 > n:
            return INVALID
        v = byte(s) - 128
    elif fmt == 212:
        p = s // 2
        if s % 2 == 0:
            if 3 * p + 2 > n:
                return INVALID
            u = byte(3 * p) + 256 * (byte(3 * p + 1) % 16)
        else:
            if 3 * p + 3 > n:
                return INVALID
            u = byte(3 * p + 2) + 256 * (byte(3 * p + 1) // 16)
        v = u - 4096 if u >= 2048 else u
    else:
        raise ValueError(fmt)
    return INVALID if v == CODE[fmt] else v


def decode_file(raw, fmt, frame, slot, skew, col, n_samp, leads_out, out=None):
    """One ecg_wfdb_decode16 call: out[t, col[j]] = stored sample (t + skew[j])*frame + slot[j]."""
    if out is None:
        out = np.zeros((n_samp, leads_out), np.int16)
    raw = np.asarray(raw, np.uint8).tobytes()
    for j in range(len(col)):
        for t in range(n_samp):
            out[t, col[j]] = stored_sample(raw, fmt, (t + skew[j]) * frame + slot[j])
    return out


def decode_record(rec, columns=None):
    """ecg_hip.wfdbraw.RawRecord -> int16 [n_samp, len(columns)], as functional.wfdb_decode16 defines it."""
    columns = list(range(len(rec.signals))) if columns is None else list(columns)
    out = np.zeros((rec.n_samp, len(columns)), np.int16)
    for j, c in enumerate(columns):
        s = rec.signals[c]
        decode_file(rec.files[s.file][s.offset:], s.fmt, s.frame, [s.slot], [s.skew], [j], rec.n_samp, len(columns), out)
    return out
