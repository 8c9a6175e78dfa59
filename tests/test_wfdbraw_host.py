"""Host side of the raw WFDB path (no GPU): the encoders of ecg_hip.wfdbraw against the independent per-sample decoder
of tests/wfdbraw_ref.py and the format-212 vectors of the specification, header layouts, lead selection, refusals."""
import numpy as np
import pytest

import wfdbraw_ref as ref
from ecg_hip import wfdb16, wfdbraw
from ecg_hip.wfdb16 import WfdbFormatError

RANGE = {16: (-32767, 32767), 61: (-32767, 32767), 160: (-32767, 32767), 80: (-127, 127), 212: (-2047, 2047)}


def values(fmt, shape, seed):
    lo, hi = RANGE[fmt]
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.int16)


def test_format_212_spec_vectors():
    a = bytes.fromhex("E333F3")                     # the first bytes of MIT-BIH record 100
    assert wfdbraw.encode_samples([995, 1011], 212).tobytes() == a
    assert [ref.stored_sample(np.frombuffer(a, np.uint8), 212, s) for s in range(2)] == [995, 1011]
    b = bytes.fromhex("FF0F00FF8700FB0F")           # 8 bytes, 5 samples: the file ends after b1 of the last pair
    assert wfdbraw.encode_samples([-1, 0, 2047, -2048, -5], 212).tobytes() == b
    got = [ref.stored_sample(np.frombuffer(b, np.uint8), 212, s) for s in range(7)]
    assert got == [-1, 0, 2047, -32768, -5, -32768, -32768]         # -2048 is the invalid code; 5 and 6 are past the end


@pytest.mark.parametrize("fmt", wfdbraw.FORMATS)
@pytest.mark.parametrize("n", [1, 2, 5, 15, 257])
def test_encode_then_reference_decode_round_trip(fmt, n):
    v = values(fmt, n, fmt + n)
    if n >= 5:
        v[1], v[3] = RANGE[fmt][0], RANGE[fmt][1]
    raw = wfdbraw.encode_samples(v, fmt)
    assert raw.dtype == np.uint8 and raw.size == wfdbraw.stored_bytes(fmt, n)
    assert [ref.stored_sample(raw, fmt, s) for s in range(n)] == v.tolist()
    assert ref.stored_sample(raw, fmt, n) == -32768
    code = wfdbraw.INVALID_CODE[fmt]
    raw = wfdbraw.encode_samples(np.array([code] * n), fmt)
    assert [ref.stored_sample(raw, fmt, s) for s in range(n)] == [-32768] * n
    with pytest.raises(ValueError):
        wfdbraw.encode_samples([RANGE[fmt][1] + 1], fmt)


def test_header_layouts_two_files_skews_and_offset(tmp_path):
    d = np.concatenate([values(212, (41, 2), 1), values(16, (41, 1), 2)], axis=1)
    d[7, 0] = d[9, 2] = -32768
    path = str(tmp_path / "two")
    wfdbraw.write_raw_record(path, d, 360, [200.0, 100.0, 1000.0], [0, 5, -3], fmt=[212, 16], files=[0, 0, 1],
                             skew=[0, 3, 2], offset=[7, 1], sig_names=["MLII", "V 5", "resp"], units=["mV", "mV", "NU"])
    rec = wfdbraw.read_raw_record(path)
    assert rec.fs == 360 and rec.n_samp == 41 and rec.n_sig == 3 and rec.file_names == ["two_0.dat", "two_1.dat"]
    assert [(s.file, s.fmt, s.frame, s.slot, s.skew, s.offset) for s in rec.signals] == [
        (0, 212, 2, 0, 0, 7), (0, 212, 2, 1, 3, 7), (1, 16, 1, 0, 2, 1)]
    assert [s.gain for s in rec.signals] == [200.0, 100.0, 1000.0] and [s.baseline for s in rec.signals] == [0, 5, -3]
    assert rec.sig_names == ["MLII", "V 5", "resp"] and rec.signals[2].units == "NU"
    assert rec.files[0].dtype == np.uint8 and rec.files[0].size == 7 + 3 * 41 and rec.files[1].size == 1 + 2 * 41
    want = d.copy()
    want[41 - 3:, 1] = -32768                       # the skewed tails are not in the files
    want[41 - 2:, 2] = -32768
    got = ref.decode_record(rec)
    assert np.array_equal(got, want)
    # the checksum identity to_device verifies: sum(d) + count(-32768) * (code + 32768), folded
    for j, s in enumerate(rec.signals):
        fix = int(got[:, j].astype(np.int64).sum()) + int((got[:, j] == -32768).sum()) * (wfdbraw.INVALID_CODE[s.fmt] + 32768)
        assert wfdbraw.fold16(fix) == s.checksum
    assert np.array_equal(ref.decode_record(rec, [2, 0]), want[:, [2, 0]])


def test_checksum_identity_for_212_with_two_invalid_samples():
    v = np.array([5, -2048, 100, -2048, -7, 2047])
    dec = np.array([ref.stored_sample(wfdbraw.encode_samples(v, 212), 212, s) for s in range(6)], np.int64)
    assert (dec == -32768).sum() == 2
    assert dec.sum() + 2 * (-2048 + 32768) == v.sum()


def test_n_samp_from_the_shortest_file(tmp_path):
    path = str(tmp_path / "r")
    wfdbraw.write_raw_record(path, values(212, (9, 3), 3), 250, [200.0] * 3, [0] * 3, fmt=212)
    hea = open(path + ".hea").read().splitlines()
    open(path + ".hea", "w").write("\n".join(["r 3 250"] + hea[1:]) + "\n")
    assert wfdbraw.read_raw_record(path).n_samp == 9          # 41 bytes: 27 samples, the last in two bytes


def test_plain_format_16_equals_wfdb16(tmp_path):
    d = values(16, (300, 12), 4)
    d[5, 5] = -32768
    path = str(tmp_path / "p")
    wfdb16.write_record(path, d, 500, np.full(12, 1000.0), np.arange(12, dtype=np.int32))
    old = wfdb16.read_record(path)
    rec = wfdbraw.read_raw_record(path)
    assert np.array_equal(ref.decode_record(rec), old.d) and rec.fs == old.fs
    assert [s.checksum for s in rec.signals] == old.checksums
    assert np.array_equal([s.gain for s in rec.signals], old.gain) and np.array_equal([s.baseline for s in rec.signals], old.baseline)


def test_wfdb16_still_refuses_212(tmp_path):
    path = str(tmp_path / "q")
    wfdbraw.write_raw_record(path, values(212, (10, 2), 5), 360, [200.0] * 2, [0] * 2, fmt=212)
    with pytest.raises(WfdbFormatError, match="format 16"):
        wfdb16.read_record(path)


def _rewrite(path, fn):
    lines = open(path + ".hea").read().splitlines()
    open(path + ".hea", "w").write("\n".join(fn(lines)) + "\n")


@pytest.mark.parametrize("fmt,why", [(8, "format 8"), (24, "format 24"), (32, "format 32"), (310, "format 310"),
                                     (311, "format 311"), (99, "unknown format")])
def test_refused_formats(tmp_path, fmt, why):
    path = str(tmp_path / "r")
    wfdbraw.write_raw_record(path, values(16, (10, 2), 6), 360, [200.0] * 2, [0] * 2, fmt=16)
    _rewrite(path, lambda ls: [ls[0]] + [ln.replace(".dat 16 ", f".dat {fmt} ") for ln in ls[1:]])
    with pytest.raises(WfdbFormatError, match=why):
        wfdbraw.read_raw_record(path)


def test_other_refusals(tmp_path):
    path = str(tmp_path / "r")
    d = values(212, (10, 2), 7)

    def fresh(**kw):
        wfdbraw.write_raw_record(path, d, 360, [200.0] * 2, [0] * 2, **{"fmt": 212, **kw})

    fresh()
    _rewrite(path, lambda ls: [ls[0], ls[1].replace(".dat 212 ", ".dat 212x2 "), ls[2]])
    with pytest.raises(WfdbFormatError, match="samples per frame"):
        wfdbraw.read_raw_record(path)
    fresh()
    _rewrite(path, lambda ls: [ls[0].replace("r 2", "r/3 2")] + ls[1:])
    with pytest.raises(WfdbFormatError, match="multi-segment"):
        wfdbraw.read_raw_record(path)
    fresh(fmt=16)
    _rewrite(path, lambda ls: [ls[0], ls[1].replace(".dat 16 ", ".dat 61 "), ls[2]])
    with pytest.raises(WfdbFormatError, match="different formats"):
        wfdbraw.read_raw_record(path)
    fresh(offset=4)
    _rewrite(path, lambda ls: [ls[0], ls[1].replace("212+4", "212+6"), ls[2]])
    with pytest.raises(WfdbFormatError, match="different byte offsets"):
        wfdbraw.read_raw_record(path)
    fresh()
    _rewrite(path, lambda ls: [ls[0].replace(" 10", " 11")] + ls[1:])
    with pytest.raises(WfdbFormatError, match="too short"):
        wfdbraw.read_raw_record(path)
    fresh(skew=[0, 4])                              # a skewed tail is not "too short"
    assert wfdbraw.read_raw_record(path).n_samp == 10


def test_select_leads(tmp_path):
    names = ["i", "II", " iii", "aVR", "AVL", "avf", "v1", "v2", "v3", "v4", "v5", "v6", "vx", "vy", "vz"]
    order = np.random.default_rng(8).permutation(15)
    path = str(tmp_path / "ptb")
    wfdbraw.write_raw_record(path, values(16, (6, 15), 9), 1000, [2000.0] * 15, [0] * 15, fmt=16,
                             sig_names=[names[i] for i in order])
    rec = wfdbraw.read_raw_record(path)
    cols = wfdbraw.select_leads(rec, wfdbraw.PTBXL_LEADS)
    assert [rec.sig_names[c].strip().upper() for c in cols] == list(wfdbraw.PTBXL_LEADS)
    assert wfdbraw.select_leads(rec, ["VZ", 3, "a v r"]) == [list(order).index(14), 3, list(order).index(3)]
    with pytest.raises(WfdbFormatError, match="missing.*vx"):
        wfdbraw.select_leads(rec, ["MLII"])
    with pytest.raises(WfdbFormatError, match="outside"):
        wfdbraw.select_leads(rec, [15])
    wfdbraw.write_raw_record(path, values(16, (6, 3), 9), 1000, [2000.0] * 3, [0] * 3, fmt=16, sig_names=["II", "V1", "ii"])
    with pytest.raises(WfdbFormatError, match="ambiguous.*V1"):
        wfdbraw.select_leads(wfdbraw.read_raw_record(path), ["II"])


def test_functional_wrapper_refuses_cpu_tensors():
    import torch
    from ecg_hip import EcgHipError, functional as F
    sig = wfdbraw.RawSignal(0, 212, 1, 0, 0, 0, 200.0, 0, "mV", "x", None, None)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        F.wfdb_decode16([torch.zeros(6, dtype=torch.uint8)], [sig], 4)
