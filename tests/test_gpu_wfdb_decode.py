"""GPU checks of ecg_wfdb_decode16 and the raw WFDB path built on it.  Everything is integer-exact: the kernel against the
per-sample numpy decoder of tests/wfdbraw_ref.py, at sizes that sit on the kernel's edges (one workgroup owns TILE frames
and stages 20 KB of the file; wider spans are read with byte loads), and score_wfdb_record bit for bit against
score_recording on the int16 tensor the record encodes."""
import ctypes

import numpy as np
import pytest
import torch

import wfdbraw_ref as ref
from ecg_hip import wfdb16, wfdbraw
from ecg_hip.wfdb16 import WfdbFormatError
from input_util import _model, dev, hip, host  # noqa: F401

pytestmark = pytest.mark.gpu

TILE = 512          # kDecTile of csrc/wfdb_decode.hip: frames per workgroup
FORMATS = wfdbraw.FORMATS
RANGE = {16: (-32767, 32767), 61: (-32767, 32767), 160: (-32767, 32767), 80: (-127, 127), 212: (-2047, 2047)}


def stored(fmt, n, seed):
    """n stored values of the format's whole range, the invalid code among them, and their bytes."""
    lo, hi = RANGE[fmt]
    v = np.random.default_rng(seed).integers(lo - 1, hi + 1, size=n)            # lo - 1 is the invalid code
    return v, wfdbraw.encode_samples(v, fmt)


def sig(fmt, frame, slot, skew=0, offset=0, file=0):
    return wfdbraw.RawSignal(file, fmt, frame, slot, skew, offset, 200.0, 0, "mV", f"s{slot}", None, None)


def abi(raw, fmt, frame, slot, skew, col, out, n_samp, leads_out):
    """ecg_wfdb_decode16 itself, on tensors the caller owns; -> return code."""
    from ecg_hip import _lib as L
    return L.load().ecg_wfdb_decode16(raw.data_ptr(), raw.numel(), fmt, frame, L.int_table(slot), L.int_table(skew),
                                      L.int_table(col), len(col), out.data_ptr(), n_samp, leads_out, L.stream())


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_at_the_tile_edges(hip, fmt):
    for frame in (1, 2, 3, 12, 15):
        for n_samp in (1, 2, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 4099):      # frame 3 x 5 samples: 23 bytes of 212
            v, raw = stored(fmt, frame * n_samp, 1000 * frame + n_samp)
            got = hip.wfdb_decode16([dev(raw)], [sig(fmt, frame, s) for s in range(frame)], n_samp)
            want = ref.decode_file(raw, fmt, frame, range(frame), [0] * frame, range(frame), n_samp, frame)
            assert got.dtype == torch.int16 and np.array_equal(host(got), want), (frame, n_samp)
            assert np.array_equal(want.reshape(-1), np.where(v == RANGE[fmt][0] - 1, -32768, v))    # (the reference itself)


@pytest.mark.parametrize("fmt", FORMATS)
def test_raw_at_any_byte_address_and_header_offsets(hip, fmt):
    frame, n_samp = 3, 2 * TILE + 3
    _, raw = stored(fmt, frame * n_samp, fmt)
    want = ref.decode_file(raw, fmt, frame, range(frame), [0] * frame, range(frame), n_samp, frame)
    for k in (0, 1, 2, 3):
        for off in (0, 1, 7):
            buf = dev(np.concatenate([np.full(k + off, 0x5A, np.uint8), raw]))
            got = hip.wfdb_decode16([buf[k:]], [sig(fmt, frame, s, offset=off) for s in range(frame)], n_samp)
            assert np.array_equal(host(got), want), (k, off)


@pytest.mark.parametrize("fmt", FORMATS)
def test_skews_and_the_tail_they_reach_past(hip, fmt):
    frame = 3
    for skews, n_samp in (((0, 2, 5), TILE + 1), ((2, 0, 5), 7), ((TILE + 190, 0, 1), 2 * TILE + 3)):
        for extra in (0, max(skews)):               # the file holds n_samp frames, or every skewed sample as well
            _, raw = stored(fmt, frame * (n_samp + extra), fmt + n_samp + extra)
            got = host(hip.wfdb_decode16([dev(raw)], [sig(fmt, frame, s, skew=skews[s]) for s in range(frame)], n_samp))
            want = ref.decode_file(raw, fmt, frame, range(frame), skews, range(frame), n_samp, frame)
            assert np.array_equal(got, want), (skews, n_samp, extra)
            if not extra:
                for s in range(frame):
                    assert (got[max(0, n_samp - skews[s]):, s] == -32768).all()


def test_spans_wider_than_the_staged_bytes(hip):
    """512 frames of 24 two-byte signals are 24 KB, and a skew of 700 frames of 15 signals lies 21 KB away: both reach past
    the 20 KB a workgroup stages, and those samples are read with byte loads."""
    for fmt, frame, skew in ((16, 24, 0), (212, 40, 3), (61, 15, 700), (80, 64, 0)):
        n_samp = TILE + 77
        _, raw = stored(fmt, frame * n_samp, frame)
        slots = list(range(max(0, frame - 16), frame))
        skews = [skew if j % 2 else 0 for j in range(len(slots))]
        got = hip.wfdb_decode16([dev(raw)], [sig(fmt, frame, s, skew=k) for s, k in zip(slots, skews)], n_samp)
        want = ref.decode_file(raw, fmt, frame, slots, skews, range(len(slots)), n_samp, len(slots))
        assert np.array_equal(host(got), want), (fmt, frame)


@pytest.mark.parametrize("fmt", FORMATS)
def test_invalid_codes_and_their_neighbours(hip, fmt):
    code = wfdbraw.INVALID_CODE[fmt]
    v = np.array([code, code + 1, 0, code + 1, code, RANGE[fmt][1], code])
    got = host(hip.wfdb_decode16([dev(wfdbraw.encode_samples(v, fmt))], [sig(fmt, 1, 0)], v.size))[:, 0]
    assert got.tolist() == [-32768, code + 1, 0, code + 1, -32768, RANGE[fmt][1], -32768]
    assert code + 1 == {212: -2047, 80: -127}.get(fmt, -32767)


def test_column_selection_and_reorder(hip):
    n_samp = TILE + 5
    for fmt in (16, 212):
        _, raw = stored(fmt, 15 * n_samp, 15 + fmt)
        layout = [sig(fmt, 15, s) for s in range(15)]
        pick = [int(c) for c in np.random.default_rng(3).permutation(15)[:12]]
        got = hip.wfdb_decode16([dev(raw)], layout, n_samp, pick)
        assert tuple(got.shape) == (n_samp, 12)
        assert np.array_equal(host(got), ref.decode_file(raw, fmt, 15, pick, [0] * 12, range(12), n_samp, 12))
        one = hip.wfdb_decode16([dev(raw)], layout, n_samp, [13])
        assert np.array_equal(host(one), ref.decode_file(raw, fmt, 15, [13], [0], [0], n_samp, 1))


def test_two_files_into_one_stream(hip):
    n_samp = TILE + 9
    _, a = stored(212, 2 * n_samp, 31)
    _, b = stored(16, n_samp, 32)
    layout = [sig(212, 2, 0, file=0), sig(16, 1, 0, skew=2, file=1), sig(212, 2, 1, file=0)]
    got = hip.wfdb_decode16([dev(a), dev(b)], layout, n_samp)
    want = ref.decode_file(a, 212, 2, [0, 1], [0, 0], [0, 2], n_samp, 3)
    ref.decode_file(b, 16, 1, [0], [2], [1], n_samp, 3, want)
    assert np.array_equal(host(got), want)


@pytest.mark.parametrize("lead_in", [0, 1, 5])      # int16 elements before out: 16-byte aligned or not
def test_nothing_outside_out_is_written(hip, lead_in):
    n_samp, frame = TILE + 3, 3
    _, raw = stored(212, frame * n_samp, 40)
    want = ref.decode_file(raw, 212, frame, range(frame), [0] * frame, range(frame), n_samp, frame)
    for cols in ([0, 1, 2], [2, 0]):                # the whole row (wide stores), and some columns of it (the others stay)
        buf = torch.full((lead_in + n_samp * frame + 64,), 12345, dtype=torch.int16, device="cuda")
        out = buf[lead_in:lead_in + n_samp * frame]
        assert abi(dev(raw), 212, frame, cols, [0] * len(cols), cols, out, n_samp, frame) == 0
        b = host(buf)
        assert (b[:lead_in] == 12345).all() and (b[lead_in + n_samp * frame:] == 12345).all()
        got = b[lead_in:lead_in + n_samp * frame].reshape(n_samp, frame)
        assert np.array_equal(got[:, cols], want[:, cols])
        rest = [c for c in range(frame) if c not in cols]
        assert (got[:, rest] == 12345).all()


def test_byte_offsets_beyond_two_gib(hip):
    """A day at 1 kHz exceeds 2^31 bytes: 16 two-byte signals x 68 M frames.  One column is decoded whole (tile starts
    beyond 2^31 bytes), and a skew of 67 M frames is read from the far end of the file."""
    frame, n_frames = 16, (1 << 26) + 1500
    raw = torch.randint(0, 256, (2 * frame * n_frames,), dtype=torch.uint8, device="cuda")
    assert raw.numel() > (1 << 31)
    got = hip.wfdb_decode16([raw], [sig(16, frame, s) for s in range(frame)], n_frames, [11])
    assert torch.equal(got[:, 0], raw.view(torch.int16)[11::frame])
    tail = host(raw[-2 * frame * 1500:])
    skew = n_frames - 1500
    far = hip.wfdb_decode16([raw], [sig(16, frame, s, skew=skew if s == 5 else 0) for s in range(frame)], 1500 + 4, [5, 0])
    want5 = ref.decode_file(tail, 16, frame, [5], [0], [0], 1500 + 4, 1)
    assert (want5[1500:] == -32768).all() and np.array_equal(host(far[:, 0]), want5[:, 0])
    assert torch.equal(far[:, 1], raw.view(torch.int16)[0:frame * 1504:frame])


def _record(tmp_path, name, fmt, n_samp=TILE + 40, n_sig=3, seed=50, **kw):
    lo, hi = RANGE[fmt if np.isscalar(fmt) else 212]
    d = np.random.default_rng(seed).integers(lo, hi + 1, size=(n_samp, n_sig)).astype(np.int16)
    d[3, 0] = d[n_samp // 2, n_sig - 1] = -32768
    path = str(tmp_path / name)
    wfdbraw.write_raw_record(path, d, 360, np.full(n_sig, 200.0), np.arange(n_sig), fmt=fmt, **kw)
    return path, d


@pytest.mark.parametrize("fmt", FORMATS)
def test_to_device_decodes_and_verifies_checksums(hip, tmp_path, fmt):
    path, d = _record(tmp_path, "r", fmt, skew=[0, 2, 0], offset=5)
    rec = wfdbraw.read_raw_record(path)
    got, gain, base = wfdbraw.to_device(rec, "cuda")
    want = d.copy()
    want[-2:, 1] = -32768
    assert got.is_cuda and np.array_equal(host(got), want) and np.array_equal(host(got), ref.decode_record(rec))
    assert gain.dtype == np.float64 and base.dtype == np.int32 and base.tolist() == [0, 1, 2]
    sel, g2, _ = wfdbraw.to_device(rec, "cuda", leads=["sig2", 0])
    assert np.array_equal(host(sel), want[:, [2, 0]]) and g2.shape == (2,)
    # one corrupted byte of signal 0 (the record holds invalid samples as well)
    f = rec.files[0]
    f[5 + (0 if fmt != 61 else 1) + wfdbraw.stored_bytes(fmt, 3 * 20)] ^= 0x01
    with pytest.raises(WfdbFormatError, match="checksum"):
        wfdbraw.to_device(rec, "cuda")
    bad, _, _ = wfdbraw.to_device(rec, "cuda", verify_checksum=False)
    assert (host(bad) != want).sum() == 1
    wfdbraw.to_device(rec, "cuda", leads=[1, 2])                    # only the selected columns are checked


def test_abi_refusals_launch_nothing(hip):
    from ecg_hip import _lib as L
    raw = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((64,), 777, dtype=torch.int16, device="cuda")
    ok = dict(fmt=212, frame=2, slot=[0, 1], skew=[0, 0], col=[0, 1], n_samp=4, leads_out=2)
    bad = [("format", dict(fmt=24)), ("format", dict(fmt=0)), ("frame", dict(frame=0)), ("slot", dict(slot=[0, 2])),
           ("slot", dict(slot=[-1, 1])), ("skew", dict(skew=[0, -1])), ("col", dict(col=[0, 2])), ("col", dict(col=[-1, 0])),
           ("twice", dict(col=[1, 1])), ("leads_out", dict(leads_out=17, col=[0, 1])), ("leads_out", dict(leads_out=0)),
           ("Ttot", dict(n_samp=0)), ("ncols", dict(slot=[], skew=[], col=[])),
           ("ncols", dict(frame=17, slot=list(range(17)), skew=[0] * 17, col=list(range(17)), leads_out=16))]
    for word, change in bad:
        a = {**ok, **change}
        assert abi(raw, a["fmt"], a["frame"], a["slot"], a["skew"], a["col"], out, a["n_samp"], a["leads_out"]) == 1, change
        assert word in L.last_error(), (word, L.last_error())
    lib, it, st = L.load(), L.int_table, L.stream()
    assert lib.ecg_wfdb_decode16(None, 64, 212, 2, it([0, 1]), it([0, 0]), it([0, 1]), 2, out.data_ptr(), 4, 2, st) == 1
    assert "null pointer" in L.last_error()
    assert lib.ecg_wfdb_decode16(raw.data_ptr(), 64, 212, 2, None, it([0, 0]), it([0, 1]), 2, out.data_ptr(), 4, 2, st) == 1
    assert lib.ecg_wfdb_decode16(raw.data_ptr(), 64, 212, 2, it([0, 1]), it([0, 0]), it([0, 1]), 2, None, 4, 2, st) == 1
    assert lib.ecg_wfdb_decode16(raw.data_ptr(), -1, 212, 2, it([0, 1]), it([0, 0]), it([0, 1]), 2, out.data_ptr(), 4, 2, st) == 1
    assert "nbytes" in L.last_error()
    torch.cuda.synchronize()
    assert (host(out) == 777).all()
    assert abi(raw, 212, 2, [0, 1], [0, 0], [0, 1], out, 4, 2) == 0          # the accepted form of the same call
    assert host(out)[:8].tolist() == [0] * 8 and (host(out)[8:] == 777).all()
    with pytest.raises(L.EcgHipError, match="CPU tensor"):
        hip.wfdb_decode16([torch.zeros(6, dtype=torch.uint8)], [sig(212, 1, 0)], 4)


# ---- end to end -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def strip():
    """A 12-lead strip of 12-bit samples, 1500 long (window 400: a few windows), two invalid samples."""
    rng = np.random.default_rng(60)
    d = rng.integers(-2000, 2000, size=(1500, 12)).astype(np.int16)
    d[700, 4] = -32768
    return d, rng.choice([200.0, 1000.0], size=12), rng.integers(-9, 9, size=12).astype(np.int32)


def _same(a, b):
    assert a.starts == b.starts and a.fs == b.fs and len(a.starts) >= 3
    assert torch.equal(a.finite, b.finite) and not bool(a.finite.all())
    assert torch.equal(a.logits.view(torch.int32), b.logits.view(torch.int32))          # bit for bit, NaN rows included
    if b.cam is not None:
        assert torch.equal(a.cam.view(torch.int32), b.cam.view(torch.int32))


def test_score_wfdb_record_on_format_212(hip, tmp_path, strip):
    from ecg_hip.filter import FilterSpec
    from ecg_hip.recording import score_recording, score_wfdb_record
    d, gain, base = strip
    model = _model()
    path = str(tmp_path / "mit")
    wfdbraw.write_raw_record(path, d, 250, gain, base, fmt=212, offset=3)
    dd = dev(d)
    a = score_wfdb_record(path, model, window=400)
    _same(a, score_recording(model, dd, gain, base, window=400, fs=250))
    assert bool(a.finite.any())
    kw = dict(window=400, filter=FilterSpec(highpass=1.0, notch=50, width=2.0), cam_classes=[1, 3])
    _same(score_wfdb_record(path, model, model_fs=500, **kw), score_recording(model, dd, gain, base, fs=250, model_fs=500, **kw))


def test_score_wfdb_record_picks_leads_by_name(hip, tmp_path, strip):
    from ecg_hip.recording import score_wfdb_record
    d, gain, base = strip
    model = _model()
    rng = np.random.default_rng(61)
    order = rng.permutation(15)                                     # file position -> which of the 15 signals sits there
    names = list(wfdbraw.PTBXL_LEADS) + ["vx", "vy", "vz"]
    d15 = np.concatenate([d, rng.integers(-2000, 2000, size=(1500, 3)).astype(np.int16)], axis=1)
    g15, b15 = np.concatenate([gain, [500.0] * 3]), np.concatenate([base, [1, 2, 3]]).astype(np.int32)
    p15, p12 = str(tmp_path / "ptb15"), str(tmp_path / "ptb12")
    wfdbraw.write_raw_record(p15, d15[:, order], 1000, g15[order], b15[order], fmt=16,
                             sig_names=[names[i].lower() for i in order])
    wfdbraw.write_raw_record(p12, d, 1000, gain, base, fmt=16, sig_names=list(wfdbraw.PTBXL_LEADS))
    a = score_wfdb_record(p15, model, leads=wfdbraw.PTBXL_LEADS, window=400, cam_classes=[2])
    _same(a, score_wfdb_record(p12, model, window=400, cam_classes=[2]))
    with pytest.raises(WfdbFormatError, match="missing"):
        score_wfdb_record(p12, model, leads=["MLII"], window=400)


def test_plain_format_16_record_keeps_its_path_and_bits(hip, tmp_path, strip, monkeypatch):
    from ecg_hip import recording
    d, gain, base = strip
    model = _model()
    path = str(tmp_path / "plain")
    wfdb16.write_record(path, d, 250, gain, base)
    want = recording.score_recording(model, dev(d), gain, base, window=400, fs=250, cam_classes=[0])
    raw_path = recording.score_wfdb_record(path, model, leads=list(range(12)), window=400, cam_classes=[0])
    monkeypatch.setattr(wfdbraw, "read_raw_record", lambda *a, **k: pytest.fail("a plain record took the raw path"))
    _same(recording.score_wfdb_record(path, model, window=400, cam_classes=[0]), want)
    _same(raw_path, want)
