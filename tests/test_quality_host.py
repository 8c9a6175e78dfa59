"""CPU-side checks of the signal-quality gate: the numpy restatement on rows whose answers are written out here, the policy
layer (QualitySpec.judge) on a hand-built table, the rails a WFDB header gives, and the host-side refusals of
ecg_wfdb16_quality (null pointers: nothing is launched, no GPU is needed)."""
import numpy as np
import pytest
import torch

import quality_ref as qr

from ecg_hip import quality as Q
from ecg_hip.quality import QualitySpec, rails_from_header
from ecg_hip.wfdb16 import parse_header


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_field_names_agree():
    assert Q.FIELDS == qr.FIELDS and len(Q.FIELDS) == 10
    assert [Q.FIELDS[i] for i in (Q.N_INVALID, Q.VMIN, Q.VMAX, Q.SUM, Q.SUMSQ, Q.FLAT_RUN, Q.N_RAIL, Q.N_PAIRS, Q.SUM_STEP,
                                  Q.MAX_STEP)] == list(Q.FIELDS)


def test_rows_with_written_out_answers():
    #                                     n_inv vmin   vmax    sum   sumsq        flat rail pairs sumstep maxstep
    assert qr.row([7] * 9) == [0, 7, 7, 63, 441, 9, 0, 8, 0, 0]                                         # constant: flat_run == Tq
    assert qr.row([-32768] * 6) == [6, 32767, -32768, 0, 0, 6, 0, 0, 0, 0]                              # all invalid
    assert qr.row([32767, -32767]) == [0, -32767, 32767, 0, 2 * 32767 ** 2, 1, 2, 1, 65534, 65534]      # both rails, adjacent
    assert qr.row([5]) == [0, 5, 5, 5, 25, 1, 0, 0, 0, 0]                                               # Tq = 1
    assert qr.row([-32768]) == [1, 32767, -32768, 0, 0, 1, 0, 0, 0, 0]
    # runs, an invalid stretch in the middle (its neighbours form no pair across it), explicit rails
    v = [1, 1, 4, -32768, -32768, -32768, 4, 4, 4, 4, -2, 9]
    assert qr.row(v, lo=-2, hi=9) == [3, -2, 9, 1 + 1 + 4 * 5 - 2 + 9, 1 + 1 + 16 * 5 + 4 + 81, 4, 2, 7, 3 + 6 + 11, 11]


def test_the_source_span_rule():
    assert qr.starts(3, 20, 4, 58) == [3, 23, 43, 58]
    assert qr.source_starts(95, 37, 3, 20, 4, 58) == ([3, 23, 43, 58], 37)                 # up == down == 1: the plain rule
    assert qr.source_starts(1255, 200, 0, 101, 4, 302, 2, 5) == ([0, 252, 505, 755], 500)  # downsampling 5/2
    assert qr.source_starts(505, 300, 7, 151, 4, 458, 3, 2) == ([4, 105, 206, 305], 200)   # upsampling; the tail is clamped
    assert 458 * 2 // 3 == 305 and 505 - 200 == 305
    assert qr.span(300, 150, 3, 2) == 150 and Q.source_span(300, 150, 3, 2) == 150
    for T, Ttot, up, down in ((200, 1255, 2, 5), (300, 505, 3, 2), (37, 95, 1, 1), (1, 1, 1, 1), (7, 1000, 512, 511)):
        assert Q.source_span(T, Ttot, up, down) == qr.span(T, Ttot, up, down)
    d = np.arange(2 * 9 * 2, dtype=np.int16).reshape(2, 9, 2)
    q = qr.table(d, 4, 1, 2, 3, 5)
    assert q.shape == (2, 3, 2, 10) and q.dtype == np.int64
    assert list(q[1, 2, 1]) == qr.row(d[1, 5:9, 1]) and list(q[0, 1, 0]) == qr.row(d[0, 3:7, 0])


# ---------------------------------------------------------------------------------------------------------------------
# the policy layer
# ---------------------------------------------------------------------------------------------------------------------
FS, TQ, GAIN = 100, 1000, 1000.0


def good_row():
    """A clean lead at 1000 counts/mV: 1 mV peak to peak, short runs, no rail, no invalid sample."""
    return [0, -500, 500, 0, 10 ** 7, 3, 0, TQ - 1, 20000, 40]


def table_with(**changes):
    """[1, 1, 3, 10]: three clean leads, lead 1 changed by field name."""
    rows = [good_row() for _ in range(3)]
    for k, v in changes.items():
        rows[1][Q.FIELDS.index(k)] = v
    return torch.tensor([[rows]], dtype=torch.int64)


def judged(spec, q, **kw):
    ok, usable = spec.judge(q, torch.full((3,), GAIN, dtype=torch.float64), **{"fs": FS, "Tq": TQ, **kw})
    assert ok.dtype == torch.bool and usable.dtype == torch.bool
    assert tuple(ok.shape) == tuple(q.shape[:3]) and tuple(usable.shape) == tuple(q.shape[:2])
    return ok[0, 0].tolist(), bool(usable[0, 0])


@pytest.mark.parametrize("changes,off", [
    (dict(flat_run=50), "flat_s"),                      # ceil(0.5 * 100) = 50 samples
    (dict(n_rail=11), "rail_frac"),                     # > 0.01 * 1000
    (dict(vmin=-20, vmax=29), "p2p_min_mv"),            # 0.049 mV
    (dict(vmin=-5000, vmax=5001), "p2p_max_mv"),        # 10.001 mV
    (dict(n_invalid=1), "invalid_frac"),                # > 0
])
def test_each_criterion_trips_alone(changes, off):
    spec = QualitySpec()
    assert judged(spec, table_with()) == ([True, True, True], True)
    assert judged(spec, table_with(**changes)) == ([True, False, True], False)
    assert judged(QualitySpec(**{off: None}), table_with(**changes)) == ([True, True, True], True)
    assert judged(QualitySpec(max_bad_leads=1), table_with(**changes)) == ([True, False, True], True)


def test_thresholds_sit_where_the_definitions_put_them():
    spec = QualitySpec()
    assert judged(spec, table_with(flat_run=49)) == ([True, True, True], True)
    assert judged(spec, table_with(n_rail=10)) == ([True, True, True], True)            # == rail_frac * Tq: not above it
    assert judged(spec, table_with(vmin=-25, vmax=25)) == ([True, True, True], True)    # 0.05 mV: inside the closed range
    assert judged(spec, table_with(vmin=-5000, vmax=5000)) == ([True, True, True], True)
    assert judged(QualitySpec(flat_s=0.501), table_with(flat_run=50)) == ([True, True, True], True)     # ceil(50.1) = 51
    # the step criterion is off by default
    assert judged(spec, table_with(max_step=900)) == ([True, True, True], True)
    assert judged(QualitySpec(step_max_mv=0.5), table_with(max_step=501)) == ([True, False, True], False)
    assert judged(QualitySpec(step_max_mv=0.5), table_with(max_step=500)) == ([True, True, True], True)
    assert judged(QualitySpec(invalid_frac=0.1), table_with(n_invalid=100)) == ([True, True, True], True)
    assert judged(QualitySpec(invalid_frac=0.1), table_with(n_invalid=101)) == ([True, False, True], False)
    # a lead without a valid sample: vmax - vmin = -65535, below any p2p_min_mv
    assert judged(QualitySpec(invalid_frac=None, flat_s=None), table_with(vmin=32767, vmax=-32768)) == ([True, False, True], False)
    # per-recording gains: the same counts are 10.001 mV at 1000 counts/mV and 5 mV at 2000.2
    q = table_with(vmin=-5000, vmax=5001).repeat(2, 1, 1, 1)
    ok, usable = spec.judge(q, torch.tensor([[GAIN] * 3, [2000.2] * 3], dtype=torch.float64), FS, TQ)
    assert ok[:, 0, 1].tolist() == [False, True] and usable[:, 0].tolist() == [False, True]


def test_every_threshold_none_and_the_missing_rate():
    off = QualitySpec(flat_s=None, rail_frac=None, p2p_min_mv=None, p2p_max_mv=None, step_max_mv=None, invalid_frac=None)
    worst = table_with(flat_run=TQ, n_rail=TQ, vmin=32767, vmax=-32768, n_invalid=TQ, max_step=65534)
    ok, usable = off.judge(worst, [GAIN] * 3)                   # nothing set: neither fs nor Tq is needed
    assert bool(ok.all()) and bool(usable.all())
    with pytest.raises(ValueError, match="fs"):
        QualitySpec().judge(table_with(), [GAIN] * 3, None, TQ)
    with pytest.raises(ValueError, match="fs"):
        QualitySpec().judge(table_with(), [GAIN] * 3, Tq=TQ)
    with pytest.raises(ValueError, match="Tq"):
        QualitySpec().judge(table_with(), [GAIN] * 3, FS)
    QualitySpec(flat_s=None).judge(table_with(), [GAIN] * 3, Tq=TQ)     # flat_s off: no rate needed
    with pytest.raises(ValueError, match="10"):
        QualitySpec().judge(torch.zeros(1, 1, 3, 9, dtype=torch.int64), [GAIN] * 3, FS, TQ)
    assert QualitySpec() == QualitySpec(0.5, 0.01, 0.05, 10.0, None, 0.0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# rails from the header
# ---------------------------------------------------------------------------------------------------------------------
HEADER = """rec 6 360 1000
rec.dat 212 200(1024)/mV 11 1024 995 -22131 0 MLII
rec.dat 212 200 0 0 5 7 0 V5
rec.dat 212
r16.dat 16 1000.0(0)/mV 16 0 -5 12 0 I
r16.dat 16 1000.0
r80.dat 80 100 12 0 3 4 0 loud
"""


def test_adc_res_is_parsed_and_gives_the_rails():
    sigs = parse_header(HEADER)["signals"]
    assert [s["adc_res"] for s in sigs] == [11, 0, 0, 16, 0, 12]
    assert [s["adc_zero"] for s in sigs] == [1024, 0, 0, 0, 0, 0]
    lo, hi = rails_from_header(sigs)
    assert lo.dtype == np.int32 and hi.dtype == np.int32
    #                       11 bits about 1024   res 0: 212   absent: 212    16 bits          absent: 16       12 bits in format 80
    assert lo.tolist() == [0, -2048, -2048, -32768, -32768, -2048]
    assert hi.tolist() == [2047, 2047, 2047, 32767, 32767, 2047]
    fallback = [dict(fmt=f) for f in (16, 61, 160, 212, 80)]
    lo, hi = rails_from_header(fallback)
    assert lo.tolist() == [-32768, -32768, -32768, -2048, -128] and hi.tolist() == [32767, 32767, 32767, 2047, 127]
    # a selection, in the order asked
    lo, hi = rails_from_header([sigs[5], sigs[0]])
    assert lo.tolist() == [-2048, 0] and hi.tolist() == [2047, 2047]


def test_the_writer_announces_the_resolution_it_is_given(tmp_path):
    from ecg_hip import wfdbraw
    d = np.array([[2047, -2047], [5, 6], [-2047, 2047], [0, 1]])
    wfdbraw.write_raw_record(str(tmp_path / "a"), d, 250, [200.0, 200.0], [0, 0], fmt=212)
    wfdbraw.write_raw_record(str(tmp_path / "b"), d, 250, [200.0, 200.0], [0, 0], fmt=212, adc_res=12)
    res = [[s["adc_res"] for s in parse_header(open(tmp_path / f"{n}.hea").read())["signals"]] for n in "ab"]
    assert res == [[16, 16], [12, 12]]


# ---------------------------------------------------------------------------------------------------------------------
# the ABI: refused on the host, before any launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import os
    import __graft_entry__ as g
    from ecg_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def test_refusals_before_any_launch(lib):
    ok = dict(R=1, Ttot=100, leads=12, T=50, first=0, hop=25, W=3, last_start=-1, up=1, down=1, Tq=50)

    def call(lo=None, hi=None, **kw):
        a = {**ok, **kw}
        rc = lib.ecg_wfdb16_quality(None, lo, hi, None, *[a[k] for k in ok], None)
        return rc, lib.ecg_last_error().decode()

    assert call() == (1, "wfdb16_quality: null pointer")        # everything else in order: only d and q are missing
    for kw, msg in ((dict(leads=0), "leads=0"), (dict(leads=17), "leads=17"), (dict(up=0), "up=0"), (dict(up=513), "up=513"),
                    (dict(down=0), "down=0"), (dict(down=513), "down=513"), (dict(Tq=0), "Tq=0"), (dict(Tq=101), "Tq=101"),
                    (dict(Tq=49), "Tq=49 is not"), (dict(Tq=51), "Tq=51 is not"),
                    (dict(up=2, down=5, Tq=100), "longer than the recording Ttot=40"),      # the model axis has 40 samples
                    (dict(up=2, down=5, T=20, W=1, Tq=49), "Tq=49 is not"),
                    (dict(hop=0), "hop=0"), (dict(W=0), "W=0"), (dict(first=-1), "first=-1"), (dict(W=4), "past Ttot-T"),
                    (dict(last_start=51), "last_start=51"), (dict(T=101, Tq=100), "longer than"), (dict(R=0), "R=0")):
        rc, err = call(**kw)
        assert rc == 1 and msg in err, (kw, err)
    assert call(up=2, down=5, T=20, W=1, Tq=50)[1] == "wfdb16_quality: null pointer"        # ceil(20 * 5 / 2) = 50
    assert call(up=3, down=2, T=150, W=1, Tq=100)[1] == "wfdb16_quality: null pointer"      # the whole recording: Tq = Ttot
    for lo, hi in ((64, None), (None, 64)):                     # never dereferenced: refused on the host
        rc, err = call(lo, hi)
        assert rc == 1 and "rail_lo and rail_hi" in err


def test_the_tile_constant_is_exported(lib):
    assert Q.tile() == lib.ecg_wfdb16_quality_tile() and Q.tile() >= 64


def test_the_wrapper_refuses_cpu_tensors():
    from ecg_hip import EcgHipError, functional as hipF
    from ecg_hip.recording import score_recording
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hipF.wfdb16_quality(torch.zeros(1, 100, 12, dtype=torch.int16), 50, 0, 25, 3)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        score_recording(None, torch.zeros(1, 100, 12, dtype=torch.int16), None, None, window=50, quality=True)
