"""The case table of the bf16 contract tests (include/ecg_hip.h "bf16 operand contract"): one case per
form the bf16 plan functions can return, at the smallest shape that reaches it, with the form each case must take.

Shared by tests/test_bf16_contracts_host.py (asks the form queries with integers only: the table is checked without a
device) and tests/test_gpu_bf16_contracts.py (asserts the same form, then runs the case in guarded buffers).  The forms were
derived by hand from bf16_ring_plan / bf16_cfg / tk_plan / pick_u / bf16_eval_plan; the FORM is the requirement of a case,
the shape only the way to reach it.

The sets of forms a plan can return are read from the constants of include/ecg_hip.h (header_sets), not repeated here.
"""
import ctypes
import os
import re

K, PAD = 15, 7
ROUND2, RING = 0, 1                       # ECG_BF16_CONV_*
EPI_PH, EPI_PF, EPI_GAP = 1, 2, 3         # ECG_BF16_EVAL_P_BF16 / _P_FP32 / _GAP


def up(n, m):
    return (n + m - 1) // m * m


# ---- forward ecg_conv1d_fwd_bf16_yh (statistics): (id, (N, Ci, Co, L), x_bf16, ldx, ldy, (family, co_t, t_t, resident)) --------
def _fwd(name, shape, xh, form, ldx=None, ldy=None):
    L = shape[3]
    return (name, shape, xh, (up(L, 8) if ldx is None else ldx) if xh else L, up(L, 8) if ldy is None else ldy, form)


FWD = [
    _fwd("r2_32x256_res_h", (2, 32, 32, 50), True, (ROUND2, 32, 256, 2)),
    _fwd("r2_32x256_res_f_oddL", (2, 12, 32, 51), False, (ROUND2, 32, 256, 2)),
    _fwd("r2_64x128_res", (2, 32, 64, 33), True, (ROUND2, 64, 128, 2)),
    _fwd("r2_64x128_str_3chunks", (2, 48, 64, 100), True, (ROUND2, 64, 128, 0)),
    _fwd("r2_64x128_on128", (2, 64, 128, 62), True, (ROUND2, 64, 128, 0)),
    _fwd("r2_64x256", (1, 32, 64, 161), True, (ROUND2, 64, 256, 2)),
    _fwd("r2_128x256", (1, 64, 128, 170), True, (ROUND2, 128, 256, 0)),
    # 131 tiles of one sample each on 66 persistent workgroups: ranges of 1 or 2 tiles (131 * g / 66 does not divide)
    _fwd("r2_persistent", (131, 32, 256, 16), True, (ROUND2, 64, 128, 2)),
    _fwd("ring_128x640", (1, 32, 128, 514), True, (RING, 128, 640, 0)),
    _fwd("ring_64x1280_res", (1, 32, 64, 1030), True, (RING, 64, 1280, 2)),
    _fwd("ring_64x1280_str", (1, 64, 64, 1030), True, (RING, 64, 1280, 0)),
    _fwd("ring_32x1280", (1, 32, 32, 1030), True, (RING, 32, 1280, 4)),
    _fwd("ring_f32_32x512", (2, 12, 32, 300), False, (RING, 32, 512, 1)),
    _fwd("r2_by_stride", (1, 32, 64, 1030), True, (ROUND2, 64, 256, 2), ldy=1034),
    _fwd("r2_by_chunks", (1, 48, 64, 1030), True, (ROUND2, 64, 256, 0)),
    # every base the contract allows below 16 bytes on a round-2 form: see FWD_BASES
    _fwd("r2_even_strides", (2, 32, 64, 33), True, (ROUND2, 64, 128, 2), ldx=34, ldy=34),
]
FWD_G = {"r2_persistent": 66}             # workgroups per channel tile where the case is about them
# byte offsets of (x, y) for the last case above: bf16 x and y at +4 (the contract: 4 bytes for both on round 2)
FWD_BASES = {"r2_even_strides": {"x": 4, "y": 4}}

# ---- input gradient ecg_conv1d_bwd_data_bf16hh: (id, (N, Ci, Co, L), ldy (dY), ldx (dx), form of (C_red = Co, C_res = Ci)) -----
BWD = [
    ("r2_64x128", (2, 64, 32, 33), 128, 40, (ROUND2, 64, 128, 0)),
    ("r2_128x256", (1, 128, 64, 170), 256, 176, (ROUND2, 128, 256, 0)),
    ("ring_128x640", (1, 128, 32, 514), 640, 520, (RING, 128, 640, 0)),
    ("ring_64x1280", (1, 64, 64, 1030), 1152, 1032, (RING, 64, 1280, 0)),
    ("r2_even_strides", (2, 64, 32, 33), 34, 34, (ROUND2, 64, 128, 0)),
]
BWD_BASES = {"r2_even_strides": {"dy": 4, "dx": 4}}

# ---- weight gradient ecg_conv1d_bwd_weight_bias_bf16_ncl: (id, (N, Ci, Co, L), x_bf16, ldx, (m_t, r_t, stages, splits, x fp32)) --
WGRAD = [
    ("128x512_1slab", (2, 32, 128, 130), True, 136, (128, 512, 2, 1, 0)),
    ("128x512_4slabs", (8, 32, 128, 130), True, 136, (128, 512, 2, 4, 0)),
    ("64x512_2slabs", (8, 32, 64, 70), True, 72, (64, 512, 1, 2, 0)),
    ("32x192_f32", (8, 12, 32, 64), False, 64, (32, 192, 1, 2, 1)),
    ("32x192_h_8of12", (4, 20, 32, 40), True, 40, (32, 192, 1, 1, 0)),
    ("shortest_row", (2, 32, 64, 16), True, 16, (64, 512, 1, 1, 0)),
    ("L41_ldx48", (2, 32, 64, 41), True, 48, (64, 512, 1, 1, 0)),
    ("one_live_step", (2, 32, 64, 129), True, 136, (64, 512, 2, 1, 0)),
]

# ---- row passes: (id, (N, C, L), ldp of a bf16 dp (dp_kind 0; the forward's p stride is L/2 rounded up to 8), which) -----------
# which: "f" forward + gap forward, "b" backward (all dp kinds, train and eval)
ROWS = [
    ("3x32x50", (3, 32, 50), None, "fb"),
    ("oddL", (2, 64, 33), None, "fb"),
    ("oddLp", (2, 96, 34), None, "fb"),
    ("L2", (2, 5, 2), None, "fb"),
    ("L3", (2, 5, 3), None, "fb"),
    ("ldp12", (2, 8, 18), 12, "fb"),
    ("fwd_U4", (1, 1, 14000), None, "f"),
    ("fwd_U5", (1, 1, 18000), None, "f"),
    ("fwd_U6", (1, 1, 22000), None, "f"),
    ("bwd_U4", (1, 1, 7000), None, "b"),
    ("bwd_U5", (1, 1, 9000), None, "b"),
    ("bwd_U6", (1, 1, 11000), None, "b"),
]
# U of (forward, backward reduce, backward dY pass) where the case is about it; every other case runs U = 3 (one trip)
ROWS_U = {"fwd_U4": (4, None, None), "fwd_U5": (5, None, None), "fwd_U6": (6, None, None),
          "bwd_U4": (None, 4, 4), "bwd_U5": (None, 5, 5), "bwd_U6": (None, 6, 6)}

# ---- eval blocks: (id, (N, Ci, Co, L), x_bf16, (co_t, t_t, resident)) crossed with the three epilogues ------------------------
EVAL = [
    ("128x640", (2, 32, 128, 600), True, (128, 640, 0)),
    ("128x256", (2, 32, 128, 200), True, (128, 256, 0)),
    ("128x128", (2, 32, 128, 100), True, (128, 128, 0)),
    ("64x1280_res", (1, 32, 64, 1100), True, (64, 1280, 2)),
    ("64x512_res", (2, 32, 64, 500), True, (64, 512, 2)),
    ("64x1280_str", (2, 64, 64, 100), True, (64, 1280, 0)),
    ("32x1280", (2, 32, 32, 100), True, (32, 1280, 4)),
    ("f32_32x512", (2, 12, 32, 100), False, (32, 512, 1)),
]
EPILOGUES = (EPI_PH, EPI_PF, EPI_GAP)


# ---- the form queries, asked with integers only -----------------------------------------------------------------------------
def _ask(lib, name, n, *args):
    f = (ctypes.c_int * n)()
    rc = getattr(lib, name)(*args, f)
    assert rc == 0, (name, args, lib.ecg_last_error().decode())
    return tuple(f)


def fwd_form(lib, case):
    _, (N, Ci, Co, L), xh, ldx, ldy, _ = case
    return _ask(lib, "ecg_conv1d_bf16_conv_forms", 6, N, Ci, Co, L, K, PAD, int(xh), ldx, ldy, 1)


def bwd_form(lib, case):
    _, (N, Ci, Co, L), ldy, ldx, _ = case
    return _ask(lib, "ecg_conv1d_bf16_conv_forms", 6, N, Co, Ci, L, K, K - 1 - PAD, 1, ldy, ldx, 0)


def wgrad_form(lib, case):
    _, (N, Ci, Co, L), xh, _, _ = case
    return _ask(lib, "ecg_conv1d_bwd_weight_bf16_ncl_forms", 5, N, Ci, Co, L, K, PAD, int(xh))


def rows_strides(lib, case):
    """-> (ldy of y, ldp of the forward's p, ldp of a bf16 dp, ldt of dY)"""
    _, (N, C, L), ldp0, _ = case
    return up(L, 8), up(L // 2, 8), up(L // 2, 8) if ldp0 is None else ldp0, lib.ecg_conv1d_bf16_tk_dy_stride(L)


def rows_form(lib, case):
    _, (N, C, L), _, _ = case
    _, ldp, _, ldt = rows_strides(lib, case)
    return _ask(lib, "ecg_bn_relu_pool_h_forms", 7, N, C, L, ldp, ldt)


def eval_form(lib, case, epi):
    _, (N, Ci, Co, L), xh, _ = case
    return _ask(lib, "ecg_conv1d_bn_relu_pool_eval_bf16_forms", 5, N, Ci, Co, L, K, PAD, int(xh), int(epi == EPI_PH),
                int(epi == EPI_GAP))


# ---- what the header says the plans can return --------------------------------------------------------------------------------
def header_sets():
    """{macro or enum name: value} of the form constants of include/ecg_hip.h: brace lists as sets of tuples, enums as ints."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ecg_hip.h")).read().replace("\\\n", " ")
    out = {}
    for name, body in re.findall(r"#define (ECG_B[A-Z0-9_]+)\s+(\{\{.*\}\})", text):
        out[name] = {tuple(int(v) for v in t.split(",")) for t in re.findall(r"\{([0-9, ]+)\}", body)}
    for name, value in re.findall(r"\b(ECG_B[A-Z0-9_]+) = (\d+)", text):
        out[name] = int(value)
    return out


def assert_coverage(lib):
    """The forms the case tables reach (asked of the queries, case by case: no run) are exactly the sets the header lists."""
    H = header_sets()
    assert (H["ECG_BF16_CONV_ROUND2"], H["ECG_BF16_CONV_RING"]) == (ROUND2, RING)
    assert (H["ECG_BF16_EVAL_P_BF16"], H["ECG_BF16_EVAL_P_FP32"], H["ECG_BF16_EVAL_GAP"]) == EPILOGUES
    for cases, ask in ((FWD, fwd_form), (BWD, bwd_form)):
        forms = [ask(lib, c) for c in cases]
        r2 = {f[1:3] for f in forms if f[0] == ROUND2}
        ring = {f[1:4] for f in forms if f[0] == RING}
        if cases is FWD:
            assert r2 == H["ECG_BF16_ROUND2_TILES"] and ring == H["ECG_BF16_RING_TILES"]
            # resident and streamed weights, a bf16 and an fp32 x, on round 2
            assert {(f[3], c[2]) for f, c in zip(forms, cases) if f[0] == ROUND2} == {(2, True), (2, False), (0, True)}
        else:                     # one case per family
            assert r2 <= H["ECG_BF16_ROUND2_TILES"] and ring <= H["ECG_BF16_RING_TILES"] and r2 and ring
    wg = [wgrad_form(lib, c) for c in WGRAD]
    assert {f[:2] for f in wg} == H["ECG_BF16_TK_TILES"]
    assert {f[4] for f in wg} == {0, 1} and {f[3] == 1 for f in wg} == {True, False} and {f[2] for f in wg} == {1, 2}
    us = set(range(H["ECG_BN_H_U_MIN"], H["ECG_BN_H_U_MAX"] + 1))
    rows = [(rows_form(lib, c), c[3]) for c in ROWS]
    assert {f[0] for f, w in rows if "f" in w} == us
    assert {f[2] for f, w in rows if "b" in w} == us and {f[4] for f, w in rows if "b" in w} == us
    ev = {eval_form(lib, c, e)[:3] + (e,) for c in EVAL for e in EPILOGUES}
    assert ev == {c + (e,) for c in H["ECG_BF16_EVAL_CANDIDATES"] for e in EPILOGUES}
