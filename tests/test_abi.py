"""CPU-side checks of the C-ABI boundary: libecg_hip.so loads, exports every symbol that
include/ecg_hip.h declares, and validates arguments on the host before any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from ecg_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "ecg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ecg_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from ecg_hip import _lib
    declared = _header_symbols()
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/ecg_hip.h but not exported"
    assert sorted(_lib.SIGNATURES) == declared, "ctypes table and header disagree"


def test_version_and_error_channel(lib):
    assert lib.ecg_version() == 100
    rc = lib.ecg_conv1d_fwd(None, None, None, None, None, 1, 12, 32, 100, 40, 7, None)
    assert rc == 1      # ECG_EINVAL: kernel size outside [1,31]; rejected before any launch
    assert b"kernel size" in lib.ecg_last_error()
    rc = lib.ecg_conv1d_fwd(None, None, None, None, None, 1, 12, 32, 100, 15, 7, None)
    assert rc == 1 and b"null pointer" in lib.ecg_last_error()
    rc = lib.ecg_conv1d_fwd(None, None, None, None, None, 1, 12, 32, 3, 15, 2, None)
    assert rc == 1 and b"empty output" in lib.ecg_last_error()
    rc = lib.ecg_adamw_step(None, None, None, None, 16, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None)
    assert rc == 1


def test_size_helpers_are_pure(lib):
    assert lib.ecg_conv1d_fwd_stat_partials(256, 12, 32, 1000, 15, 7) > 0
    assert lib.ecg_conv1d_bwd_weight_ws_floats(256, 12, 32, 1000, 15, 7) >= 32 * 12 * 15 + 32
    assert lib.ecg_bn_relu_pool_bwd_ws_floats(256, 32, 1000) >= 32 * 2
    assert lib.ecg_bn_stat_partials_count(4, 32, 100) >= 1


def test_kernel_wrappers_refuse_cpu_tensors_but_modules_route_them_to_stock_torch():
    """The ABI wrappers never see a CPU tensor: the nn modules send those to the stock torch layer they inherit
    from (tests/test_cpu_path.py checks the numbers); a CPU tensor handed to a Function directly still raises."""
    import torch
    from ecg_hip import EcgHipError, functional as hipF
    from src.models.ecg_cnn import ECGCNN
    assert ECGCNN(num_labels=5)(torch.randn(2, 12, 64)).shape == (2, 5)
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hipF.ReLUFn.apply(torch.zeros(4))
    with pytest.raises(EcgHipError, match="CPU tensor"):
        hipF.BceWithLogitsFn.apply(torch.zeros(2, 5), torch.zeros(2, 5), None, 1.0)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from ecg_hip import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.EcgHipError, match="missing"):
        _lib.load()


def test_one_launch_batchnorm_backward_is_decided_per_call_from_the_parameters(monkeypatch):
    """No process-wide switch in the library any more: ConvBlockFn.backward picks the one-launch or the two-pass entry
    point per call.  Parameters declared "busy" (hooks issue all-reduces under backward) take two passes, "quiet" ones the
    one-launch form; undeclared parameters are quiet in a single-rank process and busy as soon as more than one rank
    exists (stock DistributedDataParallel users get the safe form without asking)."""
    import torch
    from ecg_hip import functional as F, params as P
    monkeypatch.setattr(P, "_bn_one_launch", True)
    monkeypatch.setattr(P, "_records", {})
    monkeypatch.setattr(P, "_by_ptr", {})
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3))
    ka, kb = a.data_ptr(), b.data_ptr()
    assert F.bn_backward_one_launch_allowed(ka) and F.bn_backward_one_launch_allowed(kb)
    F.declare_backward_collectives([a], True)
    assert not F.bn_backward_one_launch_allowed(ka) and F.bn_backward_one_launch_allowed(kb)      # per parameter, not global
    F.declare_backward_collectives([a], False)
    assert F.bn_backward_one_launch_allowed(ka)
    monkeypatch.setattr(P, "_multi_rank", lambda: True)
    assert F.bn_backward_one_launch_allowed(ka) and not F.bn_backward_one_launch_allowed(kb)      # undeclared + multi-rank
    F.declare_backward_collectives([a], None)
    assert not F.bn_backward_one_launch_allowed(ka)
    monkeypatch.setattr(P, "_multi_rank", lambda: False)
    assert F.set_bn_backward_one_launch(False) is True
    assert not F.bn_backward_one_launch_allowed(ka) and not F.bn_backward_one_launch_allowed(kb)
    assert F.set_bn_backward_one_launch(True) is False
    # statements follow the parameter OBJECT: an optimizer that re-homes the storage afterwards (FlatAdamW, the adopted stock
    # AdamW) does not leave a wrapper's statement on a dead address, and an owner only withdraws what it said itself
    from ecg_hip.optim import flatten_tensors_
    monkeypatch.setattr(P, "_multi_rank", lambda: True)
    F.declare_backward_collectives([a, b], False, owner="wrapper")
    old = (a.data_ptr(), b.data_ptr())
    flat = flatten_tensors_([a, b])
    F.parameters_rehomed()               # (flatten_tensors_ calls it for device tensors)
    assert a.data_ptr() == flat.data_ptr() and a.data_ptr() != old[0]
    assert F.bn_backward_one_launch_allowed(a.data_ptr()) and F.bn_backward_one_launch_allowed(b.data_ptr())
    assert not F.bn_backward_one_launch_allowed(old[1])           # the abandoned address is undeclared again
    F.declare_backward_collectives([a, b], None, owner="optimizer")   # somebody else's withdrawal: no effect
    assert F.bn_backward_one_launch_allowed(a.data_ptr())
    F.declare_backward_collectives([id(a), id(b)], None, "wrapper")   # the finalizer's form: ids + the owner's token
    assert not F.bn_backward_one_launch_allowed(a.data_ptr())


# (setting, variant) -> per T the four blocks as "<input kind>:<form>"; input kinds: f = fp32 the kernels read in place,
# o = other fp32 (not 8-byte aligned), h = bf16 rows handed on by the block before
_BLOCK_FORMS = {
    ("train", "plain"): {1000: "f:fp32 f:fp32 f:fp32 f:fp32", 5000: "f:fp32 f:fp32 f:fp32 f:fp32", 12000: "f:fp32 f:fp32 f:fp32 f:fp32"},
    ("train", "bn2_frozen"): {1000: "f:fp32 f:fp32 f:fp32 f:fp32", 5000: "f:fp32 f:fp32 f:fp32 f:fp32", 12000: "f:fp32 f:fp32 f:fp32 f:fp32"},
    ("train", "dx0"): {1000: "f:fp32 f:fp32 f:fp32 f:fp32", 5000: "f:fp32 f:fp32 f:fp32 f:fp32", 12000: "f:fp32 f:fp32 f:fp32 f:fp32"},
    ("train", "unaligned"): {1000: "o:fp32 f:fp32 f:fp32 f:fp32", 5000: "o:fp32 f:fp32 f:fp32 f:fp32", 12000: "o:fp32 f:fp32 f:fp32 f:fp32"},
    ("eval", "plain"): {1000: "f:eval f:eval f:eval f:eval", 5000: "f:eval f:eval f:eval f:fp32", 12000: "f:eval f:eval f:eval f:fp32"},
    ("eval", "unaligned"): {1000: "o:eval f:eval f:eval f:eval", 5000: "o:eval f:eval f:eval f:fp32", 12000: "o:eval f:eval f:eval f:fp32"},
    ("bf16_train", "plain"): {1000: "f:bf16 h:bf16 h:bf16 h:bf16", 5000: "f:bf16 h:bf16 h:bf16 h:bf16", 12000: "f:bf16 h:bf16 h:bf16 h:bf16"},
    ("bf16_train", "bn2_frozen"): {1000: "f:bf16 h:bf16 f:fp32 f:bf16", 5000: "f:bf16 h:bf16 f:fp32 f:bf16", 12000: "f:bf16 h:bf16 f:fp32 f:bf16"},
    ("bf16_train", "dx0"): {1000: "f:fp32 f:bf16 h:bf16 h:bf16", 5000: "f:fp32 f:bf16 h:bf16 h:bf16", 12000: "f:fp32 f:bf16 h:bf16 h:bf16"},
    ("bf16_train", "unaligned"): {1000: "o:bf16 h:bf16 h:bf16 h:bf16", 5000: "o:bf16 h:bf16 h:bf16 h:bf16", 12000: "o:bf16 h:bf16 h:bf16 h:bf16"},
    ("bf16_eval", "plain"): {1000: "f:eval_bf16 h:eval_bf16 h:eval_bf16 h:eval_bf16", 5000: "f:eval_bf16 h:eval_bf16 h:eval_bf16 h:eval_bf16",
                             12000: "f:eval_bf16 h:eval_bf16 h:eval_bf16 f:fp32"},
    ("bf16_eval", "unaligned"): {1000: "o:eval f:eval f:eval f:eval", 5000: "o:eval f:eval f:eval f:fp32", 12000: "o:eval f:eval f:eval f:fp32"},
}


def test_block_form_table(lib):
    """functional.block_form for the four model layers (12 -> 32 -> 64 -> 128 -> 256, K = 15, pad = 7; the last one under the
    global average pool) at T = 1000 / 5000 / 12000: default training and evaluation, conv_precision("bf16") training,
    inference_precision("bf16") evaluation, with the BatchNorm of block 2 frozen, an input gradient wanted on block 0, and
    an fp32 input that is not 8-byte aligned.  The table was NOT written from block_form: it is what the predicates that
    block_form replaced gave for these inputs at the commit before it — _bf16_block_ok, eval_bf16.takes / covered, the
    ecg_conv1d_bn_relu_pool[_gap]_eval_supported queries and conv_block_chain's look-ahead, walked along the chain by a
    script (all pure host calls).  The input kind of a block is part of the table: h where the block before it took a bf16
    form AND the look-ahead said this block takes bf16 rows.  The same table pins the packer's walk of the chain
    (_operand_kinds): bf16 operands exactly for the blocks whose form reads them."""
    from ecg_hip import functional as F
    ch = (12, 32, 64, 128, 256)
    kinds = {"o": F._X_OTHER, "f": F._X_F32, "h": F._X_BF16}
    knobs = {"train": ("fp32", "fp32", True), "eval": ("fp32", "fp32", False), "bf16_train": ("bf16", "fp32", True),
             "bf16_eval": ("fp32", "bf16", False)}
    for (setting, variant), per_T in _BLOCK_FORMS.items():
        conv_prec, infer_prec, train = knobs[setting]
        for T, want in per_T.items():
            want, Lin = [w.split(":") for w in want.split()], T
            # ... and the packer's walk of the chain packs what these forms read: bf16 operands where the table says a bf16
            # form, the input-gradient operand where the block owes an input gradient
            geo = tuple(((ch[i + 1], ch[i], 15), 7) for i in range(4))
            packed = F._operand_kinds(geo, kinds[want[0][0]], T, tuple(train and not (variant == "bn2_frozen" and i == 2)
                                                                       for i in range(4)), train, variant == "dx0" and train,
                                      conv_prec, infer_prec)
            assert packed == tuple((f in F._BF16_FORMS, train and (i > 0 or variant == "dx0")) for i, (_, f) in enumerate(want))
            for i, (kind, form) in enumerate(want):
                batch = train and not (variant == "bn2_frozen" and i == 2)
                need_dx = train and (i > 0 or variant == "dx0")
                ask = lambda k: F.block_form(ch[i], ch[i + 1], 15, 7, Lin, i == 3, kinds[k], batch, train, need_dx,   # noqa: E731
                                             conv_prec, infer_prec)
                assert ask(kind) == form, (setting, variant, T, i, ask(kind), form)
                if i:       # the look-ahead of the block before: this block asked with bf16 rows
                    handed = want[i - 1][1] in F._BF16_FORMS and ask("h") in F._BF16_FORMS
                    assert handed == (kind == "h"), (setting, variant, T, i)
                Lin //= 2


def test_bf16_form_stops_where_its_weight_gradient_stops(lib):
    """Every mixed-precision training block's backward calls ecg_conv1d_bwd_weight_bias_bf16_ncl, which refuses input rows
    shorter than ecg_conv1d_bf16_tk_min_len().  block_form asks that query (no literal on the Python side), so a block with
    a shorter row runs the fp32 form, the block before it hands over fp32 rows, and the packer packs fp32 operands for it:
    T = 100 (rows 100 / 50 / 25 / 12) and 127 (.. / 15) end on an fp32 block, T = 128 (.. / 16) is bf16 throughout."""
    from ecg_hip import functional as F
    lo = lib.ecg_conv1d_bf16_tk_min_len()
    assert lo == 16
    # the entry point itself: L = lo - 1 refused with its message before anything else is looked at, L = lo gets further
    args = lambda L_: (None, 128, None, 1, 16, None, None, None, 1, 32, 64, L_, 15, 7, None)      # noqa: E731
    assert lib.ecg_conv1d_bwd_weight_bias_bf16_ncl(*args(lo - 1)) == 1
    assert b"conv1d_bwd_weight_bias_bf16_ncl: N=1 C_in=32 C_out=64 L=15" in lib.ecg_last_error()
    assert lib.ecg_conv1d_bwd_weight_bias_bf16_ncl(*args(lo)) == 1 and b"null pointer" in lib.ecg_last_error()
    ch = (12, 32, 64, 128, 256)
    geo = tuple(((ch[i + 1], ch[i], 15), 7) for i in range(4))
    for T, want in ((100, "bf16 bf16 bf16 fp32"), (127, "bf16 bf16 bf16 fp32"), (128, "bf16 bf16 bf16 bf16"),
                    (31, "bf16 fp32 fp32 fp32"), (15, "fp32 fp32 fp32 fp32")):
        want, Lin, kind = want.split(), T, F._X_F32
        for i, form in enumerate(want):
            assert F.block_form(ch[i], ch[i + 1], 15, 7, Lin, i == 3, kind, True, True, i > 0, "bf16", "fp32") == form, (T, i)
            assert (Lin >= lo) == (form == "bf16")
            # the look-ahead of the block before (this block asked with bf16 rows) says the same, so no bf16 rows reach an
            # fp32 block
            assert not i or F.block_form(ch[i], ch[i + 1], 15, 7, Lin, i == 3, F._X_BF16, True, True, True, "bf16", "fp32") == form
            kind, Lin = F._X_BF16 if form == "bf16" else F._X_F32, Lin // 2
        assert F._operand_kinds(geo, F._X_F32, T, (True,) * 4, True, False, "bf16", "fp32") == \
            tuple((f == "bf16", i > 0) for i, f in enumerate(want))


def test_library_reads_no_environment_and_allocates_nothing():
    """include/ecg_hip.h: "never allocates", "no global mutable state", "reads no environment variable" — checked on the
    dynamic symbol table of the built library (what it would have to import to break the promise)."""
    import subprocess
    from ecg_hip import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    syms = subprocess.run(["nm", "-D", "--undefined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for banned in ("getenv", "secure_getenv", "hipMalloc", "hipFree", "hipMemset", "hipMallocAsync", "hipHostMalloc",
                   "pthread_mutex_lock"):
        assert not any(line.split()[-1].split("@")[0] == banned for line in syms.splitlines() if line.strip()), banned
