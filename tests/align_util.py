"""Guarded, deliberately misaligned operands for the kernel-level alignment tests (tests/test_gpu_alignment.py).

Every operand of a call sits at a chosen byte offset (0, 4 or 8 modulo 16) inside a larger device buffer with at least
4096 elements of guard on either side (input_util.guarded with guard = 4096 + k):
  * inputs are surrounded by a guard VALUE that the test varies — every case runs twice, once with 12345.0 and once with
    NaN around its inputs, and the two runs' outputs must be equal bit for bit: a read outside an operand changes a result
    and faults nothing;
  * outputs are pre-filled with NaN between guards that hold a fixed bit pattern: afterwards the guards must be unchanged
    bit for bit and no NaN may be left in an output whose inputs were finite (an element the kernel forgot stays NaN);
  * workspaces are NaN-filled too (an element read before it is written poisons a result) but may keep their NaN.

bf16 operands (tests/test_gpu_bf16_contracts.py; the contract is the table of DESIGN.md section 14) are rows [N][C][ld] with a
PAD RULE for the elements [L, ld) of every row:
  * inputs: "zero" — the pad holds zeros in both runs (the kernel may rely on them); "free" — the pad holds this run's
    guard value, a finite one in run 1 and NaN in run 2, like the guards: no bit of any output may depend on it;
  * outputs: "zeroed" — the call must leave +0 there; "untouched" — the call must leave the NaN pre-fill bits there.
Guards stay at >= 4096 ELEMENTS on either side whatever the element size, byte offsets are whatever the contract allows
for the operand (multiples of the element size), and operands that exist only on the device (packed weights) are copied
between guards with put_dev.
"""
import numpy as np
import torch

from input_util import guarded

GUARD = 4096
OUT_PATTERN = 12345.0          # guards of outputs and workspaces: a fixed bit pattern
IN_VALUES = (12345.0, float("nan"))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


BF16_NAN_BITS = torch.tensor(float("nan"), dtype=torch.bfloat16).view(torch.int16).item()     # the pre-fill of bf16 outputs


class Arena:
    """The operands of ONE run of a case."""

    def __init__(self, in_value):
        self.in_value = in_value
        self._ins, self._outs = [], []

    @staticmethod
    def _place(a, off, value):
        assert off in (0, 4, 8) and a.dtype == np.float32
        k = off // 4
        t, big = guarded(np.ascontiguousarray(a), value=value, guard=GUARD + k)
        assert big.data_ptr() % 16 == 0 and t.data_ptr() % 16 == off and t.is_contiguous()
        return t, big, GUARD + k

    def put(self, a, off=0):
        """host fp32 array -> the same values on the device at byte offset `off` (mod 16), guards of this run's value."""
        t, big, g = self._place(a, off, self.in_value)
        self._ins.append((big, _bits(big).clone()))
        return t

    def out(self, shape, off=0, full=True):
        """NaN-filled output of `shape` at byte offset `off`; full: every element must have been written afterwards."""
        a = np.full(shape, np.nan, np.float32)
        t, big, g = self._place(a, off, OUT_PATTERN)
        self._outs.append((t, big, g, full))
        return t

    def scratch(self, n, off=0):
        """Workspace of n floats: guarded like an output, free to keep its NaN."""
        return self.out((max(int(n), 1),), off, full=False)

    # ---- operands of any element size (bf16 rows, packed bf16 weights, int64 counters) ---------------------------------
    def _place_t(self, src, off, value, guard_like=None):
        """host or device tensor `src` -> (view of the same shape at byte offset `off` mod 16 between guards, buffer, guard)"""
        es = src.element_size()
        assert off % es == 0 and 0 <= off < 16
        g = GUARD + off // es
        big = torch.empty(src.numel() + 2 * g + 8, dtype=src.dtype, device="cuda")
        if value is None:
            big.view(torch.int16 if es == 2 else torch.int32 if es == 4 else torch.int64).fill_(guard_like)
        else:
            big.fill_(value)
        t = big[g:g + src.numel()].view(src.shape)
        t.copy_(src)
        assert big.data_ptr() % 16 == 0 and t.data_ptr() % 16 == off and t.is_contiguous()
        return t, big, g

    def put_dev(self, src, off=0):
        """a tensor (host or device, any dtype) -> the same bits at byte offset `off`, guards of this run's value (floating
        types) or of a fixed bit pattern (integers)."""
        if src.is_floating_point():
            t, big, g = self._place_t(src, off, self.in_value)
        else:
            t, big, g = self._place_t(src, off, None, guard_like=0x3039)
        self._ins.append((big, _bits(big).clone()))
        return t

    def put_rows(self, a, ld, pad, off=0):
        """host fp32 [N][C][L] -> bf16 rows [N][C][ld] (values rounded to nearest even) at byte offset `off`; the row pads
        hold zeros (pad == "zero") or this run's guard value (pad == "free")."""
        assert pad in ("zero", "free") and ld >= a.shape[2]
        rows = torch.full(a.shape[:2] + (ld,), 0.0 if pad == "zero" else self.in_value, dtype=torch.bfloat16)
        rows[:, :, :a.shape[2]] = torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16)
        return self.put_dev(rows, off)

    def put_f32_rows(self, a, ld, off=0):
        """host fp32 [N][C][L] -> fp32 rows [N][C][ld] whose pads are free (this run's guard value)."""
        rows = torch.full(a.shape[:2] + (ld,), self.in_value, dtype=torch.float32)
        rows[:, :, :a.shape[2]] = torch.from_numpy(np.ascontiguousarray(a))
        return self.put_dev(rows, off)

    def out_rows(self, shape, L, pad, off=0):
        """NaN-filled bf16 output rows [N][C][ld] at byte offset `off`: afterwards no NaN in [0, L) of any row, and the pads
        [L, ld) hold +0 (pad == "zeroed") or still the pre-fill bits (pad == "untouched")."""
        assert pad in ("zeroed", "untouched") and shape[2] >= L
        t, big, g = self._place_t(torch.full(shape, float("nan"), dtype=torch.bfloat16), off, OUT_PATTERN)
        assert bool(torch.isnan(t).all())
        self._outs.append((t, big, g, (L, pad)))
        return t

    def check(self):
        torch.cuda.synchronize()
        for big, before in self._ins:
            assert torch.equal(_bits(big), before), "a kernel wrote into an input or its guards"
        for t, big, g, full in self._outs:
            b = _bits(big)
            want = _bits(torch.tensor([OUT_PATTERN], dtype=big.dtype))[0].item()
            assert bool((b[:g] == want).all()) and bool((b[g + t.numel():] == want).all()), "a kernel wrote outside an output"
            if isinstance(full, tuple):
                L, pad = full
                assert not bool(torch.isnan(t[..., :L]).any()), "NaN left in an output row whose inputs were finite"
                padbits = _bits(t[..., L:])
                if pad == "zeroed":
                    assert bool((padbits == 0).all()), "an output row pad the contract calls zeroed is not +0"
                else:
                    assert bool((padbits == BF16_NAN_BITS).all()), "an output row pad the contract calls untouched was written"
            elif full:
                assert not bool(torch.isnan(t).any()), "NaN left in an output whose inputs were finite"


def run_guarded(body):
    """body(arena) launches one case on operands it takes from the arena and returns {name: device tensor}.  Runs it with
    both input-guard values, checks guards and outputs after each, asserts the two runs equal bit for bit, and returns the
    first run's outputs on the host."""
    runs = []
    for v in IN_VALUES:
        ar = Arena(v)
        outs = body(ar)
        ar.check()
        runs.append({k: _host(t) for k, t in outs.items() if t is not None})
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert np.array_equal(runs[0][k][0], runs[1][k][0]), \
            f"{k}: the result depends on what lies around the inputs or in their free pads"
    return {k: v[1] for k, v in runs[0].items()}


def _host(t):
    """device tensor -> (its bits, its values as a host array: fp32 for bf16 tensors)"""
    t = t.detach()
    bits = _bits(t).cpu().numpy().copy()
    return bits, (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy().copy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))
