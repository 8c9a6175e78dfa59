"""Guarded, deliberately misaligned operands for the kernel-level alignment tests (tests/test_gpu_alignment.py).

Every operand of a call sits at a chosen byte offset (0, 4 or 8 modulo 16) inside a larger device buffer with at least
4096 elements of guard on either side (input_util.guarded with guard = 4096 + k):
  * inputs are surrounded by a guard VALUE that the test varies — every case runs twice, once with 12345.0 and once with
    NaN around its inputs, and the two runs' outputs must be equal bit for bit: a read outside an operand changes a result
    and faults nothing;
  * outputs are pre-filled with NaN between guards that hold a fixed bit pattern: afterwards the guards must be unchanged
    bit for bit and no NaN may be left in an output whose inputs were finite (an element the kernel forgot stays NaN);
  * workspaces are NaN-filled too (an element read before it is written poisons a result) but may keep their NaN.
"""
import numpy as np
import torch

from input_util import guarded

GUARD = 4096
OUT_PATTERN = 12345.0          # guards of outputs and workspaces: a fixed bit pattern
IN_VALUES = (12345.0, float("nan"))


def _bits(t):
    return t.contiguous().view(torch.int32)


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

    def check(self):
        torch.cuda.synchronize()
        for big, before in self._ins:
            assert torch.equal(_bits(big), before), "a kernel wrote into an input or its guards"
        want = torch.tensor(OUT_PATTERN).view(torch.int32).item()
        for t, big, g, full in self._outs:
            b = _bits(big)
            assert bool((b[:g] == want).all()) and bool((b[g + t.numel():] == want).all()), "a kernel wrote outside an output"
            if full:
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
        runs.append({k: t.detach().cpu().numpy().copy() for k, t in outs.items() if t is not None})
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert np.array_equal(runs[0][k].view(np.int32), runs[1][k].view(np.int32)), \
            f"{k}: the result depends on what lies around the inputs"
    return runs[0]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))
