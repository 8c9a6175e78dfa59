"""What the package knows about a parameter: ONE record per parameter object, held by weak reference, with its gradient
sink (a view of an optimizer's flat gradient that the backward kernels write straight into, so that AccumulateGrad adopts
it as `.grad` and neither the per-step gather — a `torch.cat` of ~28 tensors — nor the all-reduce staging is needed) and its
collectives statement, each with the token of the owner that made it.

ONE lookup rule.  The backward wrappers ask by ADDRESS (the `data_ptr()` of the weight they were given), and a record answers
for an address only while its parameter still lives there.  A parameter re-pointed behind the table's back (`p.data = ...`,
`module.to(...)`, `load_state_dict(assign=True)`) has no sink and counts as undeclared — as does whatever now sits at the
address it left — until `parameters_rehomed()` reads the addresses afresh or its owner registers / declares again.

ONE release.  When an owner is collected, a finaliser withdraws what was said under its token (`owner_token`), no more.
"""
import math
import os
import weakref

import torch

_records = {}         # id(parameter) -> _Record
_by_ptr = {}          # parameter address when last read -> _Record (the index the backward pass asks)
_handed = set()       # addresses whose sink went to a kernel in the backward pass that is running now


class _Record:
    __slots__ = ("ref", "ptr", "sink", "sink_owner", "busy", "busy_owner")

    def __init__(self, p):
        self.ref, self.ptr = weakref.ref(p), None
        self.sink = self.sink_owner = self.busy = self.busy_owner = None


def _record(p):
    """The record of parameter `p`, made (or re-made: the id of a dead parameter may be reused) on demand, indexed at the
    address `p` has now."""
    rec = _records.get(id(p))
    if rec is None or rec.ref() is not p:
        rec = _records[id(p)] = _Record(p)
    if _by_ptr.get(rec.ptr) is rec:
        del _by_ptr[rec.ptr]
    rec.ptr = p.data_ptr()
    _by_ptr[rec.ptr] = rec
    return rec


def _lookup(key):
    """(record, parameter) for the parameter that lives at address `key` now, or (None, None)."""
    rec = _by_ptr.get(key)
    if rec is not None:
        p = rec.ref()
        if p is not None and p.data_ptr() == key:
            return rec, p
        del _by_ptr[key]          # the parameter moved away or died: its record stops answering for this address
    return None, None


def parameters_rehomed():
    """Parameter storage moved (flatten_tensors_, or the caller re-pointed parameters itself): read every address afresh.
    Sinks and statements follow the parameter OBJECT; abandoned addresses are undeclared again."""
    _by_ptr.clear()
    for k, rec in list(_records.items()):
        p = rec.ref()
        if p is None or (rec.sink is None and rec.busy is None):      # dead, or everything said about it was withdrawn
            del _records[k]
        else:
            rec.ptr = p.data_ptr()
            _by_ptr[rec.ptr] = rec


def owner_token(owner):
    """The token under which `owner` registers sinks and declares collectives; everything said under it is withdrawn
    when `owner` is collected."""
    token = (type(owner).__name__, id(owner))
    weakref.finalize(owner, release, token)
    return token


def release(owner):
    """Withdraw the sinks and the statements made under the token `owner`, and nothing else."""
    unregister_grad_sinks(owner)
    declare_backward_collectives(list(_records), None, owner)
    parameters_rehomed()


# --------------------------------------------------------------------------------------
# Gradient sinks.  A sink is only handed out while the parameter's `.grad` is None (zero_grad(set_to_none=True), the
# default): if a gradient is already there, autograd will ADD the new one to it, and the kernel must not have overwritten
# the accumulated value.
# --------------------------------------------------------------------------------------
def register_grad_sinks(params, views, owner=None):
    """`views[i]` (a flat view of params[i].numel() floats) becomes the gradient destination of params[i]; a later
    registration for the same parameter replaces an earlier one."""
    for p, v in zip(params, views):
        rec = _record(p)
        rec.sink, rec.sink_owner = v, owner


def unregister_grad_sinks(owner):
    """Withdraw every sink registered under the token `owner`."""
    for rec in _records.values():
        if rec.sink is not None and rec.sink_owner == owner:
            rec.sink = rec.sink_owner = None


def forget_handed_sinks():
    """A new backward pass or a new step begins: every sink may be handed out again.  The autograd engine calls this when
    a pass ends, but runs no callbacks for a pass that RAISED — so backward_from_loss and the optimizers' zero_grad /
    step call it too: one failed backward must not disable the sinks for good."""
    _handed.clear()


def grad_out(key, ref, *shape):
    """Destination of the gradient of the parameter at address `key`: a FRESH view of its sink (AccumulateGrad only adopts
    a tensor nobody else holds) or a new tensor.  A sink is handed out AT MOST ONCE per backward pass: a
    parameter used twice in one graph (model called twice before backward(), shared weights) gets a private
    tensor for its second gradient, which autograd then adds to the first — two kernels writing the same
    sink would leave 2*dw2 instead of dw1 + dw2."""
    if key is not None and key not in _handed:
        rec, p = _lookup(key)
        v = None if rec is None else rec.sink
        if v is not None and p.grad is None and v.device == ref.device and v.numel() == math.prod(shape):
            try:
                if not _handed:
                    torch.autograd.Variable._execution_engine.queue_callback(forget_handed_sinks)
                _handed.add(key)
            except RuntimeError:         # not inside a backward pass (direct call of a backward formula): no tracking
                return torch.empty(shape, dtype=torch.float32, device=ref.device)
            return v.view(shape)
    return torch.empty(shape, dtype=torch.float32, device=ref.device)


# --------------------------------------------------------------------------------------
# The one-launch BatchNorm backward (csrc/bn_relu_pool.hip, bn_bwd_resident_kernel) and collectives.
# Its workgroups exchange partial sums through a bounded wait, which is only instant while every workgroup of the grid
# is resident.  A communication kernel that runs DURING backward and waits for a late peer keeps its CUs; this kernel's
# workgroups would then run out their wait and take the slow self-service path on every call.  The decision is taken
# PER CALL, from what is known about the parameters of the block whose backward is running — no process-wide switch:
#   * the owner of the parameters (FlatAdamW, FlatGradDDP) declares "busy" (its hooks issue all-reduces under backward)
#     or "quiet" (its exchange starts after the last backward kernel);
#   * parameters nobody has declared are quiet in a single-rank process and BUSY as soon as torch.distributed runs more
#     than one rank — so a model wrapped in stock torch.nn.parallel.DistributedDataParallel (bucketed all-reduces under
#     backward, invisible from here) gets the two-pass form without having to ask for it.
# ECG_BN_BWD_RESIDENT=0 keeps the two-pass form everywhere; ECG_HIP_REHEARSE_ON_ONE_GPU=1 (several ranks sharing ONE
# device: workgroups of different processes would wait for each other's CUs) does the same.  Read here, on the host side
# of the ABI: the library reads no environment.
# --------------------------------------------------------------------------------------
_bn_one_launch = (os.environ.get("ECG_BN_BWD_RESIDENT", "1") != "0"
                  and os.environ.get("ECG_HIP_REHEARSE_ON_ONE_GPU") != "1")
_bn_spin_polls = int(os.environ.get("ECG_BN_BWD_RESIDENT_SPIN", "-1"))     # tests: 0 = nobody waits (self-service path)


def set_bn_backward_one_launch(on, spin_polls=None):
    """Process default for the one-launch BatchNorm backward (True unless the environment says otherwise); returns the
    previous setting.  `spin_polls` (tests) bounds the inter-workgroup wait: 0 forces the self-service path."""
    global _bn_one_launch, _bn_spin_polls
    prev, _bn_one_launch = _bn_one_launch, bool(on)
    if spin_polls is not None:
        _bn_spin_polls = int(spin_polls)
    return prev


def declare_backward_collectives(params, busy, owner=None):
    """The owner of `params` says whether collectives can run on the device while their backward kernels do (True: the
    BatchNorm backward of their blocks keeps the two-pass form), that they cannot (False), or withdraws its statement
    (None; with an `owner` token only a statement made under the same token is withdrawn, so an optimizer going away
    does not take a live wrapper's statement with it).  `params` are the parameter tensors themselves (or their id()s,
    for a withdrawal).  Cheap; call it whenever the exchange mode changes."""
    for p in params:
        if busy is None:
            rec = _records.get(p if isinstance(p, int) else id(p))
            if rec is not None and (owner is None or rec.busy_owner == owner):
                rec.busy = rec.busy_owner = None
        elif not isinstance(p, int):
            rec = _record(p)
            rec.busy, rec.busy_owner = bool(busy), owner


def _multi_rank():
    d = torch.distributed
    return d.is_available() and d.is_initialized() and d.get_world_size() > 1


def bn_backward_one_launch_allowed(key):
    """The per-call decision described above for the block whose conv weight has data_ptr `key`."""
    if not _bn_one_launch:
        return False
    rec, _p = _lookup(key)
    busy = None if rec is None else rec.busy
    return (not _multi_rank()) if busy is None else (not busy)
