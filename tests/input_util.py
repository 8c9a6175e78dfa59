"""What the GPU tests of the input step share (test_gpu_input, _recording, _resample, _filter, _wfdb_decode, _quality):
the `hip` fixture (import it by name), host <-> device copies, guard buffers, the test-side window rule and the model the
end-to-end checks score with."""
import numpy as np
import pytest
import torch

GUARD = 4097        # elements of the guard value on either side of a guarded array: an odd element offset


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    import ecg_hip
    from ecg_hip import _lib, functional
    ecg_hip.load()
    _lib.call("ecg_check_device")
    return functional


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def guarded(a, value=12345, guard=GUARD):
    """a (int16 or fp32) on the host -> (the same values on the device, contiguous, in the middle of a buffer of `value`
    with `guard` elements on either side; the buffer).  A read outside the array changes a value and faults nothing."""
    big = torch.full((a.size + 2 * guard,), value, dtype=torch.from_numpy(a).dtype)
    big[guard:guard + a.size] = torch.from_numpy(a.reshape(-1))
    big = big.cuda()
    return big[guard:guard + a.size].view(a.shape), big


def unchanged(c, value=12345, guard=GUARD):
    """c: a case with the guarded buffer under "big" and the host array it was made from under "x" (fp32) or "d" (int16):
    array and guards still hold what they held."""
    big, a = host(c["big"]), c["x"] if "x" in c else c["d"]
    return (np.array_equal(big[guard:-guard], a.reshape(-1)) and (big[:guard] == value).all()
            and (big[-guard:] == value).all())


def plan_on(Ttot, T, hop, first):
    """The window rule with a first start that need not be 0 and tail="shift": -> (first, hop, W, last_start, starts)."""
    wreg = (Ttot - T - first) // hop + 1
    starts = [first + w * hop for w in range(wreg)]
    last = -1
    if (Ttot - T - first) % hop != 0:
        last = Ttot - T
        starts.append(last)
    return first, hop, len(starts), last, tuple(starts)


def _model(name="cnn"):
    from src.models.ecg_cnn import ECGCNN
    from src.models.ecg_multimodal import ECGMultimodal
    from src.utils.seed import set_seed
    set_seed(42)
    return (ECGCNN(num_labels=5) if name == "cnn" else ECGMultimodal()).cuda().eval()


def _score(*a, **kw):
    from ecg_hip.recording import score_recording
    return score_recording(*a, **kw)
