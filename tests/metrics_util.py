"""What the metrics tests share (test_metrics_host, test_compare_host, test_operating_host, test_gpu_metrics, test_gpu_compare,
test_gpu_operating): the bit comparison, the tolerance against scikit-learn, the library and the package module, the
header's slab, and the two copies between host and device.  The case tables and generators stay with their tests."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def tol(n):
    return n * 2.0 ** -50


def load_lib():
    """The loaded library, built first if it is not there."""
    import __graft_entry__ as g
    from ecg_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def metrics_module():
    from ecg_hip import metrics
    return metrics


def header_slab():
    text = open(os.path.join(ROOT, "include", "ecg_hip.h")).read()
    return int(re.search(r"#define ECG_METRICS_SLAB (\d+)", text).group(1))


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()
