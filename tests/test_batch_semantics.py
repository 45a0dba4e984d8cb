"""fit(batch_size=B) without a GPU: the C ABI of lisec_grad_accumulate as the header declares it and as ctypes binds
it, the refusal of a malformed batch_size before anything else happens, the batch-index arithmetic of an epoch and the
batch-size-weighted epoch mean with a weight penalty, against hand computations."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_abi_and_ctypes_signature_of_grad_accumulate():
    from lisec_amd import _lib
    header = open(os.path.join(ROOT, "include", "lisec_hip.h")).read()
    m = re.search(r"int\s+lisec_grad_accumulate\s*\(([^;]*)\)\s*;", header)
    assert m, "lisec_grad_accumulate is not declared in include/lisec_hip.h"
    args = [re.sub(r"/\*.*?\*/", "", a, flags=re.S).strip() for a in m.group(1).split(",")]
    assert [re.sub(r"\s+\w+$", "", a) for a in args] == ["float*", "float*", "long long", "int", "const float*",
                                                         "lisec_stream_t"]
    for name, value in (("LISEC_ACC_BEGIN", 0), ("LISEC_ACC_ADD", 1), ("LISEC_ACC_END", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", header), name
    assert (_lib.ACC_BEGIN, _lib.ACC_ADD, _lib.ACC_END) == (0, 1, 2)
    # the contract a test pins bit for bit is stated where the entry is declared
    doc = header[header.rfind("/*", 0, m.start()):m.start()]
    assert "contract" in doc.lower() and "never" in doc and "multiply" in doc
    lib = _lib.load()                                   # built by build(); loading it needs no GPU
    fn = lib.lisec_grad_accumulate
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
                                 ctypes.c_void_p]
    # argument checks come before any launch: they answer on a machine without a GPU too
    buf = (ctypes.c_float * 16)()
    base = ctypes.addressof(buf)
    assert fn(None, None, 4, 0, None, None) != 0
    assert fn(base, base, 4, 0, None, None) != 0        # one buffer for both


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "2", None])
def test_fit_refuses_a_malformed_batch_size_before_anything_else(bad):
    from lisec_amd import model_training as mt
    # a Model that was never constructed: the first attribute fit() touched would raise AttributeError, so the ValueError
    # shows that the check comes before the model, the data and the GPU
    with pytest.raises(ValueError, match="batch_size"):
        mt.Model.fit(object.__new__(mt.Model), None, batch_size=bad)
    with pytest.raises(ValueError, match="batch_size"):
        mt._check_batch_size(bad)


def test_batch_size_accepts_integers():
    from lisec_amd import model_training as mt
    assert mt._check_batch_size(1) == 1 and mt._check_batch_size(np.int64(4)) == 4
    assert type(mt._check_batch_size(np.int32(3))) is int


def test_epoch_batches_without_steps_per_epoch():
    from lisec_amd import model_training as mt
    assert mt._epoch_batches(5, 2) == [[0, 1], [2, 3], [4]]
    assert [len(b) for b in mt._epoch_batches(5, 2)] == [2, 2, 1]
    assert mt._epoch_batches(4, 2) == [[0, 1], [2, 3]]
    assert mt._epoch_batches(3, 8) == [[0, 1, 2]]
    assert mt._epoch_batches(3, 1) == [[0], [1], [2]]
    assert mt._epoch_batches(0, 2) == []


def test_epoch_batches_with_steps_per_epoch_wrap_around():
    from lisec_amd import model_training as mt
    got = mt._epoch_batches(3, 2, 4)
    assert got == [[(k * 2 + j) % 3 for j in range(2)] for k in range(4)] == [[0, 1], [2, 0], [1, 2], [0, 1]]
    # batch 1 is the loop the step always was: step st trains on order[st % n]
    assert mt._epoch_batches(3, 1, 5) == [[0], [1], [2], [0], [1]]


def test_batch_positions():
    from lisec_amd.network import LisecNet
    assert LisecNet.batch_positions(1) == ["single"]
    assert LisecNet.batch_positions(2) == ["first", "last"]
    assert LisecNet.batch_positions(4) == ["first", "middle", "middle", "last"]


def test_epoch_mean_with_a_penalty_and_a_short_last_batch():
    """n = 5, B = 2: batches of 2, 2, 1 sweeps.  A batch's loss is the mean of its sweeps' losses plus P once and weighs
    its size: epoch loss = (sum of the sweep losses + 2*P0 + 2*P1 + 1*P2) / 5; the per-output losses carry no penalty."""
    from lisec_amd import model_training as mt
    from lisec_amd.network import LisecNet
    cls = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    reg = np.array([0.5, 0.25, 0.125, 1.0, 2.0])
    P = [10.0, 20.0, 40.0]
    tot = np.zeros(3)
    t = 0
    for k, batch in enumerate(mt._epoch_batches(5, 2)):
        b = len(batch)
        for position in LisecNet.batch_positions(b):
            last = position in ("single", "last")
            # what a step leaves in loss_out: the penalty folded into the total by the step that ends a batch, alone
            loss_out = np.array([cls[t] + reg[t] + (P[k] if last else 0.0), cls[t], reg[t]])
            mt._add_sweep_logs(tot, loss_out, b, last, penalty=np.array([P[k]]))
            t += 1
    assert t == 5
    by_hand = (31.0 + 3.875 + 2 * 10.0 + 2 * 20.0 + 1 * 40.0) / 5
    assert tot[0] / 5 == by_hand == 26.975
    assert tot[1] / 5 == 31.0 / 5 and tot[2] / 5 == 3.875 / 5
    # the same as Keras' mean of the batch losses weighted by batch size
    batch_loss = [(1.5 + 2.25) / 2 + 10.0, (4.125 + 9.0) / 2 + 20.0, 18.0 + 40.0]
    assert abs(tot[0] / 5 - (2 * batch_loss[0] + 2 * batch_loss[1] + 1 * batch_loss[2]) / 5) < 1e-12
    # without regularizers nothing is added
    tot2 = mt._add_sweep_logs(np.zeros(3), np.array([3.0, 1.0, 2.0]), 2, True, penalty=None)
    assert tot2.tolist() == [3.0, 1.0, 2.0]
