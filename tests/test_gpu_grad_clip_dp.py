"""global_clipnorm under data parallel, two ranks on one card (after tests/test_gpu_lamb_dp.py): the clipping runs behind
the gradient exchange, on the averaged gradient, so every rank forms the same scale from the same bits and no second
exchange is needed -- and the run is the single-process one at the same global batch: with two ranks at batch_size=1
the exchanged gradient is (g0 + g1) * 0.5, which is what batch_size=2 accumulates in one process, bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
CLIP = 0.05           # far below the norm of these gradients (asserted below): every update clips


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _optimizer(mt):
    return mt.optimizers.clip_gradients(mt.optimizers.Adam(learning_rate=0.01, decay=1e-3), global_clipnorm=CLIP)


def _dump(model, path):
    import torch
    torch.cuda.synchronize()
    net = model.net
    np.savez(path, theta=net.params.theta.cpu().numpy(), m=net.slot("m").cpu().numpy(), v=net.slot("v").cpu().numpy(),
             grad=net.grad.cpu().numpy(), norm=np.array([net.gradient_norms()["global"]], np.float32),
             iterations=np.array(net.iterations), iter_dev=net._iter_dev.cpu().numpy())


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), LISEC_DIST_BACKEND="gloo", LISEC_BENCH_DEVICE="0")   # both ranks on cuda:0
    sys.path.insert(0, TESTS)
    from lisec_amd import model_training as mt
    from test_gpu_optimizers import _data
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    assert model.dp is not None and model.dp.world == 2
    model.compile(optimizer=_optimizer(mt), loss=['mse', 'mse'])
    x, y = _data(mt, True, n=4)
    # rank r trains on sweeps r, r + 2: two updates, each on the mean gradient of sweeps (0, 1), then (2, 3)
    model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, shuffle=False)
    assert model._captured is not None
    _dump(model, os.path.join(out_dir, f"rank{rank}.npz"))
    model.dp.barrier()
    model.dp.close()


def _single_worker(rank, out_dir):
    """One process without data parallel, batch_size=2 over the same four sweeps: batches (0, 1) and (2, 3).  A fresh
    process like the ranks: the summation order of some kernels follows what a process has allocated before."""
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LISEC_DIST_BACKEND", "LISEC_TUNING", "LISEC_FORCE_DP"):
        os.environ.pop(k, None)
    sys.path.insert(0, TESTS)
    from lisec_amd import model_training as mt
    from test_gpu_optimizers import _data
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    assert model.dp is None
    model.compile(optimizer=_optimizer(mt), loss=['mse', 'mse'])
    x, y = _data(mt, True, n=4)
    model.fit(x=x, y=y, batch_size=2, verbose=0, epochs=1, shuffle=False)
    assert model._captured is not None
    _dump(model, os.path.join(out_dir, "single.npz"))
    model._captured[1].close()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_two_ranks_end_identically_and_as_the_single_process_does(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = dict(np.load(tmp_path / "rank0.npz")), dict(np.load(tmp_path / "rank1.npz"))
    assert int(r0["iterations"]) == 2 and r0["iter_dev"].tolist() == [2, 0]
    assert sorted(r0) == ["grad", "iter_dev", "iterations", "m", "norm", "theta", "v"]
    for k in r0:
        assert np.array_equal(_bits(r0[k]), _bits(r1[k])), k
    # the last update clipped: the norm before was above the threshold, the gradient left behind has the threshold's norm
    after = float(np.sqrt(np.sum(r0["grad"].astype(np.float64) ** 2)))
    print("global norm before", float(r0["norm"][0]), "after", after)
    assert np.isfinite(r0["norm"][0]) and r0["norm"][0] > CLIP and abs(after - CLIP) <= 1e-6 * CLIP
    mp.spawn(_single_worker, args=(str(tmp_path),), nprocs=1, join=True)
    one = dict(np.load(tmp_path / "single.npz"))
    for k in one:
        assert np.array_equal(_bits(one[k]), _bits(r0[k])), k
