"""BatchNormalization recalibration under data parallel, two gloo ranks on one card (started as
tests/test_gpu_weight_average_dp.py starts them: fresh child processes): rank r takes sweeps r and r + 2, the fp64 sums
are all-reduced, and both ranks end with the same statistics, bit for bit -- within one float32 ulp of the
single-process result over the same four sweeps, whose sums associate differently ((s0 + s2) + (s1 + s3) against
((s0 + s1) + s2) + s3 in fp64; nothing else differs)."""
import os
import socket
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 240                        # seconds for each set of child processes, far above the few they need


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dump(model, path):
    import torch
    torch.cuda.synchronize()
    np.savez(path, state=model.net.params.state.cpu().numpy(), theta=model.net.params.theta.cpu().numpy())


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), LISEC_DIST_BACKEND="gloo", LISEC_BENCH_DEVICE="0")   # both ranks on cuda:0
    sys.path.insert(0, TESTS)
    from lisec_amd import model_training as mt
    from test_gpu_optimizers import _data
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    assert model.dp is not None and model.dp.world == 2
    x, _ = _data(mt, True, n=4)
    for statistics in ("mean", "pooled"):
        model.recalibrate_batch_norm(x, statistics=statistics)
        _dump(model, os.path.join(out_dir, f"rank{rank}-{statistics}.npz"))
    model.dp.barrier()
    model.dp.close()


def _single_worker(out_dir):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LISEC_DIST_BACKEND", "LISEC_TUNING", "LISEC_FORCE_DP"):
        os.environ.pop(k, None)
    sys.path.insert(0, TESTS)
    from lisec_amd import model_training as mt
    from test_gpu_optimizers import _data
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    assert model.dp is None
    x, _ = _data(mt, True, n=4)
    for statistics in ("mean", "pooled"):
        model.recalibrate_batch_norm(x, statistics=statistics)
        _dump(model, os.path.join(out_dir, f"single-{statistics}.npz"))


def _worker(i, port, out_dir):
    """Children 0 and 1: the two ranks; child 2, beside them: the single process (one start-up time for all three)."""
    if i < 2:
        _dp_worker(i, 2, port, out_dir)
    else:
        _single_worker(out_dir)


def _spawn(fn, args, nprocs):
    """Fresh child processes under a time limit of their own: a set that has not ended by then is killed and fails."""
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + CHILD_TIMEOUT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"{fn.__name__}: the child processes did not end within {CHILD_TIMEOUT} s")


def _ulps(a, b):
    """Distance in float32 steps between same-signed arrays."""
    assert ((a == 0) | (b == 0) | (np.signbit(a) == np.signbit(b))).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_two_ranks_end_with_the_statistics_of_one_process(tmp_path):
    _spawn(_worker, (_free_port(), str(tmp_path)), 3)
    initial = None
    for statistics in ("mean", "pooled"):
        r0, r1 = (dict(np.load(tmp_path / f"rank{r}-{statistics}.npz")) for r in (0, 1))
        one = dict(np.load(tmp_path / f"single-{statistics}.npz"))
        assert np.array_equal(r0["state"].view(np.uint32), r1["state"].view(np.uint32))
        assert np.array_equal(r0["theta"].view(np.uint32), one["theta"].view(np.uint32))
        d = _ulps(r0["state"], one["state"])
        print(f"{statistics}: {int((d > 0).sum())} of {d.size} statistics differ from the single process, by at most "
              f"{int(d.max())} float32 ulp")
        assert d.max() <= 1
        assert np.abs(r0["state"]).max() > 0
        if initial is not None:
            assert not np.array_equal(initial, r0["state"])              # the two rules give other variances
        initial = r0["state"]
