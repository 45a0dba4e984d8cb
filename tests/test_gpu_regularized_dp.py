"""Weight regularizers under data parallel: two ranks (both on cuda:0, gloo) fit a regularised model.  The penalty's
gradient term is added after the gradient average and is the same on every rank, so the replicas keep identical
variables; every rank's evaluate() returns the same loss, penalty included."""
import math
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))


def _worker(rank, world, port, out_dir):
    import torch
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), LISEC_DIST_BACKEND="gloo", LISEC_BENCH_DEVICE="0")   # both ranks on cuda:0
    sys.path.insert(0, TESTS)
    from lisec_amd import model_training as mt
    from test_gpu_optimizers import _data
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35, kernel_regularizer=mt.regularizers.l1_l2(l1=2e-5, l2=4e-3),
                           gamma_regularizer=mt.regularizers.l2(1e-3))
    assert model.dp is not None and model.dp.world == 2
    model.compile(optimizer=mt.optimizers.Adam(learning_rate=1e-3), loss=['mse', 'mse'])
    x, y = _data(mt, True, n=4)
    hist = model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=4, shuffle=False)
    ev = model.evaluate(x, y, verbose=0)
    torch.cuda.synchronize()
    p, terms = model.net.params, []
    for name, (l1, l2) in model.regularizers.items():
        w = p.view(name).detach().cpu().numpy().astype(np.float64)
        terms += [l1 * np.abs(w).sum(), l2 * (w * w).sum()]
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), theta=p.theta.cpu().numpy(), grad=model.net.grad.cpu().numpy(),
             penalty=model.net.reg_penalty.cpu().numpy(), loss=np.array(hist.history["loss"]), ev=np.array(ev),
             P=np.array(math.fsum(terms)), iterations=np.array(model.net.iterations))
    model.dp.barrier()
    model.dp.close()


def test_two_ranks_keep_identical_variables_and_penalty(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = dict(np.load(tmp_path / "rank0.npz")), dict(np.load(tmp_path / "rank1.npz"))
    assert int(r0["iterations"]) == 2
    for k in ("theta", "grad", "penalty", "ev", "P"):        # the regularised gradient too: averaged, then the same term
        assert np.array_equal(r0[k], r1[k]), k
    # evaluate(): loss = class + regression + P of the variables as they are, on both ranks
    loss, cls, reg = (float(v) for v in r0["ev"][:3])
    P = float(r0["P"])
    print(f"evaluate: loss {loss!r} = {cls + reg!r} + P {P!r}")
    assert P >= cls + reg > 0                                # see test_gpu_regularized_fit: the bound needs P >= L
    assert abs(loss - cls - reg - P) <= 2.0 ** -23 * abs(loss)
    assert abs(float(r0["penalty"][0]) - P) <= 1e-9 * P       # evaluate's penalty-only call left it in reg_penalty
