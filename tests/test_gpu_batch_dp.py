"""fit(batch_size=B) under data parallel, at most two ranks on one card: each rank forms its batches from its own shard
and the gradient exchange runs once per update, on the accumulated mean.  One forced rank (LISEC_FORCE_DP=1: the
exchange through lisec_allreduce_grads on a communicator of one) leaves the bits of the run without data parallel; two
ranks (gloo) leave the fp64 mean of the per-sweep gradients of the global batch within (B + world + 1) * 2^-24 * mean|g_i|
per element: B - 1 adds and one multiply on a rank, the reduction over the ranks and its scale."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
U = 2.0 ** -24


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


# ---- one forced rank ----------------------------------------------------------------------------------------------------------
def _forced_worker(out):
    """Two fits of B = 2 over four sweeps (two updates) from the same weights and the recorded plans: without data
    parallel, then with a DataParallel of one rank whose exchange is forced."""
    import torch
    sys.path[:0] = [ROOT, TESTS]
    from lisec_amd import model_training as mt
    from lisec_amd.parallel import DataParallel
    from test_gpu_optimizers import _data, _make_opt
    runs = {}
    weights = None
    for tag in ("plain", "forced"):
        np.random.seed(0)
        model = mt.createModel(16, 32, 8, 35)
        if weights is None:
            weights = model._snapshot_weights()
        model._restore_weights(weights)
        if tag == "forced":
            model.dp = DataParallel(model.net.device)
            assert model.dp.world == 1 and model.dp.bucketed().active
        model.compile(optimizer=_make_opt("momentum"), loss=['mse', 'mse'])
        x, y = _data(mt, True, n=4)
        hist = model.fit(x=x, y=y, batch_size=2, verbose=0, epochs=1, shuffle=False)
        torch.cuda.synchronize()
        assert model._captured is not None and model.net.iterations == 2
        net = model.net
        runs[tag] = dict(theta=net.params.theta.cpu().numpy(), state=net.params.state.cpu().numpy(),
                         grad=net.grad.cpu().numpy(), velocity=net.slot("velocity").cpu().numpy(),
                         loss=np.array(hist.history["loss"]), iter_dev=net._iter_dev.cpu().numpy())
        if tag == "forced":
            model._captured[1].close()
            model.dp.close()
    np.savez(out, **{f"{tag}_{k}": v for tag, r in runs.items() for k, v in r.items()})


def test_one_forced_rank_is_bit_identical_to_no_data_parallel(tmp_path):
    out = str(tmp_path / "forced.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LISEC_DIST_BACKEND",
                                                            "LISEC_TUNING")}
    env.update(LISEC_FORCE_DP="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "forced", out], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    d = dict(np.load(out))
    keys = sorted(k[len("plain_"):] for k in d if k.startswith("plain_"))
    assert keys == ["grad", "iter_dev", "loss", "state", "theta", "velocity"]
    for k in keys:
        assert np.array_equal(d["plain_" + k], d["forced_" + k]), k
    assert d["forced_iter_dev"].tolist() == [2, 0] and np.abs(d["forced_velocity"]).max() > 0


# ---- two ranks ----------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_dir, B):
    import torch
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), LISEC_DIST_BACKEND="gloo", LISEC_BENCH_DEVICE="0")   # both ranks on cuda:0
    sys.path.insert(0, TESTS)
    from lisec_amd import model_training as mt
    from test_gpu_optimizers import _data, _make_opt
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    assert model.dp is not None and model.dp.world == 2
    model.compile(optimizer=_make_opt("sgd"), loss=['mse', 'mse'])
    net, dev = model.net, model.net.device
    if rank == 0:
        # the eight per-sweep gradients at the starting variables, eagerly, on one rank first (on the sweeps padded as the
        # recorded step pads them); the moving statistics these forwards move are put back
        weights = model._snapshot_weights()
        xp, yp = _data(mt, False, n=8)
        grads = []
        for i in range(8):
            yc, yr = (torch.from_numpy(a[i]).to(dev) for a in yp)
            net.forward(xp[i].sample, training=True)
            net.backward(yc, yr, loss=model.loss)
            torch.cuda.synchronize()
            grads.append(net.grad.cpu().numpy().copy())
        np.save(os.path.join(out_dir, "sweep_grads.npy"), np.stack(grads))
        model._restore_weights(weights)
    model.dp.barrier()
    x, y = _data(mt, True, n=8)
    model.fit(x=x, y=y, batch_size=B, verbose=0, epochs=1, steps_per_epoch=2, shuffle=False)   # 2 // world: one update
    torch.cuda.synchronize()
    assert model._captured is not None
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), grad=net.grad.cpu().numpy(), theta=net.params.theta.cpu().numpy(),
             iterations=np.array(net.iterations), iter_dev=net._iter_dev.cpu().numpy())
    model.dp.barrier()
    model.dp.close()


@pytest.mark.parametrize("B", [2, 4])
def test_two_ranks_average_the_global_batch(tmp_path, B):
    """Eight sweeps, two ranks (rank r holds sweeps r, r + 2, ...), one update of B sweeps per rank: with B = 4 the update
    is made with all eight sweeps, with B = 2 with the first two of each shard (sweeps 0 .. 3).  Both are run: two ranks at
    B = 2 take four sweeps per update, and a mean over all eight in one update needs B = 4; the bound is the same formula."""
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), B), nprocs=world, join=True)
    r0, r1 = dict(np.load(tmp_path / "rank0.npz")), dict(np.load(tmp_path / "rank1.npz"))
    assert int(r0["iterations"]) == int(r1["iterations"]) == 1 and r0["iter_dev"].tolist() == [1, 0]
    assert np.array_equal(r0["grad"], r1["grad"]) and np.array_equal(r0["theta"], r1["theta"])
    g = np.load(tmp_path / "sweep_grads.npy").astype(np.float64)[:B * world]
    assert g.shape[0] == B * world and np.abs(g).max() > 0
    want, scale = g.mean(0), np.abs(g).mean(0)
    err = np.abs(r0["grad"].astype(np.float64) - want)
    bound = (B + world + 1) * U * scale
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"B = {B}, world = {world}: worst error / bound = {worst:.3f} over {int((scale > 0).sum())} elements with a gradient")
    assert np.all(err <= bound)
    # half the batch would not pass: the mean of rank 0's sweeps alone misses by far more than the bound somewhere
    own = g[0::world].mean(0)
    assert np.any(np.abs(own - want) > 100 * bound)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "forced":
    _forced_worker(sys.argv[2])
