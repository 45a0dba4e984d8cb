"""BatchNormalization recalibration in Model.fit's world, on the small grid of the optimizer tests (createModel(16, 32, 8,
35), five sweeps, optimizers.SWA(SGD, start_averaging=1, average_period=2)): average_weights(update_bn=x) recalibrates
for the averages and leaves without a trace -- under the Python schedule and under the recorded plans, whose launch
count does not move --; AverageModelCheckpoint(update_bn=...) writes the recalibrated statistics and keeps the live
ones; PreciseBatchNorm recalibrates the live model at the epoch's end; a Sequence gives the bits of the list form."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_batch_fit import PARENT_LAUNCHES, _tuning  # noqa: E402
from test_gpu_optimizers import _data  # noqa: E402

pytestmark = pytest.mark.gpu

AVERAGE_LAUNCHES = 1                       # the averaging pass of a wrapper (tests/test_gpu_weight_average_fit.py)
SMALL = (0.5, 0.25, 0.25, 35, 8, 16, 8)


def _bits(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy().view(np.uint32)


def _model():
    from lisec_amd import model_training as mt
    O = mt.optimizers
    m = mt.createModel(16, 32, 8, 35)
    m.compile(optimizer=O.SWA(O.SGD(lr=0.01, decay=1e-3, momentum=0.9), start_averaging=1, average_period=2),
              loss=['mse', 'mse'])
    return m


def _variables(m):
    net = m.net
    return dict(theta=_bits(net.params.theta), state=_bits(net.params.state), average=_bits(net.average),
                iter_dev=np.array(net._iter_dev.cpu().tolist()),
                **{"slot_" + k: _bits(net.slot(k)) for k in m.optimizer.spec().slots})


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _fit(m, x, y, lo, hi, callbacks=None):
    m.fit(x=x[lo:hi], y=[a[lo:hi] for a in y], batch_size=1, verbose=0, epochs=1, shuffle=False, callbacks=callbacks)


@pytest.mark.parametrize("tuning", ["step_plan=0", "", "pipeline_voxels=0"])
def test_average_weights_with_update_bn_leaves_no_trace(tuning):
    """Three updates; inside average_weights(update_bn=x[:3]) theta is the average and the statistics are those a twin
    net GIVEN the average computes by recalibrate_batchnorm; after leaving, theta, the statistics, the slots and the
    average are bit for bit where they were, and two more updates end where the run that never entered ends -- from
    the same recorded plan (no StalePlanError, not recorded again, the parent's launch count plus the averaging pass)."""
    import torch
    from lisec_amd import model_training as mt
    from lisec_amd.network import LisecNet
    from lisec_amd.params import ParamStore
    with _tuning(tuning):
        eager = tuning == "step_plan=0"
        x, y = _data(mt, not eager, n=5)
        never = _model()
        _fit(never, x, y, 0, 3)
        launches_never = None if eager else never._captured[1].launches
        _fit(never, x, y, 3, 5)
        want = _variables(never)
        if not eager:
            never._captured[1].close()

        model = _model()
        net = model.net
        _fit(model, x, y, 0, 3)
        assert (model._captured is None) == eager
        step = None if eager else model._captured[1]
        at3 = _variables(model)
        assert not np.array_equal(at3["theta"], at3["average"])
        generation = mt._lib.alloc_generation()
        with model.average_weights(update_bn=x[:3]) as inside:
            assert inside is model
            assert np.array_equal(_bits(net.params.theta), at3["average"])
            assert np.array_equal(_bits(net.average), at3["theta"])
            state_inside = _bits(net.params.state)
        assert not np.array_equal(state_inside, at3["state"])
        _same(_variables(model), at3)
        assert mt._lib.alloc_generation() == generation                  # no workspace grew: the plan is not stale
        # the restore also happens when the block, or the recalibration itself, raises
        state_pooled = None
        with pytest.raises(KeyError):
            with model.average_weights(update_bn=x[:3], statistics="pooled"):
                state_pooled = _bits(net.params.state)
                raise KeyError("inside")
        assert not np.array_equal(state_pooled, state_inside)
        _same(_variables(model), at3)
        with pytest.raises(ValueError, match="sweep"):
            with model.average_weights(update_bn=[]):
                raise AssertionError("entered")
        _same(_variables(model), at3)
        with pytest.raises(ValueError, match="statistics"):
            with model.average_weights(update_bn=x[:3], statistics="median"):
                raise AssertionError("entered")
        _same(_variables(model), at3)
        _fit(model, x, y, 3, 5)
        _same(_variables(model), want)
        if not eager:
            assert model._captured[1] is step and step.launches == launches_never
            if tuning == "pipeline_voxels=0":
                assert step.launches == PARENT_LAUNCHES + AVERAGE_LAUNCHES
            step.close()
        # the twin, made last (a second net's workspaces make the first one's recorded plans stale): the average as its
        # variables, the statistics the model had when it entered
        p = ParamStore(net.device)
        p.theta.copy_(torch.from_numpy(at3["average"].view(np.float32).copy()))
        p.state.copy_(torch.from_numpy(at3["state"].view(np.float32).copy()))
        p.touch()
        twin = LisecNet(16, 32, 8, 35, params=p)
        twin.recalibrate_batchnorm([s.sample for s in x[:3]])
        assert np.array_equal(_bits(twin.params.state), state_inside)


def test_checkpoint_precise_bn_and_sequence(tmp_path):
    from lisec_amd import augment
    from lisec_amd import model_training as mt
    import augment_cases as C
    x, y = _data(mt, True, n=3)
    path = str(tmp_path / "avg-{epoch}.h5")
    # AverageModelCheckpoint(update_bn=...): the file holds the averages with statistics recalibrated for them; the live
    # model is where the same fit without it ends (a callback in both runs: the same plan key)
    plain, ckpt = _model(), _model()
    _fit(plain, x, y, 0, 3, callbacks=[mt.callbacks.Callback()])
    _fit(ckpt, x, y, 0, 3, callbacks=[mt.callbacks.AverageModelCheckpoint(False, path, update_bn=x, statistics="pooled")])
    live = _variables(ckpt)
    _same(live, _variables(plain))
    with ckpt.average_weights(update_bn=x, statistics="pooled"):
        want_state, want_theta = _bits(ckpt.net.params.state), _bits(ckpt.net.params.theta)
    assert not np.array_equal(want_state, live["state"])
    # PreciseBatchNorm(period=1): the statistics at the epoch's end are those of a direct call
    precise = _model()
    cb = mt.callbacks.PreciseBatchNorm(x, period=1)
    _fit(precise, x, y, 0, 3, callbacks=[cb])
    assert cb.calls == 1                                                 # on_train_end found the epoch's own recalibration
    plain.recalibrate_batch_norm(x, statistics="pooled")
    got = _variables(precise)
    assert np.array_equal(got["state"], _bits(plain.net.params.state)) and not np.array_equal(got["state"], live["state"])
    for k in got:
        if k != "state":
            assert np.array_equal(got[k], live[k]), k
    every_other = mt.callbacks.PreciseBatchNorm(x, period=2, steps=2, statistics="mean")
    _fit(precise, x, y, 0, 3, callbacks=[every_other])
    assert every_other.calls == 1                                        # not at the end of epoch 1: at on_train_end
    for m in (plain, ckpt, precise):
        m._captured[1].close()
    # a Sequence as x: the bits of the list form (its label maps are ignored), `steps` counts from the front
    pts, bxs = C.fit_sweeps()
    seq = augment.AugmentedSweeps(pts, bxs, seed=4, augment=False, balance=False)
    listed = [mt.VFE_preprocessing(p, *SMALL) for p in pts]
    a, b = _model(), _model()
    for kw in (dict(), dict(steps=2, statistics="pooled")):
        a.recalibrate_batch_norm(seq, **kw)
        b.recalibrate_batch_norm(listed, **kw)
        assert np.array_equal(_bits(a.net.params.state), _bits(b.net.params.state))
    two = _bits(b.net.params.state)
    b.recalibrate_batch_norm(listed[:2], statistics="pooled")
    assert np.array_equal(_bits(b.net.params.state), two)
    # load_model of the checkpoint (last: a new model's workspaces)
    loaded = mt.load_model(path.format(epoch=1))
    assert np.array_equal(_bits(loaded.net.params.state), want_state)
    assert np.array_equal(_bits(loaded.net.params.theta), want_theta)
