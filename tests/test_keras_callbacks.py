"""EarlyStopping, ModelCheckpoint and ReduceLROnPlateau (tf.keras 2.4 rules, written into their docstrings), the two
evaluation hooks of Callback, and the argument handling of Model.evaluate / fit's validation -- driven through stub
models and hand-written sequences of logs (no GPU)."""
import inspect

import numpy as np
import pytest

from lisec_amd import model_training as mt
from lisec_amd.lr_schedules import CosineDecay

cbs = mt.callbacks


class _Opt:
    def __init__(self, lr):
        self.lr = lr


class _Model:
    """What the callbacks touch: optimizer.lr, stop_training, save(), and the variable snapshot of EarlyStopping."""

    def __init__(self, lr=0.1):
        self.optimizer = _Opt(lr)
        self.stop_training = False
        self.weights = 0
        self.saved = []

    def _snapshot_weights(self):
        return ("snapshot", self.weights)

    def _restore_weights(self, w):
        assert w[0] == "snapshot"
        self.weights = w[1]

    def save(self, path):
        self.saved.append(path)


def _drive(cb, model, values, key="val_loss", extra=None):
    """Runs epochs with logs[key] = values[epoch] until the model is told to stop; model.weights is the epoch number
    (the variables at the end of epoch e are 'e').  Returns the number of epochs run."""
    cb.set_model(model)
    cb.on_train_begin()
    for epoch, v in enumerate(values):
        cb.on_epoch_begin(epoch, {})
        model.weights = epoch
        cb.on_epoch_end(epoch, {key: v, **(extra or {})})
        if model.stop_training:
            cb.on_train_end()
            return epoch + 1
    cb.on_train_end()
    return len(values)


def test_callback_base_class_has_test_hooks():
    cb = cbs.Callback()
    for hook in (cb.on_test_begin, cb.on_test_end):
        hook()
        hook({"loss": 1.0})


def test_early_stopping_patience_and_stopped_epoch():
    m = _Model()
    es = cbs.EarlyStopping(monitor="val_loss", patience=2)
    assert _drive(es, m, [5.0, 4.0, 4.5, 4.2, 3.0]) == 4         # best at epoch 1, then two epochs without improvement
    assert es.stopped_epoch == 3 and m.stop_training and es.best == 4.0
    m = _Model()
    es = cbs.EarlyStopping(patience=0)
    assert _drive(es, m, [5.0, 5.0, 1.0]) == 2                     # an equal value is no improvement
    assert es.stopped_epoch == 1
    m = _Model()
    es = cbs.EarlyStopping(patience=3)
    assert _drive(es, m, [5.0, 4.0, 3.0, 2.0]) == 4 and not m.stop_training and es.stopped_epoch == 0
    m = _Model()                                                   # a reused callback starts afresh (on_train_begin)
    assert _drive(es, m, [1.0, 2.0, 2.0, 2.0]) == 4 and m.stop_training and es.stopped_epoch == 3


def test_early_stopping_min_delta_in_both_modes():
    m = _Model()
    es = cbs.EarlyStopping(min_delta=0.5, patience=1)              # min: an epoch must beat the best by 0.5
    assert es.min_delta == -0.5
    assert _drive(es, m, [5.0, 4.6, 4.0]) == 2 and es.best == 5.0
    m = _Model()
    es = cbs.EarlyStopping(monitor="val_acc", min_delta=-0.5, patience=1)    # auto -> max ('acc'); |min_delta|
    assert es.monitor_op == np.greater and es.min_delta == 0.5
    assert _drive(es, m, [0.1, 0.7, 0.9], key="val_acc") == 3 and es.best == 0.7 and m.stop_training
    m = _Model()
    es = cbs.EarlyStopping(monitor="val_loss", mode="max", min_delta=0.1, patience=1)
    assert _drive(es, m, [1.0, 1.2, 1.25]) == 3 and es.best == 1.2
    with pytest.warns(UserWarning, match="unknown"):
        es = cbs.EarlyStopping(mode="sideways")
    assert es.monitor_op == np.less


def test_early_stopping_baseline_and_restore_best_weights():
    m = _Model()
    es = cbs.EarlyStopping(patience=2, baseline=3.0, restore_best_weights=True)
    assert _drive(es, m, [4.0, 3.5, 3.2]) == 2 and es.stopped_epoch == 1
    assert m.weights == 1                           # no epoch beat the baseline: nothing to restore
    m = _Model()
    es = cbs.EarlyStopping(patience=2, baseline=3.0, restore_best_weights=True)
    assert _drive(es, m, [4.0, 2.0, 2.5, 1.5, 2.2, 2.1, 0.1]) == 6
    assert es.best == 1.5 and es.stopped_epoch == 5
    assert m.weights == 3                           # the variables at the end of the best epoch
    m = _Model()
    es = cbs.EarlyStopping(patience=1)
    assert _drive(es, m, [1.0, 2.0]) == 2 and m.weights == 1


def test_monitor_missing_warns_and_skips():
    m = _Model()
    es = cbs.EarlyStopping(patience=0)
    with pytest.warns(UserWarning, match="not available"):
        assert _drive(es, m, [1.0, 2.0, 3.0], key="loss") == 3
    assert not m.stop_training
    ck = cbs.ModelCheckpoint("x.h5", save_best_only=True)
    with pytest.warns(UserWarning, match="skipping"):
        _drive(ck, m, [1.0], key="loss")
    assert m.saved == []
    r = cbs.ReduceLROnPlateau(patience=0)
    r.set_model(m)
    r.on_train_begin()
    logs = {"loss": 1.0}
    with pytest.warns(UserWarning, match="not available"):
        r.on_epoch_end(0, logs)
    assert logs["lr"] == 0.1 and m.optimizer.lr == 0.1


def test_model_checkpoint_best_only_and_filepath():
    m = _Model()
    ck = cbs.ModelCheckpoint("ck-{epoch:02d}-{val_loss:.2f}.h5", save_best_only=True)
    _drive(ck, m, [3.0, 2.0, 2.0, 2.5, 1.0])        # no min_delta, and an equal value does not save
    assert m.saved == ["ck-01-3.00.h5", "ck-02-2.00.h5", "ck-05-1.00.h5"]
    m = _Model()
    ck = cbs.ModelCheckpoint("ck-{epoch}.h5", monitor="val_acc", save_best_only=True)     # auto -> max
    _drive(ck, m, [0.1, 0.3, 0.2], key="val_acc")
    assert m.saved == ["ck-1.h5", "ck-2.h5"]
    m = _Model()
    ck = cbs.ModelCheckpoint("every-{epoch}-{loss:.1f}.h5")
    _drive(ck, m, [3.0, 4.0], extra={"loss": 0.5})
    assert m.saved == ["every-1-0.5.h5", "every-2-0.5.h5"]


def test_reduce_lr_on_plateau_rate_sequence_with_cooldown_and_min_lr():
    m = _Model(lr=1.0)
    r = cbs.ReduceLROnPlateau(factor=0.5, patience=2, cooldown=2, min_lr=0.2, min_delta=0.0)
    r.set_model(m)
    r.on_train_begin()
    values = [5.0] * 7 + [4.0] * 6
    lrs = []
    for epoch, v in enumerate(values):
        logs = {"val_loss": v}
        r.on_epoch_end(epoch, logs)
        lrs.append(logs["lr"])                      # the rate the epoch ran with
    # epoch 2: plateau -> 0.5, cooldown 2; 3: cooldown; 4: wait 1; 5: -> 0.25; 6: cooldown; 7: improvement (4.0);
    # 8: wait 1; 9: -> max(0.125, 0.2) = 0.2; 10: cooldown; 11: wait 1; 12: wait 2, but lr == min_lr: unchanged
    assert lrs == [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, 0.25, 0.2, 0.2, 0.2]
    assert m.optimizer.lr == 0.2
    m = _Model(lr=1.0)
    r = cbs.ReduceLROnPlateau(factor=0.1, patience=1)           # min_delta 1e-4
    r.set_model(m)
    r.on_train_begin()
    for epoch, v in enumerate([1.0, 0.99995]):                  # not 1e-4 below the best: a plateau
        r.on_epoch_end(epoch, {"val_loss": v})
    assert m.optimizer.lr == pytest.approx(0.1)


def test_callback_argument_refusals():
    with pytest.raises(ValueError, match="factor >= 1.0"):
        cbs.ReduceLROnPlateau(factor=1.0)
    with pytest.raises(NotImplementedError, match="save_weights"):
        cbs.ModelCheckpoint("x.h5", save_weights_only=True)
    with pytest.raises(NotImplementedError, match="save_freq"):
        cbs.ModelCheckpoint("x.h5", save_freq=10)
    r = cbs.ReduceLROnPlateau()
    r.set_model(_Model(lr=CosineDecay(0.1, 100)))
    with pytest.raises(ValueError, match="CosineDecay"):
        r.on_train_begin()


def test_validation_split_takes_the_floored_tail():
    assert mt._validation_split_at(10, 0.2) == 8
    assert mt._validation_split_at(7, 0.3) == 4          # floor(7 * 0.7) = 4: three sweeps validate
    assert mt._validation_split_at(3, 0.5) == 1
    for n, f in ((1, 0.5), (2, 1e-17), (4, 0.0), (4, 1.0), (4, 1.5)):
        with pytest.raises(ValueError):
            mt._validation_split_at(n, f)


def test_validation_freq():
    assert [e for e in range(6) if mt._should_validate(e, 1)] == list(range(6))
    assert [e for e in range(6) if mt._should_validate(e, 2)] == [1, 3, 5]
    assert [e for e in range(6) if mt._should_validate(e, [1, 4])] == [0, 3]
    assert [e for e in range(6) if mt._should_validate(e, {2, 6})] == [1, 5]
    for bad in (0, -1, "2", 1.5, True):
        with pytest.raises(ValueError):
            mt._should_validate(0, bad)


def test_evaluate_and_fit_signatures_and_refusals():
    ev = inspect.signature(mt.Model.evaluate)
    assert list(ev.parameters)[1:] == ["x", "y", "batch_size", "verbose", "sample_weight", "steps", "callbacks",
                                       "return_dict"]
    fit = inspect.signature(mt.Model.fit)
    for name in ("validation_split", "validation_data", "validation_steps", "validation_freq"):
        assert name in fit.parameters
    m = mt.Model.__new__(mt.Model)                  # refusals that come before any device work
    m.optimizer = None
    y = [np.zeros((0, 8, 16, 2)), np.zeros((0, 8, 16, 14))]
    with pytest.raises(RuntimeError, match="compile"):
        m.evaluate([], y)
    m.optimizer = mt.optimizers.SGD()
    with pytest.raises(NotImplementedError, match="sample_weight"):
        m.evaluate([], y, sample_weight=np.ones(0))
