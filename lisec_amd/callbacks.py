"""tf.keras 2.4 callbacks for Model.fit(callbacks=...) and Model.evaluate(callbacks=...), exposed as
lisec_amd.model_training.callbacks: the Callback base class (set_model, set_params, on_train_begin / on_train_end,
on_epoch_begin / on_epoch_end, on_test_begin / on_test_end), LearningRateScheduler, EarlyStopping, ModelCheckpoint and
ReduceLROnPlateau; DetectionEvaluation (ours), which logs the detection metric for them to monitor; and PreciseBatchNorm
(ours), which re-estimates the BatchNormalization moving statistics between epochs.  A learning rate set between epochs reaches the update kernels through the device descriptor of
LisecNet, written on the stream of the step: the recorded step plan is not recorded again.  There are no per-batch hooks:
the fit loop reads nothing back from the device inside an epoch."""
import warnings

import numpy as np

from .lr_schedules import LearningRateSchedule


class Callback:
    """Base class; Model.fit calls set_model and set_params before training, then the four hooks."""

    def __init__(self):
        self.model = None
        self.params = {}

    def set_model(self, model):
        self.model = model

    def set_params(self, params):
        self.params = params

    def on_train_begin(self, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass

    def on_test_begin(self, logs=None):
        """Called by Model.evaluate, and by the validation inside Model.fit, before the first evaluated sweep."""
        pass

    def on_test_end(self, logs=None):
        """Called with the evaluation's logs (loss, ClassificationLayer_loss, RegressionLayer_loss) after it."""
        pass


def _monitor_op(mode, monitor, name):
    """Keras' choice of comparison: 'min' -> np.less, 'max' -> np.greater, 'auto' -> np.greater if 'acc' is in the
    monitored name, np.less otherwise.  An unknown mode warns and falls back to 'auto'."""
    if mode not in ("auto", "min", "max"):
        warnings.warn(f"{name} mode {mode} is unknown, fallback to auto mode.")
        mode = "auto"
    if mode == "min" or (mode == "auto" and "acc" not in monitor):
        return np.less
    return np.greater


def _lr_number(optimizer, name):
    """optimizer.lr as a float; a LearningRateSchedule is refused (the callback would overwrite it)."""
    if not hasattr(optimizer, "lr"):
        raise ValueError('Optimizer must have a "lr" attribute.')
    if isinstance(optimizer.lr, LearningRateSchedule):
        raise ValueError(f"{name} sets optimizer.lr, which is a {type(optimizer.lr).__name__} schedule here: give the "
                         f"optimizer a number, or keep the schedule without this callback")
    return float(optimizer.lr)


def _statistics(statistics):
    """'mean' or 'pooled', the rules of a BatchNormalization recalibration (ops.bn_statistics, restated: this module
    imports nothing that needs the device library); anything else is a ValueError."""
    if statistics not in ("mean", "pooled"):
        raise ValueError(f"statistics must be 'mean' or 'pooled', not {statistics!r}")
    return statistics


class EarlyStopping(Callback):
    """Stops training when the monitored value has stopped improving (tf.keras 2.4 rules):

    - mode 'min' / 'max' / 'auto' ('auto': max if 'acc' is in `monitor`, else min); min_delta is taken as |min_delta|,
      negated in min mode: an epoch improves when monitor_op(current - min_delta, best).
    - on_train_begin resets wait = 0, stopped_epoch = 0 and best = baseline when given (the value to beat), else +inf
      (min) / -inf (max).
    - on_epoch_end: an improvement sets best = current, wait = 0 and, with restore_best_weights, snapshots the
      variables; otherwise wait += 1 and at wait >= patience: stopped_epoch = epoch, model.stop_training = True and, with
      restore_best_weights, the snapshot is put back -- theta and the BatchNormalization moving statistics (Keras'
      get_weights / set_weights), not the optimizer slots.  No snapshot (no epoch beat the baseline): nothing is restored.
    - a monitored key missing from the logs warns and skips the epoch.
    The model's variables are snapshotted by model._snapshot_weights() and put back by model._restore_weights(w)."""

    def __init__(self, monitor="val_loss", min_delta=0, patience=0, verbose=0, mode="auto", baseline=None,
                 restore_best_weights=False):
        super().__init__()
        self.monitor, self.patience, self.verbose, self.baseline = monitor, patience, verbose, baseline
        self.min_delta = abs(min_delta)
        self.wait, self.stopped_epoch = 0, 0
        self.restore_best_weights, self.best_weights = restore_best_weights, None
        self.monitor_op = _monitor_op(mode, monitor, "EarlyStopping")
        self.min_delta *= 1 if self.monitor_op == np.greater else -1

    def on_train_begin(self, logs=None):
        self.wait, self.stopped_epoch = 0, 0
        if self.baseline is not None:
            self.best = self.baseline
        else:
            self.best = np.inf if self.monitor_op == np.less else -np.inf
        self.best_weights = None

    def on_epoch_end(self, epoch, logs=None):
        current = self.get_monitor_value(logs)
        if current is None:
            return
        if self.monitor_op(current - self.min_delta, self.best):
            self.best = current
            self.wait = 0
            if self.restore_best_weights:
                self.best_weights = self.model._snapshot_weights()
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self.stopped_epoch = epoch
                self.model.stop_training = True
                if self.restore_best_weights and self.best_weights is not None:
                    if self.verbose > 0:
                        print("Restoring model weights from the end of the best epoch.")
                    self.model._restore_weights(self.best_weights)

    def on_train_end(self, logs=None):
        if self.stopped_epoch > 0 and self.verbose > 0:
            print(f"Epoch {self.stopped_epoch + 1:05d}: early stopping")

    def get_monitor_value(self, logs):
        logs = logs or {}
        value = logs.get(self.monitor)
        if value is None:
            warnings.warn(f"Early stopping conditioned on metric `{self.monitor}` which is not available. "
                          f"Available metrics are: {','.join(logs.keys())}")
        return value


class ModelCheckpoint(Callback):
    """Saves the model (model.save) at the end of every epoch (tf.keras 2.4 rules):

    - the path is filepath.format(epoch=epoch + 1, **logs), e.g. 'ck-{epoch:02d}-{val_loss:.4f}.h5'.
    - save_best_only: saves only when monitor_op(current, best) -- no min_delta -- with best starting at +inf (min) /
      -inf (max) when the callback is made; mode as EarlyStopping ('auto': max if 'acc' is in `monitor`, else min).  A
      monitored key missing from the logs warns and skips the save.
    - data parallel: every rank calls model.save (identical logs on every rank), which writes from rank 0 behind a
      barrier.
    save_weights_only=True and a save_freq other than 'epoch' raise NotImplementedError."""

    def __init__(self, filepath, monitor="val_loss", verbose=0, save_best_only=False, save_weights_only=False,
                 mode="auto", save_freq="epoch", options=None, **kwargs):
        super().__init__()
        if save_weights_only:
            raise NotImplementedError("ModelCheckpoint(save_weights_only=True): save_weights is not implemented; "
                                      "model.save writes the whole model")
        if save_freq != "epoch":
            raise NotImplementedError(f"ModelCheckpoint(save_freq={save_freq!r}): only save_freq='epoch' is implemented "
                                      f"(there are no per-batch hooks)")
        if kwargs:
            raise TypeError(f"ModelCheckpoint: unexpected keyword argument(s) {', '.join(sorted(kwargs))}")
        self.filepath, self.monitor, self.verbose, self.save_best_only = str(filepath), monitor, verbose, save_best_only
        self.monitor_op = _monitor_op(mode, monitor, "ModelCheckpoint")
        self.best = np.inf if self.monitor_op == np.less else -np.inf

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        filepath = self.filepath.format(epoch=epoch + 1, **logs)
        if self.save_best_only:
            current = logs.get(self.monitor)
            if current is None:
                warnings.warn(f"Can save best model only with {self.monitor} available, skipping.")
                return
            if not self.monitor_op(current, self.best):
                if self.verbose > 0:
                    print(f"\nEpoch {epoch + 1:05d}: {self.monitor} did not improve from {self.best:0.5f}")
                return
            if self.verbose > 0:
                print(f"\nEpoch {epoch + 1:05d}: {self.monitor} improved from {self.best:0.5f} to {current:0.5f}, "
                      f"saving model to {filepath}")
            self.best = current
        elif self.verbose > 0:
            print(f"\nEpoch {epoch + 1:05d}: saving model to {filepath}")
        self._save(filepath)

    def _save(self, filepath):
        self.model.save(filepath)


class AverageModelCheckpoint(ModelCheckpoint):
    """tfa.callbacks.AverageModelCheckpoint: a ModelCheckpoint, with its keywords and rules, for a model compiled with
    optimizers.MovingAverage or optimizers.SWA (anything else: ValueError when training begins).
    update_weights=False: the file is written inside Model.average_weights() -- its model weights are the averages, its
    `average` slot the live weights of that moment -- and training goes on with the live weights, bit for bit as without
    the callback.  update_weights=True: optimizer.assign_average_vars(model) first -- training goes on FROM the averages --
    then the file is written, model weights and average both the averages.
    update_bn=x (ours; what Model.recalibrate_batch_norm takes, `statistics` its rule): the BatchNormalization moving
    statistics in the file are recalibrated for the averages over x (Model.average_weights(update_bn=x)) and the live
    model's are left as they were, bit for bit.  With update_weights=True -- where the averages BECOME the live model --
    the live statistics are recalibrated for them and kept.  An unknown `statistics` is a ValueError here."""

    def __init__(self, update_weights, filepath, monitor="val_loss", verbose=0, save_best_only=False,
                 save_weights_only=False, mode="auto", save_freq="epoch", update_bn=None, statistics="mean", **kwargs):
        super().__init__(filepath, monitor=monitor, verbose=verbose, save_best_only=save_best_only,
                         save_weights_only=save_weights_only, mode=mode, save_freq=save_freq, **kwargs)
        self.update_weights = bool(update_weights)
        self.update_bn, self.statistics = update_bn, _statistics(statistics)

    def on_train_begin(self, logs=None):
        if not hasattr(self.model.optimizer, "assign_average_vars"):
            raise ValueError("AverageModelCheckpoint is only used when training with MovingAverage or SWA")
        super().on_train_begin(logs)

    def _save(self, filepath):
        if self.update_weights:
            self.model.optimizer.assign_average_vars(self.model)
            if self.update_bn is not None:
                self.model.recalibrate_batch_norm(self.update_bn, statistics=self.statistics)
            self.model.save(filepath)
        elif self.update_bn is not None:
            with self.model.average_weights(update_bn=self.update_bn, statistics=self.statistics):
                self.model.save(filepath)
        else:
            with self.model.average_weights():
                self.model.save(filepath)


class ReduceLROnPlateau(Callback):
    """Multiplies the learning rate by `factor` when the monitored value has stopped improving (tf.keras 2.4 rules):

    - factor >= 1 raises ValueError.  mode 'min' (or 'auto' without 'acc' in `monitor`): improvement is
      current < best - min_delta, best starting at +inf; 'max': current > best + min_delta, from -inf.  on_train_begin
      resets best, wait and the cooldown counter.
    - on_epoch_end writes logs['lr'] (the rate of the epoch that ended).  Missing monitor key: warn and skip.  In cooldown
      the counter counts down and wait stays 0; an improvement sets best and wait = 0; otherwise, out of cooldown,
      wait += 1 and at wait >= patience, if lr > min_lr: lr = max(lr * factor, min_lr), the cooldown starts
      (cooldown_counter = cooldown) and wait = 0.
    - the optimizer's rate must be a number: a LearningRateSchedule is refused (ValueError), as LearningRateScheduler
      does.  The new rate reaches the recorded step through the device descriptor (Model.fit), without recording it again."""

    def __init__(self, monitor="val_loss", factor=0.1, patience=10, verbose=0, mode="auto", min_delta=1e-4, cooldown=0,
                 min_lr=0, **kwargs):
        super().__init__()
        if factor >= 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0.")
        if "epsilon" in kwargs:
            min_delta = kwargs.pop("epsilon")
            warnings.warn("`epsilon` argument is deprecated and will be removed, use `min_delta` instead.")
        if kwargs:
            raise TypeError(f"ReduceLROnPlateau: unexpected keyword argument(s) {', '.join(sorted(kwargs))}")
        self.monitor, self.factor, self.min_lr, self.min_delta = monitor, float(factor), float(min_lr), float(min_delta)
        self.patience, self.verbose, self.cooldown, self.mode = patience, verbose, cooldown, mode
        self._reset()

    def _reset(self):
        if self.mode not in ("auto", "min", "max"):
            warnings.warn(f"Learning rate reduction mode {self.mode} is unknown, fallback to auto mode.")
            self.mode = "auto"
        if self.mode == "min" or (self.mode == "auto" and "acc" not in self.monitor):
            self.monitor_op = lambda a, b: np.less(a, b - self.min_delta)
            self.best = np.inf
        else:
            self.monitor_op = lambda a, b: np.greater(a, b + self.min_delta)
            self.best = -np.inf
        self.cooldown_counter = 0
        self.wait = 0

    def on_train_begin(self, logs=None):
        _lr_number(self.model.optimizer, "ReduceLROnPlateau")       # a schedule is refused before the first epoch
        self._reset()

    def in_cooldown(self):
        return self.cooldown_counter > 0

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        optimizer = self.model.optimizer
        logs["lr"] = _lr_number(optimizer, "ReduceLROnPlateau")
        current = logs.get(self.monitor)
        if current is None:
            warnings.warn(f"Learning rate reduction is conditioned on metric `{self.monitor}` which is not available. "
                          f"Available metrics are: {','.join(logs.keys())}")
            return
        if self.in_cooldown():
            self.cooldown_counter -= 1
            self.wait = 0
        if self.monitor_op(current, self.best):
            self.best = current
            self.wait = 0
        elif not self.in_cooldown():
            self.wait += 1
            if self.wait >= self.patience:
                old_lr = float(optimizer.lr)
                if old_lr > self.min_lr:
                    new_lr = max(old_lr * self.factor, self.min_lr)
                    optimizer.lr = new_lr
                    if self.verbose > 0:
                        print(f"\nEpoch {epoch + 1:05d}: ReduceLROnPlateau reducing learning rate to {new_lr}.")
                    self.cooldown_counter = self.cooldown
                    self.wait = 0


class LearningRateScheduler(Callback):
    """schedule(epoch, lr) -> new lr (or schedule(epoch) when the two-argument call raises TypeError), set as
    model.optimizer.lr at the beginning of every epoch; the rate of the epoch is logged as logs['lr'] at its end, so
    History.history['lr'] appears."""

    def __init__(self, schedule, verbose=0):
        super().__init__()
        self.schedule = schedule
        self.verbose = verbose

    def on_epoch_begin(self, epoch, logs=None):
        optimizer = self.model.optimizer
        if not hasattr(optimizer, "lr"):
            raise ValueError('Optimizer must have a "lr" attribute.')
        if isinstance(optimizer.lr, LearningRateSchedule):
            raise ValueError(f"LearningRateScheduler sets optimizer.lr, which is a {type(optimizer.lr).__name__} "
                             f"schedule here: give the optimizer a number, or keep the schedule without this callback")
        try:
            lr = float(optimizer.lr)
            lr = self.schedule(epoch, lr)
        except TypeError:                               # the one-argument form of older Keras
            lr = self.schedule(epoch)
        if not isinstance(lr, (float, np.float32, np.float64)):
            raise ValueError('The output of the "schedule" function should be float.')
        optimizer.lr = float(lr)
        if self.verbose > 0:
            print(f"\nEpoch {epoch + 1:05d}: LearningRateScheduler reducing learning rate to {lr}.")

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        logs["lr"] = float(self.model.optimizer.lr)


class DetectionEvaluation(Callback):
    """Puts the data set's detection metric into the epoch logs, so that EarlyStopping and ModelCheckpoint can select on it
    (ours: Keras has no counterpart).  sweeps: a list of (n, >= 3) point arrays in ego metres; boxes: a list of (m, 7) rows
    x, y, z, l, w, h, yaw as boxes.annotationBoxes returns them, one per sweep.

    At the end of every `every`-th epoch (1-based, like validation_freq) each sweep runs what Predict.detectionEval runs --
    voxelise, forward(training=False), boxes.detect(**detector) (None: boxes.rpnToRegion with its defaults), the -50 shift --
    and ONE boxes.evaluate_detections call covers all sweeps.  logs[prefix + 'mAP'], 'mAOS', 'ATE', 'ASE', 'AOE' and
    'best_f1' are set, the last four at the lowest IoU threshold; the whole result stays in `last`.  On the other epochs the
    keys are absent: a monitoring callback then warns and skips, as it does for any missing key.  min_points > 0: a box
    owning fewer points of its sweep (boxes.points_in_boxes) is ignored.  Place it in the callbacks list BEFORE the
    callbacks that monitor its keys: fit hands one logs dict to the callbacks in list order.

    average_weights=True (a model compiled with optimizers.MovingAverage / SWA; otherwise ValueError at the first
    evaluation): the averages are evaluated, so val_mAP is their score and EarlyStopping / ModelCheckpoint select on it;
    the variables and their average are swapped back afterwards, bit for bit.  With update_bn=x (what
    Model.recalibrate_batch_norm takes; only with average_weights, otherwise ValueError here) the averages are scored
    with moving statistics recalibrated for them over x by the rule `statistics` (Model.average_weights(update_bn=x)),
    and the live model's statistics are put back, bit for bit.
    Changes no variable, BatchNormalization statistic, optimizer slot or iteration count, and records nothing into a step
    plan: eager inference forwards between epochs, as fit's own validation runs them.  Data parallel: every rank evaluates
    every sweep with the rank-mean moving statistics (what save() writes), so the logs are identical on all ranks."""

    KEYS = ("mAP", "mAOS", "ATE", "ASE", "AOE", "best_f1")

    def __init__(self, sweeps, boxes, detector=None, iou_thresholds=None, mode="3d", min_points=0, every=1, prefix="val_",
                 average_weights=False, update_bn=None, statistics="mean"):
        super().__init__()
        if update_bn is not None and not average_weights:
            raise ValueError("DetectionEvaluation(update_bn=...) recalibrates the statistics for the averaged weights: "
                             "it needs average_weights=True (callbacks.PreciseBatchNorm recalibrates the live model)")
        self.update_bn, self.statistics = update_bn, _statistics(statistics)
        from .Predict import _check_detector
        sweeps, boxes = list(sweeps), [np.asarray(b, dtype=np.float64).reshape(-1, 7) for b in boxes]
        if len(sweeps) != len(boxes):
            raise ValueError(f"DetectionEvaluation needs one box set per sweep, not {len(boxes)} for {len(sweeps)}")
        if sum(len(b) for b in boxes) == 0:
            raise ValueError("DetectionEvaluation needs at least one box: the evaluation is undefined without labels")
        if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
            raise ValueError(f"every must be an integer >= 1, not {every!r}")
        _check_detector(detector)
        self.sweeps, self.boxes, self.detector = sweeps, boxes, None if detector is None else dict(detector)
        self.iou_thresholds, self.mode, self.min_points = iou_thresholds, mode, int(min_points)
        self.every, self.prefix = int(every), str(prefix)
        self.average_weights = bool(average_weights)
        self.last = None
        self._ignore = None

    def _label_ignore(self):
        """The min_points flags, counted once (sweeps and boxes do not change)."""
        if self.min_points <= 0:
            return None
        if self._ignore is None:
            from . import boxes as _boxes
            self._ignore = [_boxes.points_in_boxes(p, b) < self.min_points for p, b in zip(self.sweeps, self.boxes)]
        return self._ignore

    def evaluate(self):
        """The evaluation of the model's current weights -- with average_weights, of their averages (inside
        Model.average_weights(); the BatchNormalization moving statistics as they stand, or with update_bn recalibrated
        for the averages) --: a boxes.DetectionEval."""
        if self.average_weights and self.update_bn is not None:
            with self.model.average_weights(update_bn=self.update_bn, statistics=self.statistics):
                return self._evaluate()
        if self.average_weights:
            with self.model.average_weights():
                return self._evaluate()
        return self._evaluate()

    def _evaluate(self):
        from . import boxes as _boxes
        from .Predict import _cut_to_counts, _detect_sweep
        model = self.model
        net, dp = model.net, getattr(model, "dp", None)
        own = None
        if dp is not None:                               # as Model._eval_sums: copy, average, evaluate, restore
            own = net.params.state.clone()
            dp.average_(net.params.state)
            net.state_version += 1
        try:
            found, probs, counts = [], [], []
            for points in self.sweeps:
                for b, p, count in _detect_sweep(points, model, self.detector):
                    found.append(b)
                    probs.append(p)
                    counts.append(count)
            found, probs = _cut_to_counts(found, probs, counts)
        finally:
            if own is not None:
                net.params.state.copy_(own)
                net.state_version += 1
        return _boxes.evaluate_detections(found, probs, self.boxes, label_ignore=self._label_ignore(),
                                          iou_thresholds=self.iou_thresholds, mode=self.mode)

    def on_epoch_end(self, epoch, logs=None):
        if (epoch + 1) % self.every != 0:
            return
        r = self.last = self.evaluate()
        if logs is None:
            return
        lowest = int(np.argmin(r.thresholds))
        values = (r.mAP, r.mAOS, r.ate[lowest], r.ase[lowest], r.aoe[lowest], r.best_f1[lowest])
        for key, v in zip(self.KEYS, values):
            logs[self.prefix + key] = float(v)


class PreciseBatchNorm(Callback):
    """Re-estimates the BatchNormalization moving statistics of the LIVE model over the sweeps of x ("precise BN"; ours:
    Keras has no counterpart) at the end of every `period`-th epoch (1-based) and when training ends, by
    Model.recalibrate_batch_norm(x, steps=steps, statistics=statistics): instead of a 0.99 moving average fed by
    single-sweep batches that trails the weights, the statistics of the weights as they are over N sweeps.  x: what
    recalibrate_batch_norm takes; steps: at most that many sweeps; statistics: 'pooled' (the default here: plus the
    variance of the sweeps' means) or 'mean'.  Training goes on from the recalibrated statistics, which the next steps'
    finalisers move on from as from any others; no variable, slot or iteration count changes.
    Place it in the callbacks list BEFORE ModelCheckpoint, EarlyStopping(restore_best_weights=True) and
    DetectionEvaluation: fit calls the callbacks in list order, and a checkpoint written ahead of it would hold the
    statistics from before the recalibration.  Fit's own validation runs before any callback and sees the statistics
    of the previous recalibration.  ValueError here: a period or steps below 1, an unknown `statistics`."""

    def __init__(self, x, period=1, steps=None, statistics="pooled"):
        super().__init__()
        for name, v in (("period", period), ("steps", steps)):
            if v is None and name == "steps":
                continue
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{name} must be an integer >= 1, not {v!r}")
        self.x, self.period, self.steps = x, int(period), None if steps is None else int(steps)
        self.statistics = _statistics(statistics)
        self.calls = 0                       # recalibrations so far
        self._fresh = False                  # the statistics are those of the last recalibration (no step since)

    def _recalibrate(self):
        self.model.recalibrate_batch_norm(self.x, steps=self.steps, statistics=self.statistics)
        self.calls += 1

    def on_epoch_begin(self, epoch, logs=None):
        self._fresh = False

    def on_epoch_end(self, epoch, logs=None):
        if (epoch + 1) % self.period == 0:
            self._recalibrate()
            self._fresh = True

    def on_train_end(self, logs=None):
        if not self._fresh:                  # (the last epoch's recalibration stands: the same sweeps, the same weights)
            self._recalibrate()
