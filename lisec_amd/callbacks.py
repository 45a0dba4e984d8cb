"""tf.keras 2.4 callbacks for Model.fit(callbacks=...), exposed as lisec_amd.model_training.callbacks: the Callback base
class (set_model, set_params, on_train_begin / on_train_end, on_epoch_begin / on_epoch_end) and LearningRateScheduler.
A learning rate set between epochs reaches the update kernels through the device descriptor of LisecNet, written on
the stream of the step: the recorded step plan is not recorded again."""
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
