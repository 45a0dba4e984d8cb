"""tf.keras 2.4 learning-rate schedules (tf.keras.optimizers.schedules; CosineDecay and CosineDecayRestarts are
tf.keras.experimental there), exposed as lisec_amd.model_training.optimizers.schedules.

Same constructor arguments, defaults, validation, get_config / from_config and serialize / deserialize as Keras.
`__call__(step)` evaluates in double precision, with TF's order of operations, for `step` the optimizer's iteration
count before the update (OptimizerV2._decayed_lr).  The update kernels evaluate the same formulas on the device from a
descriptor (lisec_lr_schedule, include/lisec_hip.h) that descriptor() builds: a schedule subclass of one's own cannot be
evaluated there and is refused."""
import math

from . import _lib


class LearningRateSchedule:
    """The base class of the schedules (tf.keras.optimizers.schedules.LearningRateSchedule)."""

    def __call__(self, step):
        raise NotImplementedError("Learning rate schedule must override __call__")

    def get_config(self):
        raise NotImplementedError("Learning rate schedule must override get_config")

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class ExponentialDecay(LearningRateSchedule):
    """initial_learning_rate * decay_rate ** (step / decay_steps), the exponent floored with staircase=True."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate, self.decay_steps, self.decay_rate = initial_learning_rate, decay_steps, decay_rate
        self.staircase, self.name = staircase, name

    def __call__(self, step):
        p = float(step) / float(self.decay_steps)
        if self.staircase:
            p = math.floor(p)
        return float(self.initial_learning_rate) * float(self.decay_rate) ** p

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "decay_rate": self.decay_rate, "staircase": self.staircase, "name": self.name}


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[0] for step <= boundaries[0], values[i] for boundaries[i-1] < step <= boundaries[i], values[-1] after."""

    def __init__(self, boundaries, values, name=None):
        if len(boundaries) != len(values) - 1:
            raise ValueError("The length of boundaries should be 1 less than the length of values")
        self.boundaries, self.values, self.name = boundaries, values, name

    def __call__(self, step):
        s = float(step)
        for b, v in zip(self.boundaries, self.values):
            if s <= float(b):
                return float(v)
        return float(self.values[-1])

    def get_config(self):
        return {"boundaries": self.boundaries, "values": self.values, "name": self.name}


class PolynomialDecay(LearningRateSchedule):
    """(initial - end) * (1 - step/decay_steps) ** power + end; step capped at decay_steps, or with cycle=True
    decay_steps stretched to the next multiple of itself at or above step."""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0, cycle=False, name=None):
        self.initial_learning_rate, self.decay_steps, self.end_learning_rate = (initial_learning_rate, decay_steps,
                                                                               end_learning_rate)
        self.power, self.cycle, self.name = power, cycle, name

    def __call__(self, step):
        s, d = float(step), float(self.decay_steps)
        if self.cycle:
            d = d * (1.0 if s == 0 else math.ceil(s / d))
        else:
            s = min(s, d)
        end = float(self.end_learning_rate)
        return (float(self.initial_learning_rate) - end) * (1.0 - s / d) ** float(self.power) + end

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "end_learning_rate": self.end_learning_rate, "power": self.power, "cycle": self.cycle, "name": self.name}


class InverseTimeDecay(LearningRateSchedule):
    """initial_learning_rate / (1 + decay_rate * step / decay_steps), the quotient floored with staircase=True."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate, self.decay_steps, self.decay_rate = initial_learning_rate, decay_steps, decay_rate
        self.staircase, self.name = staircase, name

    def __call__(self, step):
        p = float(step) / float(self.decay_steps)
        if self.staircase:
            p = math.floor(p)
        return float(self.initial_learning_rate) / (1.0 + float(self.decay_rate) * p)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "decay_rate": self.decay_rate, "staircase": self.staircase, "name": self.name}


class CosineDecay(LearningRateSchedule):
    """initial_learning_rate * ((1 - alpha) * 0.5 * (1 + cos(pi * min(step, decay_steps) / decay_steps)) + alpha)."""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None):
        self.initial_learning_rate, self.decay_steps, self.alpha, self.name = initial_learning_rate, decay_steps, alpha, name

    def __call__(self, step):
        d = float(self.decay_steps)
        f = min(float(step), d) / d
        c = 0.5 * (1.0 + math.cos(math.pi * f))
        a = float(self.alpha)
        return float(self.initial_learning_rate) * ((1.0 - a) * c + a)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps, "alpha": self.alpha,
                "name": self.name}


class CosineDecayRestarts(LearningRateSchedule):
    """Cosine decay with warm restarts (SGDR): period i lasts first_decay_steps * t_mul**i steps and starts at
    initial_learning_rate * m_mul**i."""

    def __init__(self, initial_learning_rate, first_decay_steps, t_mul=2.0, m_mul=1.0, alpha=0.0, name=None):
        self.initial_learning_rate, self.first_decay_steps = initial_learning_rate, first_decay_steps
        self._t_mul, self._m_mul, self.alpha, self.name = t_mul, m_mul, alpha, name

    def __call__(self, step):
        f = float(step) / float(self.first_decay_steps)
        t = float(self._t_mul)
        if t == 1.0:
            i = math.floor(f)
            f -= i
        else:
            i = math.floor(math.log(1.0 - f * (1.0 - t)) / math.log(t))
            ti = t ** i
            f = (f - (1.0 - ti) / (1.0 - t)) / ti
        c = 0.5 * float(self._m_mul) ** i * (1.0 + math.cos(math.pi * f))
        a = float(self.alpha)
        return float(self.initial_learning_rate) * ((1.0 - a) * c + a)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "first_decay_steps": self.first_decay_steps,
                "t_mul": self._t_mul, "m_mul": self._m_mul, "alpha": self.alpha, "name": self.name}


_BUILTIN = {c.__name__: c for c in (ExponentialDecay, PiecewiseConstantDecay, PolynomialDecay, InverseTimeDecay,
                                    CosineDecay, CosineDecayRestarts)}


def serialize(learning_rate_schedule):
    """{"class_name", "config"}: what Keras writes for a schedule hyper-parameter (the optimizer's get_config and the
    training_config of a saved model)."""
    return {"class_name": type(learning_rate_schedule).__name__, "config": learning_rate_schedule.get_config()}


def deserialize(config, custom_objects=None):
    """The schedule serialize() wrote; custom_objects: {class name: class} of schedules of one's own."""
    classes = dict(_BUILTIN, **(custom_objects or {}))
    name = config.get("class_name") if isinstance(config, dict) else None
    if name not in classes:
        raise ValueError(f"Unknown decay: {name}")
    return classes[name].from_config(config["config"])


# ---- the device descriptor ---------------------------------------------------------------------------------------------
KIND = {None: 0, ExponentialDecay: 1, PiecewiseConstantDecay: 2, PolynomialDecay: 3, InverseTimeDecay: 4,
        CosineDecay: 5, CosineDecayRestarts: 6}


def descriptor(learning_rate, decay=0.0):
    """The lisec_lr_schedule (an _lib.LrSchedule) of a learning rate -- a number (the constant kind) or one of the
    schedules above -- and the optimizer's legacy `decay`.  NotImplementedError for a schedule of one's own (the kernels
    evaluate the built-in formulas only); ValueError for decay_steps <= 0 or more than _lib.LR_MAX_BOUNDARIES
    boundaries."""
    d = _lib.LrSchedule()
    d.decay = float(decay)
    if not isinstance(learning_rate, LearningRateSchedule):
        d.kind, d.initial = KIND[None], float(learning_rate)
        return d
    cls = type(learning_rate)
    if cls not in KIND:
        raise NotImplementedError(f"learning-rate schedule {cls.__name__}: only the built-in Keras schedules "
                                  f"({', '.join(_BUILTIN)}) run on the device")
    s = learning_rate
    d.kind = KIND[cls]
    if cls is PiecewiseConstantDecay:
        if not 1 <= len(s.boundaries) <= _lib.LR_MAX_BOUNDARIES:
            raise ValueError(f"PiecewiseConstantDecay: 1 to {_lib.LR_MAX_BOUNDARIES} boundaries run on the device, "
                             f"not {len(s.boundaries)}")
        d.n_boundaries = len(s.boundaries)
        for i, b in enumerate(s.boundaries):
            d.boundaries[i] = float(b)
        for i, v in enumerate(s.values):
            d.values[i] = float(v)
        return d
    d.initial = float(s.initial_learning_rate)
    d.decay_steps = float(s.first_decay_steps if cls is CosineDecayRestarts else s.decay_steps)
    if not d.decay_steps > 0:
        raise ValueError(f"{cls.__name__}: decay steps must be > 0, not {d.decay_steps}")
    if cls in (ExponentialDecay, InverseTimeDecay):
        d.decay_rate, d.flag = float(s.decay_rate), int(bool(s.staircase))
    elif cls is PolynomialDecay:
        d.end_learning_rate, d.power, d.flag = float(s.end_learning_rate), float(s.power), int(bool(s.cycle))
    elif cls is CosineDecay:
        d.alpha = float(s.alpha)
    else:
        d.t_mul, d.m_mul, d.alpha = float(s._t_mul), float(s._m_mul), float(s.alpha)
    return d
