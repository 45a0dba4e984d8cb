"""The optimizers of the training step, one record each: the only place that says which hyper-parameters a tf.keras 2.4
optimizer has (their Keras order, defaults, types and ranges), which slots it keeps and which entries of lisec_amd.ops
update it.  OptimizerSpec and LisecNet (network.py), the optimizer objects and Model (model_training.py) and the Keras
checkpoint layout (keras_h5.py) all read these records; adding an optimizer means adding a record (and its kernels).

A leaf module: it imports neither torch nor the library, so keras_h5 stays usable without a GPU, and it names the ops
entries as strings, which network.py resolves.
"""
import collections


class Hyper(collections.namedtuple("Hyper", "name default below error")):
    """One hyper-parameter after learning_rate and decay.  Its type is that of its default (float or bool); a float must
    lie in [0, below) -- below None: [0, inf) -- or OptimizerSpec raises ValueError(error)."""
    __slots__ = ()

    def coerce(self, value):
        """value as the type of the default: np.float32(0.5) -> 0.5."""
        return type(self.default)(value)

    def valid(self, value):
        return self.error is None or (0 <= value and (self.below is None or value < self.below))


def _nonneg(name, default, error=None):
    return Hyper(name, default, None, error or f"{name} must be >= 0")


def _unit(name, default, error=None):
    return Hyper(name, default, 1.0, error or f"{name} must lie in [0, 1)")


def _flag(name):
    return Hyper(name, False, None, None)


# kind: the name of the slot in Keras' optimizer_weights; name: the LisecNet slot (LisecNet.slot), which differs only for
# SGD, whose Keras "momentum" is the net's velocity (RMSprop's "momentum" is a buffer of its own); when: the
# hyper-parameter that must be > 0 (a flag: set) for the slot to exist, None for a slot the optimizer always keeps
Slot = collections.namedtuple("Slot", "kind name when")


def _slot(kind, when=None, name=None):
    return Slot(kind, name or kind, when)


class Optimizer(collections.namedtuple("Optimizer", "kind class_name lr decay hyper slots step args schedule_decay "
                                                    "takes_schedule slot_start scalar layerwise",
                                        defaults=(False, True, None, None, False))):
    """kind: OptimizerSpec's; class_name: Keras'.
    lr, decay: Keras' defaults.  schedule_decay: `decay` is the optimizer's momentum-schedule decay (Nadam's
        schedule_decay), not a decay of the rate: the learning-rate descriptor is built with decay 0 and the by-value
        entry takes lr alone.  takes_schedule: a LearningRateSchedule is accepted as the rate.
    hyper: the Hypers after learning_rate and decay, in the order of Keras' get_config() -- also the order of
        OptimizerSpec.config, (kind, rate, decay, *hyper), and of optimizer_config in a checkpoint's training_config.
    slots: the Slots in Keras' order (optimizer_weights holds one kind for every variable before the next kind), which is
        also the order of the slot pointers of both entries (None for a slot that does not exist).
    slot_start: the hyper-parameter a fresh slot is filled with (None: zero).
    scalar: the float32 device scalar of LisecNet the optimizer owns besides the iteration count (None: none); the
        entries take it after the slots, a checkpoint holds it as <class_name>/<scalar>:0 after iter:0.
    step: the names of the (by-value, descriptor) entries of lisec_amd.ops:
            by value    entry(theta, grad, *slots, [scalar], lr, [decay unless schedule_decay], *args, state, advance=)
            descriptor  entry(theta, grad, *slots, [scalar], device descriptor, *args, state, advance=)
    args: the OptimizerSpec attributes both entries take after the rate.
    layerwise: the update is not element-wise -- a step of a variable depends on a reduction over the whole variable
        (LAMB's trust ratio) --, so a range of theta can only be cut at variable boundaries: both entries take the WHOLE
        buffers and, as keywords, an ops.LambTable with the rows of the range (first / n_chunks, first_var / n_vars: the
        spans of its two ChunkTables), a workspace and the ratio buffer (LisecNet._update; ops.lamb_step_dev).  Such an
        optimizer also has the two exclusion lists `lists`."""
    __slots__ = ()

    @property
    def lists(self):
        """The names of the variable lists (tuples of ParamStore names and / or kinds, or None) the optimizer's config
        carries behind its hyper-parameters: LAYERWISE_LISTS for a layer-wise optimizer, none otherwise."""
        return LAYERWISE_LISTS if self.layerwise else ()

    def values(self, given):
        """{name: value} of every hyper-parameter, from a mapping that may lack some (Keras' default), coerced."""
        return {h.name: h.coerce(given.get(h.name, h.default)) for h in self.hyper}

    def active_slots(self, hp):
        """The Slots an optimizer with the hyper-parameters hp (values()) keeps."""
        return tuple(s for s in self.slots if s.when is None or hp[s.when] > 0)

    def as_dict(self, lr, decay, hp):
        """The optimizer dict of keras_h5.save_model / load_model: class_name, lr, decay and the hyper-parameters hp."""
        head = {} if self is LEGACY else {"class_name": self.class_name}
        return dict(head, lr=lr, decay=decay, **hp)

    def launch(self, hp, device_lr):
        """How one update runs: (ops entry, its LisecNet slot names -- None for a slot that does not exist --, args)."""
        active = self.active_slots(hp)
        names = tuple(s.name if s in active else None for s in self.slots)
        if self.kind == "sgd" and not device_lr and hp["momentum"] > 0 and hp["nesterov"]:
            # the reference's configuration keeps its own kernel (eltwise.hip): always a velocity, no nesterov flag
            return "sgd_nesterov_step_dev", names, ("momentum",)
        return self.step[1 if device_lr else 0], names, self.args


LAYERWISE_LISTS = ("exclude_from_weight_decay", "exclude_from_layer_adaptation")

_BETAS = "beta_1 and beta_2 must lie in [0, 1)"
_ADAM = _BETAS + ", epsilon must be >= 0"
_EPSILON = _nonneg("epsilon", 1e-7)
_ADAMAX = (_unit("beta_1", 0.9, _BETAS), _unit("beta_2", 0.999, _BETAS), _EPSILON)

OPTIMIZERS = (
    Optimizer("sgd", "SGD", lr=0.01, decay=0.0,
              hyper=(_nonneg("momentum", 0.0), _flag("nesterov")),
              slots=(_slot("momentum", when="momentum", name="velocity"),),
              step=("sgd_step_dev", "sgd_step_sched"), args=("momentum", "nesterov")),
    Optimizer("adam", "Adam", lr=0.001, decay=0.0,
              hyper=(_unit("beta_1", 0.9, _ADAM), _unit("beta_2", 0.999, _ADAM), _nonneg("epsilon", 1e-7, _ADAM),
                     _flag("amsgrad")),
              slots=(_slot("m"), _slot("v"), _slot("vhat", when="amsgrad")),
              step=("adam_step_dev", "adam_step_sched"), args=("beta_1", "beta_2", "epsilon")),
    # momentum == 0 takes TF's Python path (epsilon outside the square root), momentum > 0 ResourceApplyRMSProp /
    # ResourceApplyCenteredRMSProp (epsilon inside it) -- see include/lisec_hip.h
    Optimizer("rmsprop", "RMSprop", lr=0.001, decay=0.0,
              hyper=(_unit("rho", 0.9), _nonneg("momentum", 0.0), _EPSILON, _flag("centered")),
              slots=(_slot("rms"), _slot("momentum", when="momentum"), _slot("mg", when="centered")),
              step=("rmsprop_step_dev", "rmsprop_step_sched"), args=("rho", "momentum", "epsilon")),
    Optimizer("adagrad", "Adagrad", lr=0.001, decay=0.0,
              hyper=(_nonneg("initial_accumulator_value", 0.1), _EPSILON),
              slots=(_slot("accumulator"),), slot_start="initial_accumulator_value",
              step=("adagrad_step_dev", "adagrad_step_sched"), args=("epsilon",)),
    Optimizer("adadelta", "Adadelta", lr=0.001, decay=0.0,
              hyper=(_unit("rho", 0.95), _EPSILON),
              slots=(_slot("accum_grad"), _slot("accum_var")),
              step=("adadelta_step_dev", "adadelta_step_sched"), args=("rho", "epsilon")),
    Optimizer("adamax", "Adamax", lr=0.001, decay=0.0,
              hyper=_ADAMAX, slots=(_slot("m"), _slot("v")),
              step=("adamax_step_dev", "adamax_step_sched"), args=("beta_1", "beta_2", "epsilon")),
    # decay is schedule_decay; momentum_cache is the product of the momentum schedule so far (1 before the first step);
    # a LearningRateSchedule is refused as in tf.keras 2.4
    Optimizer("nadam", "Nadam", lr=0.001, decay=0.004, schedule_decay=True, takes_schedule=False,
              hyper=_ADAMAX, slots=(_slot("m"), _slot("v")), scalar="momentum_cache",
              step=("nadam_step_dev", "nadam_step_sched"), args=("beta_1", "beta_2", "epsilon", "decay")),
    # tfa.optimizers.LAMB as this project restates it: Adam's step, per variable of length ||w|| / ||u||
    # (csrc/lamb.hip); weight_decay_rate is LAMB's own decay, inside the step -- not the decoupled pass of <Base>W
    Optimizer("lamb", "LAMB", lr=0.001, decay=0.0, layerwise=True,
              hyper=(_nonneg("weight_decay_rate", 0.0), _unit("beta_1", 0.9, _BETAS), _unit("beta_2", 0.999, _BETAS),
                     _nonneg("epsilon", 1e-6)),
              slots=(_slot("m"), _slot("v")),
              step=("lamb_step_dev", "lamb_step_sched"), args=("weight_decay_rate", "beta_1", "beta_2", "epsilon")),
)

BY_KIND = {o.kind: o for o in OPTIMIZERS}
BY_CLASS = {o.class_name: o for o in OPTIMIZERS}
# every LisecNet slot name / every Keras slot kind, each once, in the order of the records
SLOT_NAMES = tuple(dict.fromkeys(s.name for o in OPTIMIZERS for s in o.slots))
SLOT_KINDS = tuple(dict.fromkeys(s.kind for o in OPTIMIZERS for s in o.slots))


# SGD's optimizer dict is the one save_model took before there was a second optimizer: it has no class_name
LEGACY = BY_KIND["sgd"]


def base_class(class_name):
    """The class of the table whose record an optimizer class uses: itself for a class of the table, <Base> for <Base>W
    -- the class optimizers.extend_with_decoupled_weight_decay makes of <Base>: same kernels, same slots, no row of its
    own --, None for anything else."""
    if class_name in BY_CLASS:
        return class_name
    if isinstance(class_name, str) and class_name.endswith("W") and class_name[:-1] in BY_CLASS:
        return class_name[:-1]
    return None


def record_of(optimizer):
    """The record of an optimizer dict (Optimizer.as_dict), <Base>W resolved to <Base>'s; a class that is not in the
    table is written as SGD, as it always was."""
    return BY_CLASS.get(base_class(optimizer.get("class_name")), LEGACY)


def slot_name(class_name, kind):
    """The LisecNet slot name of the Keras slot `kind` in a file of optimizer `class_name` (one not in the table: kind)."""
    class_name = base_class(class_name)
    slots = BY_CLASS[class_name].slots if class_name in BY_CLASS else ()
    return next((s.name for s in slots if s.kind == kind), kind)
