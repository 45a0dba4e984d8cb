"""tf.keras 2.4 losses (tf.keras.losses), exposed as lisec_amd.model_training.losses, and what Model.compile makes of its
loss / loss_weights / metrics arguments: a LossSpec, the descriptor (lisec_loss_cfg, include/lisec_hip.h) of the kernels
that evaluate it (csrc/losses.hip).
VoxelNetLoss is the one loss here that Keras does not have: the detection loss of VoxelNet section 2.2, a joint loss of both
outputs, compiled to a DetectionLossSpec (lisec_detection_loss_cfg, csrc/detection_loss.hip); VoxelNetIoULoss adds a
rotated-box IoU term to its regression part (DetectionIoULossSpec, lisec_detection_iou_loss_cfg, csrc/detection_iou_loss.hip).

Same names, constructor arguments, defaults, get_config / from_config and serialize / deserialize as Keras.  Every loss is
Keras' mean over the last axis and then over the cells (SUM_OVER_BATCH_SIZE): the mean over all M*C elements of an output.
A loss of one's own -- a Python callable, or a subclass with its own call() -- cannot run in the kernels and is refused
(NotImplementedError), as are the Keras losses the kernels do not implement (hinge family, categorical and sparse
cross-entropy, KL divergence, cosine similarity).  Importable and fully validated without the HIP library."""
import ctypes
import math

from . import _lib

EPSILON = 1e-7                                   # K.epsilon()
OUTPUTS = ("ClassificationLayer", "RegressionLayer")

# lisec_loss_term kinds (LISEC_LOSS_* / LISEC_METRIC_* of include/lisec_hip.h)
MSE, MAE, MAPE, MSLE, HUBER, LOGCOSH, BCE, POISSON, SIGMOID_CE_CLAMPED, SMOOTH_L1 = range(10)
BINARY_ACCURACY, CATEGORICAL_ACCURACY = 10, 11
MAX_METRICS = _lib.LOSS_MAX_METRICS


class Loss:
    """The base class of the losses (tf.keras.losses.Loss).  term() is what the kernels evaluate:
    (kind, from_logits, param, label_smoothing)."""

    _kind = None

    def __init__(self, reduction="auto", name=None):
        if reduction != "auto":
            raise NotImplementedError(f"{type(self).__name__}: only reduction='auto' (SUM_OVER_BATCH_SIZE) is implemented")
        self.reduction, self.name = reduction, name

    def __call__(self, y_true, y_pred, sample_weight=None):
        raise NotImplementedError("the losses are evaluated by the kernels of Model.fit / Model.evaluate")

    def term(self):
        if type(self) not in _BUILTIN.values() or self._kind is None:
            raise NotImplementedError(f"loss {type(self).__name__}: only the built-in Keras losses ({', '.join(_BUILTIN)}) "
                                      "run in the kernels")
        return (self._kind, 0, 0.0, 0.0)

    def get_config(self):
        return {"reduction": self.reduction, "name": self.name}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class MeanSquaredError(Loss):
    _kind = MSE

    def __init__(self, reduction="auto", name="mean_squared_error"):
        super().__init__(reduction, name)


class MeanAbsoluteError(Loss):
    _kind = MAE

    def __init__(self, reduction="auto", name="mean_absolute_error"):
        super().__init__(reduction, name)


class MeanAbsolutePercentageError(Loss):
    _kind = MAPE

    def __init__(self, reduction="auto", name="mean_absolute_percentage_error"):
        super().__init__(reduction, name)


class MeanSquaredLogarithmicError(Loss):
    _kind = MSLE

    def __init__(self, reduction="auto", name="mean_squared_logarithmic_error"):
        super().__init__(reduction, name)


class Huber(Loss):
    _kind = HUBER

    def __init__(self, delta=1.0, reduction="auto", name="huber_loss"):
        super().__init__(reduction, name)
        self.delta = delta
        if not float(delta) > 0:
            raise ValueError(f"Huber: delta must be > 0, got {delta}")

    def term(self):
        return (super().term()[0], 0, float(self.delta), 0.0)

    def get_config(self):
        return dict(super().get_config(), delta=self.delta)


class LogCosh(Loss):
    _kind = LOGCOSH

    def __init__(self, reduction="auto", name="log_cosh"):
        super().__init__(reduction, name)


class BinaryCrossentropy(Loss):
    _kind = BCE

    def __init__(self, from_logits=False, label_smoothing=0, reduction="auto", name="binary_crossentropy"):
        super().__init__(reduction, name)
        self.from_logits, self.label_smoothing = from_logits, label_smoothing
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"BinaryCrossentropy: label_smoothing must lie in [0, 1], got {label_smoothing}")

    def term(self):
        return (super().term()[0], int(bool(self.from_logits)), 0.0, float(self.label_smoothing))

    def get_config(self):
        return dict(super().get_config(), from_logits=self.from_logits, label_smoothing=self.label_smoothing)


class Poisson(Loss):
    _kind = POISSON

    def __init__(self, reduction="auto", name="poisson"):
        super().__init__(reduction, name)


class VoxelNetLoss(Loss):
    """The detection loss of VoxelNet section 2.2 on the label code of preprocessLabels / rpnTargets (y_cls 0 ignore, 1
    negative, 2 positive; y_reg non-zero on positives only, carrying the reference's +1): classification normalised
    separately over positives and negatives, SmoothL1 regression over positives only, neutral anchors ignored.  With p =
    sigmoid(logit):  L_cls = alpha/N_pos sum_pos (1-p)^gamma softplus(-z) + beta/N_neg sum_neg p^gamma softplus(z),
    L_reg = 1/N_pos sum_pos sum_k SmoothL1_b(r - (y_reg - target_offset)).  gamma=0 is the paper's loss, gamma=2 (with,
    say, alpha=0.25*2, beta=0.75*2) the focal form of SECOND / PointPillars.  Not a Keras loss: it is ONE loss of BOTH
    outputs (the class map decides where the regression counts), so compile() takes it only as loss=VoxelNetLoss(...) or
    loss='voxelnet', never per output; lisec_detection_loss (csrc/detection_loss.hip) evaluates it."""

    def __init__(self, alpha=1.5, beta=1.0, gamma=0.0, smooth_l1_beta=1.0, target_offset=1.0, reduction="auto",
                 name="voxelnet_loss"):
        super().__init__(reduction, name)
        self.alpha, self.beta, self.gamma = alpha, beta, gamma
        self.smooth_l1_beta, self.target_offset = smooth_l1_beta, target_offset
        for key in ("alpha", "beta", "gamma"):
            if not float(getattr(self, key)) >= 0:
                raise ValueError(f"VoxelNetLoss: {key} must be >= 0, got {getattr(self, key)}")
        if not float(smooth_l1_beta) > 0:
            raise ValueError(f"VoxelNetLoss: smooth_l1_beta must be > 0, got {smooth_l1_beta}")
        if not math.isfinite(float(target_offset)):
            raise ValueError(f"VoxelNetLoss: target_offset must be finite, got {target_offset}")

    def term(self):
        raise ValueError("VoxelNetLoss is a joint loss of both outputs (the class labels decide which cells the regression "
                         "counts), not a per-output loss: pass it as compile(loss=VoxelNetLoss(...)) or loss='voxelnet', "
                         "not inside a list or dict")

    def params(self):
        return tuple(float(getattr(self, k)) for k in DETECTION_PARAMS)

    def get_config(self):
        return dict(super().get_config(), **{k: getattr(self, k) for k in DETECTION_PARAMS})


class VoxelNetIoULoss(VoxelNetLoss):
    """VoxelNetLoss with a rotated-box IoU term beside SmoothL1, so that training pulls on what the Lyft metric scores:
    L_reg = 1/N_pos sum_pos [sum_k SmoothL1_b(r_k - t_k) + iou_weight (1 - IoU(decode(r), decode(t)))], with the decode and
    the IoU of metrics.PositiveIoU (iou_mode 'bev': footprints; '3d': times the clamped height overlap, over the volume of
    the union) against the anchors of the compiled spec (Constants.anchors).  The target box is a constant; a positive
    whose boxes do not overlap, or are not finite, has IoU 0 and gets no gradient from the term -- SmoothL1 still pulls it.
    iou_weight=0 is VoxelNetLoss bit for bit.  A joint loss like VoxelNetLoss: compile(loss=VoxelNetIoULoss(...)) or
    loss='voxelnet_iou', never per output; lisec_detection_iou_loss (csrc/detection_iou_loss.hip) evaluates it."""

    def __init__(self, alpha=1.5, beta=1.0, gamma=0.0, smooth_l1_beta=1.0, target_offset=1.0, iou_weight=1.0,
                 iou_mode="bev", reduction="auto", name="voxelnet_iou_loss"):
        super().__init__(alpha, beta, gamma, smooth_l1_beta, target_offset, reduction, name)
        self.iou_weight, self.iou_mode = iou_weight, iou_mode
        if not (float(iou_weight) >= 0 and math.isfinite(float(iou_weight))):
            raise ValueError(f"VoxelNetIoULoss: iou_weight must be finite and >= 0, got {iou_weight}")
        if iou_mode not in IOU_MODES:
            raise ValueError(f"VoxelNetIoULoss: iou_mode must be one of {sorted(IOU_MODES)}, got {iou_mode!r}")

    def get_config(self):
        return dict(super().get_config(), iou_weight=self.iou_weight, iou_mode=self.iou_mode)


DETECTION_PARAMS = ("alpha", "beta", "gamma", "smooth_l1_beta", "target_offset")
IOU_MODES = {"3d": 0, "bev": 1}                  # LISEC_IOU_3D, LISEC_IOU_BEV
JOINT_FUNCTIONS = {"voxelnet": VoxelNetLoss, "voxelnet_loss": VoxelNetLoss,      # names of the joint losses
                   "voxelnet_iou": VoxelNetIoULoss, "voxelnet_iou_loss": VoxelNetIoULoss}


class _NotImplementedLoss(Loss):
    """A Keras loss the kernels do not implement: it can be built and serialized, compile() refuses it."""

    def __init__(self, *args, reduction="auto", name=None, **kwargs):
        super().__init__(reduction, name)
        self._config = kwargs

    def term(self):
        raise NotImplementedError(f"loss {type(self).__name__} is not implemented: the kernels evaluate "
                                  f"{', '.join(_BUILTIN)}")

    def get_config(self):
        return dict(super().get_config(), **self._config)


class Hinge(_NotImplementedLoss):
    pass


class SquaredHinge(_NotImplementedLoss):
    pass


class CategoricalHinge(_NotImplementedLoss):
    pass


class CategoricalCrossentropy(_NotImplementedLoss):
    pass


class SparseCategoricalCrossentropy(_NotImplementedLoss):
    pass


class KLDivergence(_NotImplementedLoss):
    pass


class CosineSimilarity(_NotImplementedLoss):
    pass


_BUILTIN = {c.__name__: c for c in (MeanSquaredError, MeanAbsoluteError, MeanAbsolutePercentageError,
                                    MeanSquaredLogarithmicError, Huber, LogCosh, BinaryCrossentropy, Poisson)}
_NOT_IMPLEMENTED = {c.__name__: c for c in (Hinge, SquaredHinge, CategoricalHinge, CategoricalCrossentropy,
                                            SparseCategoricalCrossentropy, KLDivergence, CosineSimilarity)}

# the function names of tf.keras.losses (case-insensitive here, as compile() always was): name -> term
FUNCTIONS = {
    "mse": (MSE, 0, 0.0, 0.0), "mean_squared_error": (MSE, 0, 0.0, 0.0),
    "mae": (MAE, 0, 0.0, 0.0), "mean_absolute_error": (MAE, 0, 0.0, 0.0),
    "mape": (MAPE, 0, 0.0, 0.0), "mean_absolute_percentage_error": (MAPE, 0, 0.0, 0.0),
    "msle": (MSLE, 0, 0.0, 0.0), "mean_squared_logarithmic_error": (MSLE, 0, 0.0, 0.0),
    "huber": (HUBER, 0, 1.0, 0.0),
    "logcosh": (LOGCOSH, 0, 0.0, 0.0), "log_cosh": (LOGCOSH, 0, 0.0, 0.0),
    "binary_crossentropy": (BCE, 0, 0.0, 0.0),
    "poisson": (POISSON, 0, 0.0, 0.0),
}
NOT_IMPLEMENTED_FUNCTIONS = frozenset((
    "hinge", "squared_hinge", "categorical_hinge", "categorical_crossentropy", "sparse_categorical_crossentropy",
    "kld", "kl_divergence", "kullback_leibler_divergence", "cosine_similarity"))


def get(identifier):
    """A loss function name or a Loss object as is; a {"class_name", "config"} dict deserialized."""
    if identifier is None or isinstance(identifier, (str, Loss)):
        return identifier
    if isinstance(identifier, dict):
        return deserialize(identifier)
    if callable(identifier):
        return identifier
    raise ValueError(f"Could not interpret loss function identifier: {identifier!r}")


def serialize(loss):
    """A name stays a name; an object becomes {"class_name", "config"} (what Keras writes in training_config)."""
    if isinstance(loss, Loss):
        return {"class_name": type(loss).__name__, "config": loss.get_config()}
    return loss


def deserialize(config, custom_objects=None):
    if isinstance(config, str):
        return config
    classes = dict(_BUILTIN, VoxelNetLoss=VoxelNetLoss, VoxelNetIoULoss=VoxelNetIoULoss, **_NOT_IMPLEMENTED,
                   **(custom_objects or {}))
    name = config.get("class_name") if isinstance(config, dict) else None
    if name not in classes:
        raise ValueError(f"Unknown loss function: {name}")
    return classes[name].from_config(config.get("config", {}))


def loss_term(identifier):
    """The kernels' term of one output's loss.  ValueError: an unknown name; NotImplementedError: a Keras loss the
    kernels do not implement, None (no loss for the output) or a callable of one's own."""
    if identifier is None:
        raise NotImplementedError("loss=None for an output is not implemented: both outputs need a loss")
    if isinstance(identifier, str):
        key = identifier.lower()
        if key in FUNCTIONS:
            return FUNCTIONS[key]
        if key in JOINT_FUNCTIONS:
            return JOINT_FUNCTIONS[key]().term()        # refuses: a joint loss is no per-output loss
        if key in NOT_IMPLEMENTED_FUNCTIONS or identifier in _NOT_IMPLEMENTED:
            raise NotImplementedError(f"loss {identifier!r} is not implemented: the kernels evaluate "
                                      f"{', '.join(sorted(set(FUNCTIONS)))}")
        raise ValueError(f"Unknown loss function: {identifier}")
    if isinstance(identifier, Loss):
        return identifier.term()
    if callable(identifier):
        raise NotImplementedError(f"loss {getattr(identifier, '__name__', identifier)!r}: a loss of one's own cannot run "
                                  "in the kernels; use a built-in Keras loss")
    raise ValueError(f"Could not interpret loss function identifier: {identifier!r}")


# ---- compile() ---------------------------------------------------------------------------------------------------------
class LossSpec:
    """The loss of a training step as the kernels see it: per output (class, regression) the loss term, its weight and
    up to MAX_METRICS metric terms; hashable, so that it keys recorded step plans.  A term is (kind, from_logits, param,
    label_smoothing).  metric_names (Keras' "<output>_<name>", class output first) are not part of the key.
    weighted: per output, bit j = metric j is one of compile(weighted_metrics=): under sample weights it is sum w*v / sum w
    (lisec_sample_weights.weighted_metrics); without them it is the unweighted metric.  Part of the key where any is set."""

    def __init__(self, losses, weights=(1.0, 1.0), metrics=((), ()), metric_names=(), weighted=(0, 0)):
        self.losses = tuple(tuple(t) for t in losses)
        self.weights = tuple(float(w) for w in weights)
        self.metrics = tuple(tuple(tuple(t) for t in m) for m in metrics)
        self.metric_names = tuple(metric_names)
        self.weighted = tuple(int(b) for b in weighted)
        if len(self.losses) != 2 or len(self.weights) != 2 or len(self.metrics) != 2 or len(self.weighted) != 2:
            raise ValueError("a LossSpec has two outputs")
        if any(len(m) > MAX_METRICS for m in self.metrics):
            raise ValueError(f"at most {MAX_METRICS} metrics per output are implemented")
        if any(b < 0 or b >> len(m) for b, m in zip(self.weighted, self.metrics)):
            raise ValueError("a weighted-metric bit beyond the metrics of its output")

    @property
    def config(self):
        if any(self.weighted):
            return (self.losses, self.weights, self.metrics, self.weighted)
        return (self.losses, self.weights, self.metrics)

    @property
    def n_metrics(self):
        return len(self.metrics[0]) + len(self.metrics[1])

    def descriptor(self):
        """The lisec_loss_cfg (an _lib.LossCfg)."""
        d = _lib.LossCfg()

        def fill(dst, t):
            dst.kind, dst.from_logits, dst.param, dst.label_smoothing = int(t[0]), int(t[1]), float(t[2]), float(t[3])

        for o in range(2):
            fill(d.loss[o], self.losses[o])
            d.weight[o] = self.weights[o]
            d.n_metrics[o] = len(self.metrics[o])
            for j, t in enumerate(self.metrics[o]):
                fill(d.metric[o][j], t)
        return d

    def __eq__(self, other):
        return isinstance(other, LossSpec) and self.config == other.config

    def __hash__(self):
        return hash(self.config)

    def __repr__(self):
        return f"LossSpec{self.config}"


class DetectionLossSpec:
    """The VoxelNet detection loss of a training step as lisec_detection_loss sees it: the five parameters of a
    VoxelNetLoss and the loss_weights; hashable, so that it keys recorded step plans, like a LossSpec.  Its metrics are
    the detection metrics (lisec_amd/metrics.py; lisec_detection_metrics): (kind, mode, threshold) terms in the order of
    metric_names, and the anchors (l, w, h, yaw) PositiveIoU decodes against (Constants.anchors unless given).  The
    terms and anchors are part of the key -- the recorded plan contains their launch --, metric_names are not.  Without
    metrics the key is the one of a spec built from parameters and weights alone."""

    def __init__(self, params, weights=(1.0, 1.0), metrics=(), metric_names=(), anchors=None):
        self.params = tuple(float(v) for v in params)
        self.weights = tuple(float(w) for w in weights)
        self.metrics = tuple((int(k), int(m), float(t)) for k, m, t in metrics)
        self.metric_names = tuple(metric_names)
        if len(self.params) != len(DETECTION_PARAMS) or len(self.weights) != 2:
            raise ValueError("a DetectionLossSpec has five parameters and two weights")
        if len(self.metrics) > _lib.DET_MAX_METRICS:
            raise ValueError(f"at most {_lib.DET_MAX_METRICS} detection metrics are implemented")
        self.anchors = ()
        if self.metrics:
            if anchors is None:
                from . import Constants
                anchors = Constants.anchors
            self.anchors = tuple(tuple(float(v) for v in a) for a in anchors)
            if len(self.anchors) != 2 or any(len(a) != 4 for a in self.anchors):
                raise ValueError("a DetectionLossSpec with metrics has two anchors (l, w, h, yaw)")

    @property
    def config(self):
        if not self.metrics:
            return (self.params, self.weights)
        return (self.params, self.weights, self.metrics, self.anchors)

    @property
    def n_metrics(self):
        return len(self.metrics)

    def descriptor(self):
        """The lisec_detection_loss_cfg (an _lib.DetectionLossCfg)."""
        d = _lib.DetectionLossCfg()
        d.struct_bytes = ctypes.sizeof(_lib.DetectionLossCfg)
        for k, v in zip(DETECTION_PARAMS, self.params):
            setattr(d, k, v)
        d.weight[0], d.weight[1] = self.weights
        return d

    def metrics_descriptor(self):
        """The lisec_detection_metrics_cfg (an _lib.DetectionMetricsCfg) of the metrics; None without any."""
        if not self.metrics:
            return None
        d = _lib.DetectionMetricsCfg()
        d.struct_bytes = ctypes.sizeof(_lib.DetectionMetricsCfg)
        d.n_metrics = len(self.metrics)
        d.target_offset = self.params[DETECTION_PARAMS.index("target_offset")]
        for a in range(2):
            for k in range(4):
                d.anchors[a][k] = self.anchors[a][k]
        for i, (kind, mode, threshold) in enumerate(self.metrics):
            d.metric[i].kind, d.metric[i].mode, d.metric[i].threshold = kind, mode, threshold
        return d

    def __eq__(self, other):
        return isinstance(other, DetectionLossSpec) and self.config == other.config

    def __hash__(self):
        return hash(("detection",) + self.config)

    def __repr__(self):
        return f"DetectionLossSpec{self.config}"


class DetectionIoULossSpec(DetectionLossSpec):
    """The step loss of a VoxelNetIoULoss as lisec_detection_iou_loss sees it: a DetectionLossSpec -- params, weights and
    metrics are its own, and the step treats it as one -- plus iou_weight, iou_mode ('3d' / 'bev') and the anchors the term
    decodes against, which it always has (Constants.anchors unless given).  All of them are part of the key, so no
    DetectionIoULossSpec equals a DetectionLossSpec."""

    def __init__(self, params, weights=(1.0, 1.0), metrics=(), metric_names=(), anchors=None, iou_weight=1.0,
                 iou_mode="bev"):
        super().__init__(params, weights, metrics, metric_names, anchors)
        self.iou_weight, self.iou_mode = float(iou_weight), iou_mode
        if not (self.iou_weight >= 0 and math.isfinite(self.iou_weight)) or iou_mode not in IOU_MODES:
            raise ValueError("a DetectionIoULossSpec has a finite iou_weight >= 0 and the iou_mode '3d' or 'bev'")
        if not self.anchors:
            if anchors is None:
                from . import Constants
                anchors = Constants.anchors
            self.anchors = tuple(tuple(float(v) for v in a) for a in anchors)
        if len(self.anchors) != 2 or any(len(a) != 4 for a in self.anchors):
            raise ValueError("a DetectionIoULossSpec has two anchors (l, w, h, yaw)")

    @property
    def config(self):
        return (self.params, self.weights, self.metrics, self.anchors, self.iou_weight, self.iou_mode)

    def descriptor(self):
        """The lisec_detection_iou_loss_cfg (an _lib.DetectionIoULossCfg)."""
        d = _lib.DetectionIoULossCfg()
        d.struct_bytes = ctypes.sizeof(_lib.DetectionIoULossCfg)
        d.det = super().descriptor()
        d.iou_weight, d.iou_mode = self.iou_weight, IOU_MODES[self.iou_mode]
        for a in range(2):
            for k in range(4):
                d.anchors[a][k] = self.anchors[a][k]
        return d

    def __eq__(self, other):
        return isinstance(other, DetectionIoULossSpec) and self.config == other.config

    def __hash__(self):
        return hash(("detection_iou",) + self.config)

    def __repr__(self):
        return f"DetectionIoULossSpec{self.config}"


LEGACY = {"mse": ((MSE, 0, 0.0, 0.0), (MSE, 0, 0.0, 0.0)),
          "smoothl1_ce": ((SIGMOID_CE_CLAMPED, 0, 0.0, 0.0), (SMOOTH_L1, 0, 0.0, 0.0))}


def _per_output(arg, what):
    """One value for both outputs, a list of two in output order, or a dict keyed by output name -> [cls, reg]."""
    if isinstance(arg, dict):
        bad = [k for k in arg if k not in OUTPUTS]
        if bad:
            raise ValueError(f"Unknown entries in {what} dictionary: {bad}. Only expected following keys: {list(OUTPUTS)}")
        return [arg.get(o) for o in OUTPUTS]
    if isinstance(arg, (list, tuple)):
        if len(arg) != 2:
            raise ValueError(f"When passing a list as {what}, it should have one entry per model output. The model has 2 "
                             f"outputs, but you passed {what}={list(arg)!r}")
        return list(arg)
    return [arg, arg]


def _weights(loss_weights):
    if loss_weights is None:
        return (1.0, 1.0)
    if not isinstance(loss_weights, (list, tuple, dict)):
        raise ValueError(f"loss_weights must be a list or a dict, got {loss_weights!r}")
    w = _per_output(loss_weights, "loss_weights")
    return tuple(1.0 if x is None else float(x) for x in w)


def _legacy_key(loss):
    """'mse' / 'smoothl1_ce' for the spellings compile() accepted before the Keras losses, else None."""
    if isinstance(loss, str) and loss.lower() in ("smoothl1_ce",):
        return "smoothl1_ce"
    if isinstance(loss, (list, tuple)) and all(isinstance(x, str) for x in loss):
        kinds = [x.lower() for x in loss]
        if kinds == ["cross_entropy", "smooth_l1"] or kinds == ["smoothl1_ce"]:
            return "smoothl1_ce"
    return None


def _joint_loss(loss):
    """The VoxelNetLoss when compile()'s loss argument as a whole is one (an object, its name or its serialized dict),
    else None."""
    if isinstance(loss, dict) and "class_name" in loss:
        loss = deserialize(loss)
    if isinstance(loss, str) and loss.lower() in JOINT_FUNCTIONS:
        return JOINT_FUNCTIONS[loss.lower()]()
    return loss if isinstance(loss, VoxelNetLoss) else None         # a VoxelNetIoULoss is one


def compile_loss(loss, loss_weights=None, metrics=None, weighted_metrics=None):
    """The step loss of a compile() without weighted metrics: compile_weighted_loss(loss, loss_weights, metrics), whose
    description is this function's.  weighted_metrics other than None is refused here (NotImplementedError), as it
    always was: a step compiled through this function knows no sample weights.  Model.compile goes through
    compile_weighted_loss."""
    if weighted_metrics is not None:
        raise NotImplementedError("weighted_metrics is not implemented by compile_loss (a step without sample weights): "
                                  "compile_weighted_loss, which Model.compile calls, takes them")
    return compile_weighted_loss(loss, loss_weights, metrics)


def compile_weighted_loss(loss, loss_weights=None, metrics=None, weighted_metrics=None):
    """Model.compile's loss arguments -> (step loss, metric names).  The step loss is the plain string 'mse' or
    'smoothl1_ce' -- lisec_rpn_loss, the reference's step unchanged -- when the loss is MSE on both outputs, or the legacy
    'smoothl1_ce' spelling, with neither loss_weights nor metrics; a DetectionLossSpec (lisec_detection_loss) for a
    VoxelNetLoss or 'voxelnet', a DetectionIoULossSpec (lisec_detection_iou_loss) for a VoxelNetIoULoss or
    'voxelnet_iou'; otherwise a LossSpec (lisec_head_loss).  With the detection loss, metrics takes the
    detection metrics of lisec_amd/metrics.py and only those (metrics.compile_detection_metrics: a flat list routes each
    metric to its own output); with every other loss, the Keras metrics and only those.  Every refusal is raised here:
    ValueError (unknown name, unknown output key, a list of the wrong length, a VoxelNetLoss given per output, a
    detection metric on the wrong output, too many of them), NotImplementedError (a Keras loss or metric the kernels do
    not implement, one's own callable, loss=None for an output, weighted_metrics with a VoxelNetLoss, a Keras metric with
    a VoxelNetLoss, a detection metric without one).
    weighted_metrics takes the Keras metrics in the forms metrics= takes; an output's weighted metrics follow its
    metrics (Keras' order) under the names "<output>_weighted_<name>", and share the cap of MAX_METRICS per output."""
    from . import metrics as metrics_mod
    joint = _joint_loss(loss)
    if joint is not None:
        if weighted_metrics is not None:
            raise NotImplementedError("weighted_metrics with the VoxelNet detection loss is not implemented: the detection "
                                      "metrics stay unweighted")
        mterms, names = metrics_mod.compile_detection_metrics(metrics)
        if isinstance(joint, VoxelNetIoULoss):
            return DetectionIoULossSpec(joint.params(), _weights(loss_weights), mterms, names,
                                        iou_weight=joint.iou_weight, iou_mode=joint.iou_mode), list(names)
        return DetectionLossSpec(joint.params(), _weights(loss_weights), mterms, names), list(names)
    legacy = _legacy_key(loss)
    if legacy is not None:
        terms = LEGACY[legacy]
    else:
        terms = tuple(loss_term(get(x)) for x in _per_output(loss, "loss"))
    weights = _weights(loss_weights)
    mterms, names, weighted = metrics_mod.compile_metrics(metrics, weighted_metrics)
    if loss_weights is None and not any(mterms):
        if legacy is not None:
            return legacy, []
        if terms == LEGACY["mse"]:
            return "mse", []
    return LossSpec(terms, weights, mterms, names, weighted), list(names)
