"""tf.keras 2.4 metrics of Model.compile(metrics=...), exposed as lisec_amd.model_training.metrics: running means over
the sweeps of an epoch (or of an evaluation) of per-sweep values that the loss kernels compute with the losses
(csrc/losses.hip).

    strings   mse, mae, mape, msle, logcosh, binary_crossentropy (probabilities), poisson (and their long names),
              binary_accuracy (threshold 0.5), accuracy / acc (categorical_accuracy for these shapes: argmax(t) == argmax(p)
              per cell, the first index winning ties)
    objects   BinaryAccuracy(threshold=), BinaryCrossentropy(from_logits=, label_smoothing=), MeanAbsoluteError(),
              MeanSquaredError()

The detection metrics are ours, not Keras': AnchorPrecision, AnchorRecall, AnchorAccuracy, PositiveMeanAbsoluteError and
PositiveIoU read the 0 / 1 / 2 label code of the VoxelNet detection loss and run only with loss='voxelnet'
(lisec_detection_metrics, csrc/detection_metrics.hip): ratios of two sums pooled over the sweeps, not means of per-sweep
values.

Importable and fully validated without the HIP library."""
from . import losses as _losses


class Metric:
    """The base class of the metric objects (tf.keras.metrics.Metric); term() is what the kernels evaluate."""

    _kind = None

    def __init__(self, name=None, dtype=None):
        self.name, self.dtype = name, dtype

    def term(self):
        if type(self) not in _BUILTIN.values():
            raise NotImplementedError(f"metric {type(self).__name__}: only {', '.join(_BUILTIN)} run in the kernels")
        return (self._kind, 0, 0.0, 0.0)

    def get_config(self):
        return {"name": self.name, "dtype": self.dtype or "float32"}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class BinaryAccuracy(Metric):
    _kind = _losses.BINARY_ACCURACY

    def __init__(self, name="binary_accuracy", dtype=None, threshold=0.5):
        super().__init__(name, dtype)
        self.threshold = threshold

    def term(self):
        return (super().term()[0], 0, float(self.threshold), 0.0)

    def get_config(self):
        return dict(super().get_config(), threshold=self.threshold)


class BinaryCrossentropy(Metric):
    _kind = _losses.BCE

    def __init__(self, name="binary_crossentropy", dtype=None, from_logits=False, label_smoothing=0):
        super().__init__(name, dtype)
        self.from_logits, self.label_smoothing = from_logits, label_smoothing
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"BinaryCrossentropy: label_smoothing must lie in [0, 1], got {label_smoothing}")

    def term(self):
        return (super().term()[0], int(bool(self.from_logits)), 0.0, float(self.label_smoothing))

    def get_config(self):
        return dict(super().get_config(), from_logits=self.from_logits, label_smoothing=self.label_smoothing)


class MeanAbsoluteError(Metric):
    _kind = _losses.MAE

    def __init__(self, name="mean_absolute_error", dtype=None):
        super().__init__(name, dtype)


class MeanSquaredError(Metric):
    _kind = _losses.MSE

    def __init__(self, name="mean_squared_error", dtype=None):
        super().__init__(name, dtype)


_BUILTIN = {c.__name__: c for c in (BinaryAccuracy, BinaryCrossentropy, MeanAbsoluteError, MeanSquaredError)}


# ---- the detection metrics (ours; Keras has no counterpart) -----------------------------------------------------------
# lisec_detection_metric kinds (LISEC_DET_METRIC_* of include/lisec_hip.h) and IoU modes (LISEC_IOU_*)
ANCHOR_PRECISION, ANCHOR_RECALL, ANCHOR_ACCURACY, POSITIVE_MAE, POSITIVE_IOU = range(5)
IOU_MODES = {"3d": 0, "bev": 1}
DET_MAX_METRICS = _losses._lib.DET_MAX_METRICS    # LISEC_DET_MAX_METRICS: over both outputs


class DetectionMetric(Metric):
    """The base class of the metrics that read the label code of the VoxelNet detection loss (y_cls 0 ignore, 1 negative,
    2 positive: pos = y_cls > 1.5, neg = 0.5 < y_cls <= 1.5, anything else, a NaN included, is ignored).  NOT Keras
    metrics: each belongs to ONE output (`output`: 0 class, 1 regression) and runs only with compile(loss='voxelnet' /
    VoxelNetLoss(...)).  Its value over an epoch or an evaluation is num/den of two sums POOLED over the sweeps (as
    tf.keras.metrics.Precision pools its counts), 0.0 when den == 0; so a sweep without positives does not poison an
    epoch.  det_term() is what lisec_detection_metrics evaluates: (kind, mode, threshold)."""

    output = None

    def term(self):
        raise NotImplementedError(f"metric {type(self).__name__} reads the label code of the detection loss: it runs only "
                                  "with compile(loss='voxelnet') / loss=VoxelNetLoss(...), not with the per-output losses")

    def det_term(self):
        if type(self) not in _DETECTION.values():
            raise NotImplementedError(f"metric {type(self).__name__}: only {', '.join(_DETECTION)} run in the kernels")
        return (self._kind, 0, 0.0)


class _ThresholdMetric(DetectionMetric):
    """With p = sigmoid(logit), evaluated in double, an anchor is predicted positive when p > threshold (a NaN logit
    compares false: predicted negative).  threshold must lie in the open interval (0, 1)."""

    output = 0

    def __init__(self, threshold=0.5, name=None, dtype=None):
        super().__init__(name, dtype)
        self.threshold = threshold
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"{type(self).__name__}: threshold must lie in the open interval (0, 1), got {threshold}")

    def det_term(self):
        return (super().det_term()[0], 0, float(self.threshold))

    def get_config(self):
        return dict(super().get_config(), threshold=self.threshold)


class AnchorPrecision(_ThresholdMetric):
    """#(positive and predicted) / #((positive or negative) and predicted) on the ClassificationLayer output.  Ours, not
    Keras' Precision: ignored anchors count nowhere."""
    _kind = ANCHOR_PRECISION

    def __init__(self, threshold=0.5, name="anchor_precision", dtype=None):
        super().__init__(threshold, name, dtype)


class AnchorRecall(_ThresholdMetric):
    """#(positive and predicted) / N_pos on the ClassificationLayer output.  Ours, not Keras' Recall."""
    _kind = ANCHOR_RECALL

    def __init__(self, threshold=0.5, name="anchor_recall", dtype=None):
        super().__init__(threshold, name, dtype)


class AnchorAccuracy(_ThresholdMetric):
    """(#(positive and predicted) + #(negative and not predicted)) / (N_pos + N_neg) on the ClassificationLayer output.
    Ours, not Keras' BinaryAccuracy, which averages over the ignored anchors too."""
    _kind = ANCHOR_ACCURACY

    def __init__(self, threshold=0.5, name="anchor_accuracy", dtype=None):
        super().__init__(threshold, name, dtype)


class PositiveMeanAbsoluteError(DetectionMetric):
    """sum over the positives of sum_k |r_k - t_k| / (7 N_pos) on the RegressionLayer output, t = y_reg - target_offset of
    the compiled VoxelNetLoss.  Ours, not Keras' MeanAbsoluteError, which averages over every cell."""
    _kind = POSITIVE_MAE
    output = 1

    def __init__(self, name="positive_mae", dtype=None):
        super().__init__(name, dtype)


class PositiveIoU(DetectionMetric):
    """The mean over the positives of IoU(decode(r), decode(t)) on the RegressionLayer output: both decoded against the
    anchor of their channel block as rpnToRegion decodes (centre offsets r0..2 * (l_a, w_a, h_a), extents exp(r3..5) *
    (l_a, w_a, h_a), yaw r6 + yaw_a), IoU as boxes.box_iou defines it; mode 'bev' (footprints) or '3d' (times the clamped
    height overlap).  A positive whose decoded box is not finite (exp overflows for an untrained head) has IoU 0 and still
    counts.  Ours, not Keras' MeanIoU."""
    _kind = POSITIVE_IOU
    output = 1

    def __init__(self, mode="bev", name="positive_iou", dtype=None):
        super().__init__(name, dtype)
        self.mode = mode
        if mode not in IOU_MODES:
            raise ValueError(f"PositiveIoU: mode must be one of {sorted(IOU_MODES)}, got {mode!r}")

    def det_term(self):
        return (super().det_term()[0], IOU_MODES[self.mode], 0.0)

    def get_config(self):
        return dict(super().get_config(), mode=self.mode)


_DETECTION = {c.__name__: c for c in (AnchorPrecision, AnchorRecall, AnchorAccuracy, PositiveMeanAbsoluteError, PositiveIoU)}
# the string forms: the class with its default arguments
DETECTION_FUNCTIONS = {"anchor_precision": AnchorPrecision, "anchor_recall": AnchorRecall, "anchor_accuracy": AnchorAccuracy,
                       "positive_mae": PositiveMeanAbsoluteError, "positive_iou": PositiveIoU}

FUNCTIONS = {k: v for k, v in _losses.FUNCTIONS.items() if k != "huber"}
FUNCTIONS.update({"binary_accuracy": (_losses.BINARY_ACCURACY, 0, 0.5, 0.0),
                  "accuracy": (_losses.CATEGORICAL_ACCURACY, 0, 0.0, 0.0),
                  "acc": (_losses.CATEGORICAL_ACCURACY, 0, 0.0, 0.0),
                  "categorical_accuracy": (_losses.CATEGORICAL_ACCURACY, 0, 0.0, 0.0)})
NOT_IMPLEMENTED_FUNCTIONS = _losses.NOT_IMPLEMENTED_FUNCTIONS | frozenset((
    "huber", "crossentropy", "ce", "sparse_categorical_accuracy", "top_k_categorical_accuracy",
    "sparse_top_k_categorical_accuracy", "auc", "precision", "recall", "mean_iou", "root_mean_squared_error"))


def get(identifier):
    if isinstance(identifier, (str, Metric)):
        return identifier
    if isinstance(identifier, dict):
        return deserialize(identifier)
    if callable(identifier):
        return identifier
    raise ValueError(f"Could not interpret metric function identifier: {identifier!r}")


def serialize(metric):
    """A name stays a name; an object becomes {"class_name", "config"} (what Keras writes in training_config)."""
    if isinstance(metric, Metric):
        return {"class_name": type(metric).__name__, "config": metric.get_config()}
    return metric


def deserialize(config, custom_objects=None):
    if isinstance(config, str):
        return config
    classes = dict(_BUILTIN, **_DETECTION, **(custom_objects or {}))
    name = config.get("class_name") if isinstance(config, dict) else None
    if name not in classes:
        raise ValueError(f"Unknown metric function: {name}")
    return classes[name].from_config(config.get("config", {}))


def metric_term(identifier):
    """(term, Keras name) of one metric: a string keeps its spelling as the name, an object its .name."""
    if isinstance(identifier, str):
        key = identifier.lower()
        if key in FUNCTIONS:
            return FUNCTIONS[key], identifier
        if key in NOT_IMPLEMENTED_FUNCTIONS:
            raise NotImplementedError(f"metric {identifier!r} is not implemented: the kernels evaluate "
                                      f"{', '.join(sorted(FUNCTIONS))}")
        if key in DETECTION_FUNCTIONS:
            return DETECTION_FUNCTIONS[key]().term()        # refuses: a detection metric needs loss='voxelnet'
        raise ValueError(f"Unknown metric function: {identifier}")
    if isinstance(identifier, Metric):
        return identifier.term(), identifier.name
    if isinstance(identifier, _losses.Loss):
        raise NotImplementedError(f"a loss object ({type(identifier).__name__}) as a metric is not implemented: use its "
                                  "metric string or metric class")
    if callable(identifier):
        raise NotImplementedError(f"metric {getattr(identifier, '__name__', identifier)!r}: a metric of one's own cannot "
                                  "run in the kernels")
    raise ValueError(f"Could not interpret metric function identifier: {identifier!r}")


def _as_list(x, what):
    if x is None:
        return []
    if isinstance(x, (list, tuple)):
        return list(x)
    return [x]


def _metrics_per_output(metrics, what):
    """[class output's list, regression output's list] of one of compile()'s metric arguments."""
    if metrics is None:
        return [[], []]
    if isinstance(metrics, dict):
        return [_as_list(m, what) for m in _losses._per_output(metrics, what)]
    if isinstance(metrics, (list, tuple)):
        nested = [isinstance(m, (list, tuple)) for m in metrics]
        if any(nested):
            if not all(nested) or len(metrics) != 2:
                raise ValueError(f"{what} as nested lists need one list per model output (2 outputs), got "
                                 f"{list(metrics)!r}")
            return [list(m) for m in metrics]
        return [list(metrics), list(metrics)]
    raise TypeError(f"Type of `{what}` argument not understood. Expected a list or dictionary, found: {metrics!r}")


def compile_metrics(metrics, weighted_metrics=None):
    """compile(metrics=..., weighted_metrics=...) -> (terms per output, names, weighted bits per output): each argument a
    list (every metric on each output), a list of two lists (one per output) or a dict keyed by output name (a metric or
    a list of them each).  Names are Keras' multi-output "<output>_<name>", in the order: the class output's metrics and
    behind them its weighted metrics, then the regression output's.  A weighted metric is named
    "<output>_weighted_<name>" (our choice: a metric in both lists has two keys); bit j of an output's word says that its
    metric j is a weighted one.  The two lists share the cap of MAX_METRICS per output."""
    per = _metrics_per_output(metrics, "metrics")
    wper = _metrics_per_output(weighted_metrics, "weighted_metrics")
    terms, names, bits = [[], []], [], [0, 0]
    for o in range(2):
        for ms, prefix in ((per[o], ""), (wper[o], "weighted_")):
            seen = set()
            for m in ms:
                t, name = metric_term(get(m))
                if name in seen:
                    raise ValueError(f"metric name {prefix + name!r} appears twice for output {_losses.OUTPUTS[o]}")
                seen.add(name)
                if prefix:
                    bits[o] |= 1 << len(terms[o])
                terms[o].append(t)
                names.append(f"{_losses.OUTPUTS[o]}_{prefix}{name}")
        if len(terms[o]) > _losses.MAX_METRICS:
            raise ValueError(f"at most {_losses.MAX_METRICS} metrics per output are implemented (metrics and "
                             f"weighted_metrics together), {_losses.OUTPUTS[o]} has {len(terms[o])}")
    return (tuple(terms[0]), tuple(terms[1])), names, tuple(bits)


def _detection_metric(identifier):
    """The DetectionMetric of one entry of compile(loss='voxelnet', metrics=...): an object, or its lower-case name (the
    class with default arguments).  Every Keras metric is refused (NotImplementedError): it would average over every cell
    of a label map that codes ignore / negative / positive."""
    m = get(identifier)
    if isinstance(m, str) and m.lower() in DETECTION_FUNCTIONS:
        return DETECTION_FUNCTIONS[m.lower()]()
    if isinstance(m, DetectionMetric):
        m.det_term()                                 # refuses a subclass of one's own
        return m
    known = isinstance(m, str) and (m.lower() in FUNCTIONS or m.lower() in NOT_IMPLEMENTED_FUNCTIONS)
    if isinstance(m, str) and not known:
        raise ValueError(f"Unknown metric function: {m}")
    raise NotImplementedError(f"metrics= with the VoxelNet detection loss takes only the detection metrics "
                              f"({', '.join(DETECTION_FUNCTIONS)}), not {getattr(m, 'name', None) or m!r}: the Keras metrics "
                              "average over every cell of a label map that codes ignore / negative / positive")


def compile_detection_metrics(metrics):
    """compile(loss='voxelnet', metrics=...) -> (terms, names): the (kind, mode, threshold) terms in the order of the
    names, "<output>_<name>", the class output's metrics first.  A detection metric belongs to one output, so a FLAT list
    routes each metric to its own output (unlike Keras, which applies a flat list to every output); a dict keyed by
    output name or a list of two lists that puts a metric on the other output is a ValueError, as are a name twice on
    one output and more than DET_MAX_METRICS metrics in all."""
    if metrics is None:
        per = [[], []]
    elif isinstance(metrics, dict):
        given = [_as_list(m, "metrics") for m in _losses._per_output(metrics, "metrics")]
        per = [[_detection_metric(m) for m in ms] for ms in given]
    elif isinstance(metrics, (list, tuple)):
        nested = [isinstance(m, (list, tuple)) for m in metrics]
        if any(nested):
            if not all(nested) or len(metrics) != 2:
                raise ValueError("metrics as nested lists need one list per model output (2 outputs), got "
                                 f"{list(metrics)!r}")
            per = [[_detection_metric(m) for m in ms] for ms in metrics]
        else:
            per = [[], []]
            for m in (_detection_metric(m) for m in metrics):
                per[m.output].append(m)
    else:
        raise TypeError(f"Type of `metrics` argument not understood. Expected a list or dictionary, found: {metrics!r}")
    terms, names = [], []
    for o, ms in enumerate(per):
        seen = set()
        for m in ms:
            if m.output != o:
                raise ValueError(f"metric {m.name!r} ({type(m).__name__}) belongs to output {_losses.OUTPUTS[m.output]}, "
                                 f"not {_losses.OUTPUTS[o]}")
            if m.name in seen:
                raise ValueError(f"metric name {m.name!r} appears twice for output {_losses.OUTPUTS[o]}")
            seen.add(m.name)
            terms.append(m.det_term())
            names.append(f"{_losses.OUTPUTS[o]}_{m.name}")
    if len(terms) > DET_MAX_METRICS:
        raise ValueError(f"at most {DET_MAX_METRICS} detection metrics in all are implemented, got {len(terms)}")
    return tuple(terms), names
