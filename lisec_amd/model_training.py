"""Drop-in counterpart of the reference's model_training.py (same public names and argument order):

    get_voxel, VFE_preprocessing, combine_lidar_data, rotate_points, RepeatLayer, MaxPoolingVFELayer,
    createModel, load_model, optimizers.SGD, optimizers.Adam, train, train_with_model

and, for Model.fit / Model.evaluate, the tf.keras 2.4 learning-rate schedules (optimizers.schedules), callbacks
(callbacks.Callback, LearningRateScheduler, EarlyStopping, ModelCheckpoint, ReduceLROnPlateau), losses and metrics
(losses.MeanSquaredError, ..., BinaryCrossentropy, Huber; metrics.BinaryAccuracy, ...) of compile(), and the weight
regularizers (regularizers.l1, l2, l1_l2; createModel(..., kernel_regularizer=...)).

The Keras graph is replaced by lisec_amd.network.LisecNet (HIP kernels behind the C ABI); lidar sweeps
stay sparse on the GPU instead of being densified to (8,200,400,35,6) and stacked in host RAM
(reference model_training.py:279,285).  There is no CPU fallback.
"""
import collections.abc
import contextlib
import json
import math
import numbers
import os
import time
import warnings

import numpy as np
import torch

from . import Constants, _lib
from . import callbacks, losses, lr_schedules, metrics, mixed_precision, ops, optimizer_table, regularizers
from .network import (AverageSpec, ClipSpec, DecaySpec, EvalStep, LisecNet, OptimizerSpec, PipelinedStep, RecordedStep,
                      loss_acc_len, loss_acc_logs, loss_acc_split, weight_form)
from .params import ParamStore, fold_depth, param_specs
from .voxelizer import VoxelSample, Voxelizer, check_subsample, host_row_stats


# ---------------------------------------------------------------------------------------------------
# voxeliser front end (reference model_training.py:103-152)
def get_voxel(point, xSize, ySize, zSize):
    """Voxel coordinate of a point; voxels are named by their lower corner (model_training.py:103-107)."""
    from math import floor
    return (floor(point[0] / xSize), floor(point[1] / ySize), floor(point[2] / zSize))


_VOXELIZERS = {}


def VFE_preprocessing(points, xSize, ySize, zSize, sampleSize, maxVoxelX, maxVoxelY, maxVoxelZ, seed=None, item=0, epoch=0):
    """points (n, >=3) -> SparseVoxels, the stand-in for the tf.SparseTensor of dense_shape
    [maxVoxelZ, 2*maxVoxelX, 2*maxVoxelY, sampleSize, 6] the reference returns (model_training.py:112-152).
    Deterministic: a voxel holding more than sampleSize points keeps the lowest point indices (seed=None) or, with a
    seed, the reference's random sampleSize of them as the draw of (seed, item, epoch) (Voxelizer(subsample='random'));
    the slots stay in ascending point index."""
    key = (float(xSize), float(ySize), float(zSize), int(sampleSize), int(maxVoxelX), int(maxVoxelY), int(maxVoxelZ))
    if seed is not None:
        rkey = key + ("random",)
        if rkey not in _VOXELIZERS:
            _VOXELIZERS[rkey] = Voxelizer(*key[:3], key[3], *key[4:], subsample="random")
        vox = _VOXELIZERS[rkey]
        vox.seed = int(seed)
        return SparseVoxels(vox(points, draw=(item, epoch)))
    if key not in _VOXELIZERS:
        _VOXELIZERS[key] = Voxelizer(*key[:3], key[3], *key[4:])
    return SparseVoxels(_VOXELIZERS[key](points))


def _sequence_subsample(seq):
    """The voxeliser's subsample mode for a Sequence of raw sweeps: its `subsample` when its items carry their draw into a
    recorded step (AugmentedSweeps.staged), else 'first'."""
    return check_subsample(getattr(seq, "subsample", "first")) if hasattr(seq, "staged") else "first"


class SparseVoxels:
    """Quacks like the SparseTensor the reference builds: .indices (z,x,y,t,f), .values, .dense_shape
    (materialised on the host only when asked for); carries the device-resident VoxelSample the network eats."""

    def __init__(self, sample):
        self.sample = sample
        c = sample.cfg
        self.dense_shape = [c.maxVoxelZ, 2 * c.maxVoxelX, 2 * c.maxVoxelY, c.sampleSize, 6]
        self.shape = tuple(self.dense_shape)
        self._coo = None

    def _materialise(self):
        if self._coo is None:
            h = self.sample.to_host()
            V, T = len(h["coords"]), self.sample.cfg.sampleSize
            idx = np.empty((V, T, 6, 5), dtype=np.int64)
            idx[..., :3] = h["coords"][:, None, None, :]
            idx[..., 3] = np.arange(T)[None, :, None]
            idx[..., 4] = np.arange(6)[None, None, :]
            self._coo = (idx.reshape(-1, 5), h["feats"].reshape(-1))
        return self._coo

    @property
    def indices(self):
        return self._materialise()[0]

    @property
    def values(self):
        return self._materialise()[1]


class sparse:   # noqa: N801  (mirrors `from tensorflow import sparse`)
    @staticmethod
    def to_dense(st, default_value=0., validate_indices=False):
        """tf.sparse.to_dense (model_training.py:279): host numpy array of st.dense_shape.  Only meant for
        small grids / inspection -- the network consumes the sparse form directly."""
        dense = np.full(st.dense_shape, default_value, dtype=np.float32)
        idx, val = st.indices, st.values
        dense[tuple(idx.T)] = val
        return dense

    @staticmethod
    def reshape(st, shape):
        return st            # (1,) + shape: the batch axis is implicit (Predict.py:29)


def dense_to_sample(dense, device=None):
    """(D,H,W,T,6) dense array -> VoxelSample.  Every row of a non-empty voxel is kept as a real row
    (zero rows are numerically identical to pad rows), so this is exact for ANY dense input."""
    device = device or _lib.require_gpu()
    dense = np.asarray(dense, dtype=np.float32)
    D, H, W, T, F = dense.shape
    if F != 6:
        raise ValueError("last axis must be 6")
    flat = dense.reshape(D * H * W, T, 6)
    occ = np.nonzero(np.abs(flat).reshape(len(flat), -1).max(1) > 0)[0]
    V = len(occ)
    cfg = _lib.VoxelCfg(1.0, 1.0, 1.0, H // 2, W // 2, D, T)
    cell_voxel = np.full(D * H * W, -1, np.int32)
    cell_voxel[occ] = np.arange(V, dtype=np.int32)
    coords = np.stack([occ // (H * W), (occ // W) % H, occ % W], 1).astype(np.int32)
    npts = np.full(V, T, np.int32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)  # noqa: E731
    n_rows = max(V * T, 1)
    rows = np.zeros((n_rows, 6), np.float32)
    rows[:V * T] = flat[occ].reshape(-1, 6)
    s = VoxelSample(cfg, n_rows, max(V, 1), t(np.array([V, V * T, V * T, T, 0, 0, 0, 0]), torch.int32),
                    t(cell_voxel, torch.int32), t(coords if V else np.zeros((1, 3)), torch.int32),
                    t(npts if V else np.zeros(1), torch.int32), t(npts if V else np.zeros(1), torch.int32),
                    t(np.arange(max(V, 1) + 1) * T, torch.int32), t(rows, torch.float32),
                    t(np.arange(n_rows), torch.int32), t(host_row_stats(rows[:V * T]), torch.int64))
    return s


# ---------------------------------------------------------------------------------------------------
# lidar assembly (reference model_training.py:65-98)
def _quaternion_matrix(q):
    w, x, y, z = (float(v) for v in q)
    n = (w * w + x * x + y * y + z * z) ** 0.5
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rotate_points(points, rotation, inverse=False):
    """Rotate by a (w,x,y,z) quaternion (model_training.py:65-69)."""
    R = _quaternion_matrix(rotation)
    if inverse:
        R = R.T
    return np.dot(R, np.asarray(points).T).T


def combine_lidar_data(sample, dataDir, level5Data):
    """Every lidar point of a sample in the car frame, float64 (n,3) (model_training.py:73-98)."""
    sensorTypes = ['LIDAR_TOP', 'LIDAR_FRONT_RIGHT', 'LIDAR_FRONT_LEFT']
    actual = [s for s in sensorTypes if s in sample['data']]     # not every sample has all three (:75-79)
    allPoints = []
    for sensorType in actual:
        frame = level5Data.get('sample_data', sample['data'][sensorType])
        sensor = level5Data.get('calibrated_sensor', frame['calibrated_sensor_token'])
        filePath = os.path.join(dataDir, *frame['filename'].replace('\\', '/').split('/'))
        raw = np.fromfile(filePath, dtype=np.float32).reshape(-1, 5)[:, :3]          # :87-90
        pts = rotate_points(raw, sensor['rotation']) + np.array(sensor['translation'])   # :93-94
        allPoints.append(pts)
    return np.concatenate(allPoints)


def combine_lidar_data_gpu(sample, dataDir, level5Data, device=None):
    """combine_lidar_data with the rotate + translate + concatenate done on the GPU: the raw float32 .bin rows
    are uploaded once (20 B/point) and the float64 (n,3) cloud never exists on the host.  Returns a device
    tensor that VFE_preprocessing accepts directly."""
    import ctypes
    device = device or _lib.require_gpu()
    lib = _lib.load()
    sensorTypes = ['LIDAR_TOP', 'LIDAR_FRONT_RIGHT', 'LIDAR_FRONT_LEFT']
    frames = []
    for sensorType in [s for s in sensorTypes if s in sample['data']]:
        frame = level5Data.get('sample_data', sample['data'][sensorType])
        sensor = level5Data.get('calibrated_sensor', frame['calibrated_sensor_token'])
        filePath = os.path.join(dataDir, *frame['filename'].replace('\\', '/').split('/'))
        raw = np.fromfile(filePath, dtype=np.float32).reshape(-1, 5)
        frames.append((raw, sensor))
    total = sum(len(r) for r, _ in frames)
    out = torch.empty((total, 3), dtype=torch.float64, device=device)
    at = 0
    for raw, sensor in frames:
        d_raw = torch.from_numpy(raw).to(device)
        R = np.ascontiguousarray(_quaternion_matrix(sensor['rotation']), dtype=np.float64)
        t = np.ascontiguousarray(np.asarray(sensor['translation'], dtype=np.float64))
        _lib.check(lib.lisec_lidar_transform(
            _lib.ptr(d_raw), len(raw), 5, R.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.c_void_p(out.data_ptr() + at * 24),
            _lib.current_stream()))
        at += len(raw)
    return out


# ---------------------------------------------------------------------------------------------------
# the two custom layers the reference names in custom_objects (model_training.py:32-61)
class RepeatLayer:
    """repeat_elements(x, maxPoints, axis=-2): (…,1,C) -> (…,35,C)."""

    def __init__(self, **kwargs):
        pass

    def compute_output_shape(self, inputShape):
        """(…, 1, C) -> (…, maxPoints, C) (reference model_training.py:36-37)."""
        inputShape = tuple(inputShape)
        return inputShape[:Constants.pointIndex] + (Constants.maxPoints,) + inputShape[Constants.pointIndex + 1:]

    def __call__(self, inputs):
        return torch.repeat_interleave(torch.as_tensor(inputs), Constants.maxPoints, dim=Constants.pointIndex)

    call = __call__


class MaxPoolingVFELayer:
    """max over the point axis, keepdims unless combine=True; pad rows take part (no mask)."""

    def __init__(self, combine=False, **kwargs):
        self.combineDim = combine

    def compute_output_shape(self, inputShape):
        """(…, T, C) -> (…, 1, C), or (…, C) with combine=True (reference model_training.py:49-53)."""
        inputShape = tuple(inputShape)
        mid = () if self.combineDim else (1,)
        return inputShape[:Constants.pointIndex] + mid + inputShape[Constants.pointIndex + 1:]

    def __call__(self, inputs):
        return torch.as_tensor(inputs).max(dim=Constants.pointIndex, keepdim=not self.combineDim).values

    call = __call__

    def get_config(self):
        return {'combine': self.combineDim}


# ---------------------------------------------------------------------------------------------------
_CLIP_KINDS = {"clipnorm": "norm", "clipvalue": "value", "global_clipnorm": "global_norm"}      # attribute -> ClipSpec kind


def _no_clipping(cls, kwargs):
    """tf.keras optimizers take clipnorm / clipvalue / global_clipnorm as constructor keywords: those stay refused here.
    Clipping is set on the constructed optimizer: the attributes of the same names, or optimizers.clip_gradients."""
    clip = sorted(k for k in _CLIP_KINDS if kwargs.get(k) is not None)
    if clip:
        raise NotImplementedError(f"{cls}: gradient clipping ({', '.join(clip)}) is not implemented as a constructor "
                                  f"keyword: use optimizers.clip_gradients(optimizer, ...) or assign the attribute")
    rest = sorted(k for k in kwargs if k not in _CLIP_KINDS)
    if rest:
        raise TypeError(f"{cls}: unexpected keyword argument(s) {', '.join(rest)}")


def _clip_spec(clipnorm, clipvalue, global_clipnorm):
    """The ClipSpec of the three thresholds; None when all are None.  ValueError: more than one at once (tf.keras 2.4
    takes clipvalue beside a norm; that combination is refused here), or a threshold that is not a finite number > 0."""
    given = {k: v for k, v in (("clipnorm", clipnorm), ("clipvalue", clipvalue), ("global_clipnorm", global_clipnorm))
             if v is not None}
    if len(given) > 1:
        raise ValueError(f"exactly one of clipnorm, clipvalue and global_clipnorm may be set, not {', '.join(given)}")
    for key, value in given.items():
        return ClipSpec(_CLIP_KINDS[key], value)
    return None


def _rate(lr):
    """A learning rate as the optimizers keep it: a LearningRateSchedule as is, anything else as a float."""
    return lr if isinstance(lr, lr_schedules.LearningRateSchedule) else float(lr)


def _serialize_rate(lr):
    """Keras' _serialize_hyperparameter: a schedule as its {"class_name", "config"} dict."""
    return lr_schedules.serialize(lr) if isinstance(lr, lr_schedules.LearningRateSchedule) else lr


class _Optimizer:
    """What the optimizers share: the attributes (lr, decay, name and the hyper-parameters of the class's record in
    lisec_amd/optimizer_table.py), spec() and get_config().  lr stays a plain attribute -- callbacks assign it between
    epochs -- that spec() reads when it is called.  clipnorm, clipvalue and global_clipnorm are plain attributes too:
    None after construction (the constructor keywords are refused), assignable afterwards or set by
    optimizers.clip_gradients; spec() validates them, as they may have been assigned directly."""

    clipnorm = clipvalue = global_clipnorm = None

    @property
    def record(self):
        return optimizer_table.BY_CLASS[optimizer_table.base_class(type(self).__name__)]

    def clip_spec(self):
        """The ClipSpec of the clipping attributes; None when none is set.  ValueError: _clip_spec's."""
        return _clip_spec(self.clipnorm, self.clipvalue, self.global_clipnorm)

    def _clip_config(self):
        """The clipping keys of get_config(): as in Keras, a key is there only when its value is not None."""
        return {k: getattr(self, k) for k in _CLIP_KINDS if getattr(self, k) is not None}

    def decay_spec(self):
        """The DecaySpec of the optimizer's decoupled weight decay; None for an optimizer without one."""
        return None

    def _set(self, name, lr, decay, kwargs, **hyper):
        _no_clipping(type(self).__name__, kwargs)
        self.lr = _rate(lr)
        self.decay, self.name = float(decay), name
        for h in self.record.hyper:
            setattr(self, h.name, h.coerce(hyper[h.name]))
        self.spec()                 # range checks; a schedule the kernels cannot evaluate (or Nadam any) is refused here

    @property
    def hyper(self):
        """{name: value} of the hyper-parameters after the rate and decay, in the order of Keras' get_config()."""
        return {h.name: getattr(self, h.name) for h in self.record.hyper}

    def spec(self, device_lr=False):
        """device_lr: the kernels read the rate from the device descriptor even when it is a number (Model.fit with
        callbacks, which may change it between epochs)."""
        return OptimizerSpec(self.record.kind, self.lr, self.decay, device_lr=device_lr, weight_decay=self.decay_spec(),
                             clip=self.clip_spec(), **self.hyper, **self.lists)

    @property
    def lists(self):
        """{name: value} of the variable lists of the class's record (a layer-wise optimizer's exclusion lists; none
        for every other class)."""
        return {name: getattr(self, name) for name in self.record.lists}

    def get_config(self):
        return {"name": self.name, "learning_rate": _serialize_rate(self.lr), "decay": self.decay, **self.hyper,
                **self._clip_config()}


class _DecoupledWeightDecay:
    """What the classes of optimizers.extend_with_decoupled_weight_decay put in front of their base optimizer: the
    first argument weight_decay -- a number or a built-in LearningRateSchedule, a plain attribute that a callback may
    assign between epochs, like lr --, the keyword decay_var_list, the DecaySpec in spec() and both in get_config().
    The record, the kernels and the slots are the base class's."""

    def _set_decay(self, weight_decay, decay_var_list):
        if not isinstance(weight_decay, lr_schedules.LearningRateSchedule):
            DecaySpec(weight_decay)                 # ValueError for anything but a finite number >= 0
            weight_decay = float(weight_decay)
        self.weight_decay = weight_decay
        if decay_var_list is not None:
            decay_var_list = [decay_var_list] if isinstance(decay_var_list, str) else list(decay_var_list)
        self.decay_var_list = decay_var_list
        self.decay_spec()           # the range checks; a schedule the kernel cannot evaluate is refused here

    def decay_spec(self):
        return DecaySpec(self.weight_decay, self.decay_var_list)

    def get_config(self):
        config = super().get_config()
        clip = {k: config.pop(k) for k in _CLIP_KINDS if k in config}        # (stay last, as a checkpoint writes them)
        config["weight_decay"] = _serialize_rate(self.weight_decay)
        if self.decay_var_list is not None:
            config["decay_var_list"] = list(self.decay_var_list)
        config.update(clip)
        return config


class _AveragingOptimizer(_Optimizer):
    """What optimizers.MovingAverage and optimizers.SWA share: the wrapped optimizer, to which lr, decay and every
    hyper-parameter read and write through (ReduceLROnPlateau and LearningRateScheduler assign optimizer.lr), the spec --
    the wrapped optimizer's with an AverageSpec --, the nested config and the calls that use the averages."""

    _OWN = ("name",)                     # the wrapper's own attributes; every other one is the wrapped optimizer's

    def _wrap(self, optimizer, name):
        if isinstance(optimizer, _AveragingOptimizer):
            raise ValueError(f"{type(self).__name__} cannot wrap {type(optimizer).__name__}: one averaging wrapper at most")
        if not isinstance(optimizer, (str, _Optimizer)):
            raise ValueError(f"{type(self).__name__}: optimizer must be an optimizer object or 'sgd' / 'adam', "
                             f"not {optimizer!r}")
        object.__setattr__(self, "_optimizer", optimizers.get(optimizer))
        self.name = name

    @property
    def record(self):
        return self._optimizer.record

    # the clipping attributes are class attributes of _Optimizer, which __getattr__ below would never be asked for: they
    # read through to the wrapped optimizer by name (assignments go there through __setattr__, like lr)
    clipnorm = property(lambda self: self._optimizer.clipnorm)
    clipvalue = property(lambda self: self._optimizer.clipvalue)
    global_clipnorm = property(lambda self: self._optimizer.global_clipnorm)

    def __getattr__(self, attr):             # only reached for what the wrapper does not have itself
        if attr.startswith("_"):
            raise AttributeError(attr)
        return getattr(self._optimizer, attr)

    def __setattr__(self, attr, value):
        if attr in self._OWN or attr.startswith("_"):
            object.__setattr__(self, attr, value)
        else:
            setattr(self._optimizer, attr, value)

    def spec(self, device_lr=False):
        inner = self._optimizer
        return OptimizerSpec(inner.record.kind, inner.lr, inner.decay, device_lr=device_lr, average=self.average_spec(),
                             weight_decay=inner.decay_spec(), clip=inner.clip_spec(), **inner.hyper, **inner.lists)

    def decay_spec(self):
        return self._optimizer.decay_spec()

    def _nested(self):
        inner = self._optimizer
        return {"class_name": type(inner).__name__, "config": inner.get_config()}

    @staticmethod
    def _net_of(model):
        if not isinstance(getattr(model, "optimizer", None), _AveragingOptimizer):
            raise ValueError("the model is not compiled with an averaging optimizer (optimizers.MovingAverage / SWA)")
        return model.net

    def assign_average_vars(self, model):
        """theta <- average on `model` (a Model compiled with this optimizer); the average is kept.  Training that
        follows goes on from the averages."""
        self._net_of(model).assign_average()

    def swap_weights(self, model):
        """theta <-> average on `model`, by content (LisecNet.swap_average); a second call swaps back, bit for bit."""
        self._net_of(model).swap_average()


def _step_number(name, value):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{name} must be an integer, not {value!r}")
    return int(value)


def _momentum_in_unit_interval(momentum):
    """Keras' own check of SGD and RMSprop (OptimizerSpec only asks for momentum >= 0)."""
    if not 0.0 <= float(momentum) <= 1.0:
        raise ValueError("`momentum` must be between [0, 1].")


class optimizers:   # noqa: N801  (mirrors `from tensorflow.keras import optimizers`)
    """tf.keras 2.4 SGD, Adam, RMSprop, Adagrad, Adadelta, Adamax and Nadam (OptimizerV2): lr_t = lr / (1 +
    decay*iterations) (Nadam: lr), lr either a number or one of the built-in schedules of optimizers.schedules (then
    lr_t = schedule(iterations) / (1 + decay*iterations); not for Nadam); `lr=` is the legacy spelling of
    `learning_rate=`.  The updates run as HIP kernels on the flat variables (csrc/eltwise.hip, csrc/optim.hip,
    csrc/optim_keras.hip).  The signatures mirror Keras'; everything else about an optimizer is its record in
    lisec_amd/optimizer_table.py."""

    schedules = lr_schedules

    class SGD(_Optimizer):
        def __init__(self, lr=0.01, decay=0.0, momentum=0.0, nesterov=False, learning_rate=None, name="SGD", **kwargs):
            _momentum_in_unit_interval(momentum)
            self._set(name, learning_rate if learning_rate is not None else lr, decay, kwargs, momentum=momentum,
                      nesterov=nesterov)

    class Adam(_Optimizer):
        def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, name="Adam",
                     lr=None, decay=0.0, **kwargs):
            self._set(name, lr if lr is not None else learning_rate, decay, kwargs, beta_1=beta_1, beta_2=beta_2,
                      epsilon=epsilon, amsgrad=amsgrad)

    class RMSprop(_Optimizer):
        """Keras' RMSprop: momentum == 0 takes TF's Python path (epsilon outside the square root), momentum > 0
        ResourceApplyRMSProp / ResourceApplyCenteredRMSProp (epsilon inside it) -- see include/lisec_hip.h."""

        def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, name="RMSprop",
                     lr=None, decay=0.0, **kwargs):
            _momentum_in_unit_interval(momentum)
            self._set(name, lr if lr is not None else learning_rate, decay, kwargs, rho=rho, momentum=momentum,
                      epsilon=epsilon, centered=centered)

    class Adagrad(_Optimizer):
        def __init__(self, learning_rate=0.001, initial_accumulator_value=0.1, epsilon=1e-7, name="Adagrad", lr=None,
                     decay=0.0, **kwargs):
            if initial_accumulator_value < 0.0:
                raise ValueError(f"initial_accumulator_value must be non-negative: {initial_accumulator_value}")
            self._set(name, lr if lr is not None else learning_rate, decay, kwargs,
                      initial_accumulator_value=initial_accumulator_value, epsilon=epsilon)

    class Adadelta(_Optimizer):
        def __init__(self, learning_rate=0.001, rho=0.95, epsilon=1e-7, name="Adadelta", lr=None, decay=0.0, **kwargs):
            self._set(name, lr if lr is not None else learning_rate, decay, kwargs, rho=rho, epsilon=epsilon)

    class Adamax(_Optimizer):
        def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, name="Adamax", lr=None,
                     decay=0.0, **kwargs):
            self._set(name, lr if lr is not None else learning_rate, decay, kwargs, beta_1=beta_1, beta_2=beta_2,
                      epsilon=epsilon)

    class Nadam(_Optimizer):
        """Keras' Nadam: `decay` is the momentum-schedule decay (schedule_decay, default 0.004; `decay=` is taken as
        its alias, the key its config is saved under), and the learning rate is never divided by 1 + decay*iterations.
        A LearningRateSchedule is refused (ValueError), as in tf.keras 2.4; a rate set by a callback still reaches the
        kernels through the device descriptor."""

        def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, name="Nadam", lr=None,
                     schedule_decay=0.004, decay=None, **kwargs):
            self._set(name, lr if lr is not None else learning_rate, schedule_decay if decay is None else decay, kwargs,
                      beta_1=beta_1, beta_2=beta_2, epsilon=epsilon)

    class AdamW(_DecoupledWeightDecay, Adam):
        """tfa.optimizers.AdamW as this project restates it (parity unpinned): Adam with DECOUPLED weight
        decay.  Directly in front of every update w <- w - wd_t*w (a float32 multiply and a float32 subtraction;
        csrc/weight_decay.hip), then Adam updates the decayed variable.  weight_decay: a number or one of the built-in
        schedules of optimizers.schedules, evaluated at the iteration count before the update; a plain attribute that a
        callback may assign between epochs.  As in tfa, the decay is NOT multiplied by the learning rate: who
        schedules the one must schedule the other.  decay_var_list: the variables to decay -- ParamStore names and / or
        the kinds 'kernel', 'bias', 'gamma', 'beta'; None: every trainable variable, tfa's default.  It is a
        constructor keyword here: tfa passes it to minimize(), which this API does not have.  lr=, decay= and the
        clipping keywords behave as in Adam (clipping is refused).  ValueError: a weight_decay that is not a finite
        number >= 0; NotImplementedError: a schedule of one's own."""

        def __init__(self, weight_decay, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False,
                     name="AdamW", decay_var_list=None, **kwargs):
            self._set_decay(weight_decay, decay_var_list)
            optimizers.Adam.__init__(self, learning_rate=learning_rate, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon,
                                     amsgrad=amsgrad, name=name, **kwargs)

    class SGDW(_DecoupledWeightDecay, SGD):
        """tfa.optimizers.SGDW as this project restates it (parity unpinned): SGD (momentum, Nesterov) on the variables
        after w <- w - wd_t*w.  Arguments as in AdamW; tfa's default learning rate of 0.001, not SGD's 0.01."""

        def __init__(self, weight_decay, learning_rate=0.001, momentum=0.0, nesterov=False, name="SGDW",
                     decay_var_list=None, **kwargs):
            self._set_decay(weight_decay, decay_var_list)
            lr = kwargs.pop("lr", None)
            optimizers.SGD.__init__(self, lr=lr if lr is not None else learning_rate, momentum=momentum,
                                    nesterov=nesterov, name=name, **kwargs)

    class LAMB(_Optimizer):
        """tfa.optimizers.LAMB (You et al. 2019) as this project restates it (parity unpinned: TensorFlow
        Addons is not installed): layer-wise adaptive Adam for large batches.  Per trainable variable, t = iterations + 1:
            m <- beta_1*m + (1 - beta_1)*g;  v <- beta_2*v + (1 - beta_2)*g*g
            u  = (m / (1 - beta_1^t)) / (sqrt(v / (1 - beta_2^t)) + epsilon), + weight_decay_rate*w on a decayed variable
            r  = ||w|| / ||u|| when both norms are > 0, else 1;  1 for a variable excluded from layer adaptation
            w <- w - (r*lr_t)*u
        (csrc/lamb.hip: two passes and a per-variable reduction in between; include/lisec_hip.h has the arithmetic).
        exclude_from_weight_decay / exclude_from_layer_adaptation: the variables that are not decayed / whose ratio is
        not used -- ParamStore names and / or the kinds 'kernel', 'bias', 'gamma', 'beta', as AdamW's decay_var_list
        takes them; tfa takes regular expressions on TF variable names, which do not exist here.  As in tfa,
        exclude_from_layer_adaptation=None means the list of exclude_from_weight_decay.  lr=, decay= and the clipping
        keywords behave as in Adam (clipping is refused).  The slots are m and v; LisecNet.trust_ratios() returns r of
        the last update.  ValueError: beta_1 or beta_2 outside [0, 1), a negative epsilon or weight_decay_rate, a list
        that is not made of strings."""

        def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-6, weight_decay_rate=0.0,
                     exclude_from_weight_decay=None, exclude_from_layer_adaptation=None, name="LAMB", lr=None,
                     decay=0.0, **kwargs):
            for key, value in (("exclude_from_weight_decay", exclude_from_weight_decay),
                               ("exclude_from_layer_adaptation", exclude_from_layer_adaptation)):
                if value is not None:
                    value = [value] if isinstance(value, str) else list(value)
                setattr(self, key, value)
            self._set(name, lr if lr is not None else learning_rate, decay, kwargs, weight_decay_rate=weight_decay_rate,
                      beta_1=beta_1, beta_2=beta_2, epsilon=epsilon)

        def get_config(self):
            """tfa's keys in tfa's order: weight_decay_rate sits between learning_rate and decay."""
            return {"name": self.name, "learning_rate": _serialize_rate(self.lr),
                    "weight_decay_rate": self.weight_decay_rate, "decay": self.decay, "beta_1": self.beta_1,
                    "beta_2": self.beta_2, "epsilon": self.epsilon, **self.lists, **self._clip_config()}

    _DECOUPLED = {SGD: SGDW, Adam: AdamW}       # base class -> its class with decoupled weight decay, made once

    @staticmethod
    def extend_with_decoupled_weight_decay(base_class):
        """tfa.optimizers.extend_with_decoupled_weight_decay: the class <Base>W of one of the seven optimizer classes
        above -- its first argument is weight_decay, the others are the base class's, plus the keyword decay_var_list
        (see AdamW).  AdamW and SGDW are the classes of Adam and SGD.  The same class object at every call.
        ValueError for anything but one of the seven."""
        made = optimizers._DECOUPLED.get(base_class)
        if made is not None:
            return made
        name = getattr(base_class, "__name__", None)
        if name not in optimizer_table.BY_CLASS or getattr(optimizers, name, None) is not base_class:
            raise ValueError(f"extend_with_decoupled_weight_decay takes one of the optimizer classes "
                             f"{', '.join(optimizer_table.BY_CLASS)}, not {base_class!r}")
        if optimizer_table.BY_CLASS[name].layerwise:
            raise ValueError(f"extend_with_decoupled_weight_decay({name}): {name} carries its own weight decay "
                             f"(weight_decay_rate)")

        def __init__(self, weight_decay, *args, decay_var_list=None, **kwargs):
            self._set_decay(weight_decay, decay_var_list)
            kwargs.setdefault("name", name + "W")
            base_class.__init__(self, *args, **kwargs)

        made = type(name + "W", (_DecoupledWeightDecay, base_class), {
            "__init__": __init__,
            "__doc__": f"{name} with decoupled weight decay: w <- w - wd_t*w directly in front of every update "
                       f"(optimizers.AdamW describes weight_decay and decay_var_list); the other arguments are {name}'s."})
        optimizers._DECOUPLED[base_class] = made
        return made

    class MovingAverage(_AveragingOptimizer):
        """tfa.optimizers.MovingAverage as this project restates it (parity unpinned): after every update
        average <- average - (average - w)*(1 - decay_s), decay_s = 0 before iteration start_step, then average_decay, or
        with dynamic_decay min(average_decay, (1 + k)/(10 + k)), k = iterations - start_step.  num_updates folds into
        average_decay once, here: min(average_decay, (1 + num_updates)/(10 + num_updates)).  Only the trainable
        variables are averaged, not the BatchNormalization moving statistics.  ValueError: wrapping a wrapper,
        sequential_update=False, average_decay outside [0, 1], start_step < 0 or not an integer."""

        _OWN = ("name", "average_decay", "num_updates", "start_step", "dynamic_decay", "sequential_update")

        def __init__(self, optimizer, sequential_update=True, average_decay=0.99, num_updates=None, start_step=0,
                     dynamic_decay=False, name="MovingAverage"):
            self._wrap(optimizer, name)
            if sequential_update is not True:
                raise ValueError("MovingAverage(sequential_update=False) is not implemented: the average is updated "
                                 "after the variables")
            if not 0.0 <= float(average_decay) <= 1.0:
                raise ValueError(f"average_decay must lie in [0, 1], not {average_decay!r}")
            self.sequential_update, self.average_decay = True, float(average_decay)
            self.num_updates = None if num_updates is None else _step_number("num_updates", num_updates)
            if self.num_updates is not None and self.num_updates < 0:
                raise ValueError(f"num_updates must be >= 0, not {num_updates}")
            self.start_step, self.dynamic_decay = _step_number("start_step", start_step), bool(dynamic_decay)
            self.average_spec()                  # the range checks, before any launch

        def average_spec(self):
            decay = self.average_decay
            if self.num_updates is not None:
                decay = min(decay, (1.0 + self.num_updates) / (10.0 + self.num_updates))
            return AverageSpec("ema", decay=decay, dynamic=self.dynamic_decay, start=self.start_step)

        def get_config(self):
            return {"name": self.name, "optimizer": self._nested(), "sequential_update": True,
                    "average_decay": self.average_decay, "num_updates": self.num_updates, "start_step": self.start_step,
                    "dynamic_decay": self.dynamic_decay}

    class SWA(_AveragingOptimizer):
        """tfa.optimizers.SWA as this project restates it (parity unpinned): at the iterations
        start_averaging + m*average_period, m = 0, 1, ..., average <- (average*m + w)/(m + 1) on the variables after that
        update (m = 0: average <- w); at every other iteration the average keeps its bits.  ValueError: wrapping a
        wrapper, start_averaging < 0, average_period < 1, either not an integer."""

        _OWN = ("name", "start_averaging", "average_period")

        def __init__(self, optimizer, start_averaging=0, average_period=10, name="SWA"):
            self._wrap(optimizer, name)
            self.start_averaging = _step_number("start_averaging", start_averaging)
            self.average_period = _step_number("average_period", average_period)
            self.average_spec()                  # the range checks, before any launch

        def average_spec(self):
            return AverageSpec("swa", start=self.start_averaging, period=self.average_period)

        def get_config(self):
            return {"name": self.name, "optimizer": self._nested(), "start_averaging": self.start_averaging,
                    "average_period": self.average_period}

    WRAPPERS = ("MovingAverage", "SWA")

    @staticmethod
    def serialize(optimizer):
        """{"class_name", "config"} of an optimizer object; a wrapper nests the wrapped optimizer's under "optimizer"."""
        return {"class_name": type(optimizer).__name__, "config": optimizer.get_config()}

    @staticmethod
    def deserialize(config):
        """The optimizer of a {"class_name", "config"} dict (optimizers.serialize, or a checkpoint's optimizer_config).
        ValueError, naming the class, for one that is not implemented."""
        cls, c = config.get("class_name"), dict(config.get("config", {}))
        if cls in optimizers.WRAPPERS:
            inner = optimizers.deserialize(c.pop("optimizer"))       # (the clipping keys travel in the nested config)
            return getattr(optimizers, cls)(inner, **c)
        clip = {k: c.get(k) for k in _CLIP_KINDS}
        return optimizers.clip_gradients(optimizers._deserialize_plain(cls, c), **clip)

    @staticmethod
    def _deserialize_plain(cls, c):
        """deserialize's optimizer of class `cls` from the config dict c, before its clipping keys are applied."""
        base = optimizer_table.base_class(cls)   # <Base>W: <Base> with decoupled weight decay
        rec = optimizer_table.BY_CLASS.get(base)
        if rec is None:
            raise ValueError(f"optimizer class {cls!r} is not implemented")
        lr = c.get("learning_rate", c.get("lr", rec.lr))
        if isinstance(lr, dict):
            lr = lr_schedules.deserialize(lr)
        given = dict(learning_rate=lr, decay=c.get("decay", rec.decay), name=c.get("name", cls),
                     **{h.name: c.get(h.name, h.default) for h in rec.hyper}, **{k: c.get(k) for k in rec.lists})
        if base == cls:
            return getattr(optimizers, cls)(**given)
        wd = c.get("weight_decay", 0.0)
        if isinstance(wd, dict):
            wd = lr_schedules.deserialize(wd)
        return optimizers.extend_with_decoupled_weight_decay(getattr(optimizers, base))(
            wd, decay_var_list=c.get("decay_var_list"), **given)

    @staticmethod
    def clip_gradients(optimizer, clipnorm=None, clipvalue=None, global_clipnorm=None):
        """Gradient clipping as tf.keras 2.4 defines it, in this project's restatement (parity unpinned), on
        an optimizer object or one of the strings optimizers.get takes; returns the optimizer object, with the
        attributes of the same names set (on a MovingAverage / SWA wrapper: the wrapped optimizer's).
            clipvalue=c         every gradient element is clamped to [-c, c]
            clipnorm=c          every variable's gradient is scaled so that its L2 norm is at most c
            global_clipnorm=c   the whole gradient is scaled so that its L2 norm over all trainable variables is at most c
        The clipped gradient is the regularised one (Keras' penalty sits in the tape) of the whole mini-batch, behind
        the data-parallel average; a decoupled weight decay and LAMB's own act on the variable and are not clipped
        (csrc/grad_clip.hip; include/lisec_hip.h has the arithmetic).  All three None clears the clipping.
        ValueError: more than one threshold at once -- tf.keras 2.4 takes clipvalue beside a norm, this does not --, or
        a threshold that is not a finite number > 0, finite in float32 (a bool is refused).  The constructor keywords
        of the same names stay refused (NotImplementedError)."""
        optimizer = optimizers.get(optimizer)
        _clip_spec(clipnorm, clipvalue, global_clipnorm)                # every refusal, before anything is assigned
        for key, value in (("clipnorm", clipnorm), ("clipvalue", clipvalue), ("global_clipnorm", global_clipnorm)):
            setattr(optimizer, key, None if value is None else float(value))
        return optimizer

    @staticmethod
    def get(identifier):
        """compile(optimizer='sgd' | 'adam') -> the optimizer with Keras' defaults; an optimizer object is returned as is."""
        if isinstance(identifier, _Optimizer):
            return identifier
        if isinstance(identifier, str):
            kinds = {"sgd": optimizers.SGD, "adam": optimizers.Adam}
            if identifier.lower() in kinds:
                return kinds[identifier.lower()]()
        raise ValueError(f"unsupported optimizer {identifier!r}: an optimizer object (optimizers.SGD, Adam, RMSprop, "
                         f"Adagrad, Adadelta, Adamax, Nadam) or the string 'sgd' or 'adam' -- pass the others as "
                         f"objects, e.g. optimizers.RMSprop()")


class History:
    def __init__(self):
        self.history = {}


_LOSS_NAMES = ("loss", "ClassificationLayer_loss", "RegressionLayer_loss")


def _validation_split_at(n, validation_split):
    """Keras 2.4 fit(validation_split=f): the first floor(n * (1 - f)) sweeps train, the tail validates (taken before
    any shuffling).  ValueError for f outside (0, 1) or a split that leaves either part empty."""
    f = float(validation_split)
    if not 0.0 < f < 1.0:
        raise ValueError(f"validation_split must lie in (0, 1), got {validation_split}")
    split_at = int(math.floor(n * (1.0 - f)))
    if split_at == 0 or split_at == n:
        raise ValueError(f"Training data contains {n} samples, which is not sufficient to split it into a validation and "
                         f"training set as specified by `validation_split={validation_split}`. Either provide more data, "
                         f"or a different value for the `validation_split` argument.")
    return split_at


def _should_validate(epoch, validation_freq):
    """Keras 2.4: an int validates when (epoch + 1) % validation_freq == 0, a container (list, set, range, ...) on the
    1-based epochs it holds."""
    if isinstance(validation_freq, bool):
        raise ValueError(f"Expected `validation_freq` to be a list or int. Received: validation_freq={validation_freq!r}")
    if isinstance(validation_freq, numbers.Integral):
        if validation_freq < 1:
            raise ValueError("`validation_freq` can not be less than 1.")
        return (epoch + 1) % int(validation_freq) == 0
    if isinstance(validation_freq, collections.abc.Container) and not isinstance(validation_freq, (str, bytes)):
        return epoch + 1 in validation_freq
    raise ValueError(f"Expected `validation_freq` to be a list or int. Received: validation_freq={validation_freq!r}")


def _check_batch_size(batch_size):
    """fit(batch_size=): an integer >= 1 (numpy integers included), returned as an int.  Anything else -- a bool, as
    boxes._count refuses it, a float, a string, 0 or a negative number -- is a ValueError."""
    if isinstance(batch_size, bool) or not isinstance(batch_size, numbers.Integral) or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size!r}")
    return int(batch_size)


def _epoch_batches(n, batch_size, steps_per_epoch=None):
    """The batches of one epoch over an order of n sweeps, as lists of positions into that order; one update each.
    steps_per_epoch=None: ceil(n / B) batches, batch k = positions k*B .. (k+1)*B - 1, the last one possibly shorter.
    steps_per_epoch given: that many batches of B sweeps each, sweep j of batch k at position (k*B + j) % n -- the
    wrap-around of the batch-1 loop."""
    B = batch_size
    if steps_per_epoch is None:
        return [list(range(k, min(k + B, n))) for k in range(0, n, B)]
    if n < 1:
        raise ValueError("no sweeps to train on")
    return [[(k * B + j) % n for j in range(B)] for k in range(int(steps_per_epoch))]


def _add_sweep_logs(tot, loss_out, b, last, penalty=None):
    """Adds one sweep's [total, class, regression] (loss_out) to the epoch sums `tot` (float64; numpy arrays or device
    tensors alike) so that tot / sweeps is Keras' batch-size-weighted epoch mean.  A batch's `loss` is the mean of its b
    sweeps' losses plus the weight penalty P once, and weighs b in the epoch mean: b*P in the sums.  The step that ends
    a batch (`last`) has folded P into its own total once; the other b - 1 shares are added here, from `penalty` (the
    float64[1] P of that update; None without regularizers)."""
    tot[:3] += loss_out
    if last and penalty is not None and b > 1:
        tot[0] += (b - 1) * penalty[0]
    return tot


def _grid_key(samples):
    """The voxel grid every sample shares, when each is a voxelised sweep that still holds its device points; else None
    (e.g. dense arrays turned into samples: no point cloud to voxelise again)."""
    pts = [getattr(s, "_keepalive", None) for s in samples]
    if not samples or any(p is None or not p.is_cuda for p in pts):
        return None
    keys = {(c.xSize, c.ySize, c.zSize, c.sampleSize, c.maxVoxelX, c.maxVoxelY, c.maxVoxelZ)
            for c in (s.cfg for s in samples)}
    return keys.pop() if len(keys) == 1 else None


def _reusable(cached, key, need):
    """The step of a cached (key, step) when it serves the request.  Otherwise it is closed: another grid / loss /
    optimizer / network, a larger sweep, or an eager call since (predict() on a larger sweep, a second model)
    reallocated a workspace the plan holds the raw address of."""
    if cached is None:
        return None
    if cached[0] == key and cached[1].capacity >= need and cached[1].alloc_gen == _lib.alloc_generation():
        return cached[1]
    cached[1].close()
    return None


def _targets(ycls, yreg, rows, dev):
    """target(i) -> the device (y_cls, y_reg) of label map i, for the i of `rows` (a range).  Those maps live on the
    device for the whole call when they fit comfortably (1.28 MB per sample); otherwise each is uploaded when asked for."""
    upload = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    if len(rows) * ycls[0].size * 4 * 8 < (2 << 30):
        maps = slice(rows.start, rows.stop, rows.step)
        ycls_d, yreg_d = upload(ycls[maps]), upload(yreg[maps])
        return lambda i, at=rows.index: (ycls_d[at(i)], yreg_d[at(i)])
    return lambda i: (upload(ycls[i]), upload(yreg[i]))


def _sample_weight_arrays(sample_weight, n, grid, what="sample_weight"):
    """fit / evaluate's sample_weight -> None, or [w_cls, w_reg], each None (that output has weight 1) or a float32 array
    of at least n rows: (rows,) -- one weight per sweep -- or (rows, Ho, Wo) -- one per cell of the output grid.  One
    array serves both outputs, a list or tuple holds one entry per output, a dict is keyed by output name; None entries
    are allowed.  ValueError: another shape, fewer rows than samples, a value that is not finite, a list of another
    length, an unknown output name."""
    if sample_weight is None:
        return None
    if isinstance(sample_weight, (dict, list, tuple)):
        per = losses._per_output(sample_weight, what)
    else:
        per = [sample_weight, sample_weight]
    out = []
    for name, w in zip(losses.OUTPUTS, per):
        if w is None:
            out.append(None)
            continue
        try:
            a = np.asarray(w, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError(f"{what} for {name} is not an array of numbers") from None
        if a.ndim not in (1, 3) or (a.ndim == 3 and tuple(a.shape[1:]) != tuple(grid)):
            raise ValueError(f"{what} for {name} must have the shape (n,) or (n, {grid[0]}, {grid[1]}), got {a.shape}")
        if a.shape[0] < n:
            raise ValueError(f"{what} for {name} has {a.shape[0]} rows for {n} samples")
        if not np.isfinite(a[:n]).all():
            raise ValueError(f"{what} for {name} holds a value that is not finite")
        out.append(a)
    return None if all(a is None for a in out) else out


def _refuse_empty_sample_weight(sample_weight):
    """A sample_weight array without a single row weighs no sweep: the weighted losses would be means over nothing and
    every weighted metric 0/0.  NotImplementedError, raised by evaluate() and fit() in front of everything else they do
    with their data; None, and None entries, pass."""
    if sample_weight is None:
        return
    if isinstance(sample_weight, dict):
        entries = list(sample_weight.values())
    elif isinstance(sample_weight, (list, tuple)):
        entries = list(sample_weight)
    else:
        entries = [sample_weight]
    for w in entries:
        if w is not None and np.size(w) == 0:
            raise NotImplementedError("a sample_weight array without any row is not implemented: pass sample_weight=None "
                                      "to evaluate or fit without weights")


def _weight_form(sw):
    """network.weight_form of _sample_weight_arrays' result: None, or per output None / 'sweep' / 'cell'."""
    if sw is None:
        return None
    return tuple(None if a is None else ("sweep" if a.ndim == 1 else "cell") for a in sw)


def _weights_at(sw, rows, dev):
    """weight(i) -> the device sample weights of sample i, for the i of `rows` (a range): a pair of float32 tensors,
    (1,) or (Ho, Wo), or None per output; the arrays live on the device for the whole call (80 KB per Lyft-grid map)."""
    if sw is None:
        return None
    maps = slice(rows.start, rows.stop, rows.step)
    up = [None if a is None else torch.from_numpy(np.ascontiguousarray(a[maps])).to(dev) for a in sw]

    def weight(i, at=rows.index):
        k = at(i)
        return tuple(None if u is None else (u[k:k + 1] if u.dim() == 1 else u[k]) for u in up)
    return weight


def _item_weights(w, grid, dev=None):
    """The sample weights of ONE sweep, as a Sequence item brings them (its third element): _sample_weight_arrays' forms
    without the leading axis -- a number or an (Ho, Wo) map per output.  -> None, or a pair of float32 arrays / None of
    the shapes (1,) and (Ho, Wo) (device tensors with `dev`)."""
    if w is None:
        return None
    if isinstance(w, (dict, list, tuple)):
        per = losses._per_output(w, "sample_weight")
    else:
        per = [w, w]
    rows = [None if a is None else np.asarray(a, dtype=np.float32)[None] for a in per]
    rows = [a.reshape(1) if a is not None and a.size == 1 else a for a in rows]
    sw = _sample_weight_arrays(rows, 1, grid, "a Sequence item's sample_weight")
    if sw is None:
        return None
    out = tuple(None if a is None else np.ascontiguousarray(a[0] if a.ndim == 3 else a[:1]) for a in sw)
    if dev is None:
        return out
    return tuple(None if a is None else torch.from_numpy(a).to(dev) for a in out)


def _is_sequence(x):
    """keras.utils.Sequence by its interface; lists, arrays and voxelised sweeps are not."""
    return (not isinstance(x, (list, tuple, np.ndarray)) and all(callable(getattr(x, m, None))
            for m in ("__getitem__", "__len__", "on_epoch_end")))


def _refuse_mixed_training(policy):
    if policy.compute_dtype != "float32":
        raise NotImplementedError(
            f"training under the '{policy.name}' policy is not implemented: it serves predict() and evaluate(); "
            "build the model under 'float32' to fit() it")


class Model:
    """What createModel returns: the subset of the keras.Model interface the reference uses."""

    def __init__(self, nx, ny, nz, maxPoints, params=None, kernel_regularizer=None, bias_regularizer=None,
                 gamma_regularizer=None, beta_regularizer=None, activity_regularizer=None, variable_regularizers=None):
        """<kind>_regularizer: anything regularizers.get accepts (None, regularizers.l2(1e-4), 'l2', a {"class_name",
        "config"} dict), applied to every variable of that kind in params.param_specs() -- what passing it to every layer
        of the reference's createModel does.  variable_regularizers: {ParamStore name: (l1, l2)}, the per-variable form
        (what load_model reads from a file whose layers differ); it overrides the per-kind one for the variables it
        names.  The model keeps the merged dict as self.regularizers (pairs other than (0, 0) only).  The penalty is part of `loss`
        (not of the per-output losses, not scaled by loss_weights) in fit, evaluate and val_loss.
        activity_regularizer: NotImplementedError."""
        if activity_regularizer is not None:
            raise NotImplementedError("activity_regularizer is not implemented: only the weights can be penalised")
        self.nx, self.ny, self.nz, self.maxPoints = nx, ny, nz, maxPoints
        coeffs = regularizers.coefficients(param_specs(fold_depth(nz)), kernel=kernel_regularizer, bias=bias_regularizer,
                                           gamma=gamma_regularizer, beta=beta_regularizer)
        for name, (a, b) in (variable_regularizers or {}).items():
            coeffs[name] = regularizers.L1L2(a, b).pair()
        self.regularizers = {n: p for n, p in coeffs.items() if p != (0.0, 0.0)}
        # tf.keras.mixed_precision: the global policy in force NOW, fixed for the model's life (mixed_precision.py)
        self.dtype_policy = mixed_precision.global_policy()
        self.net = LisecNet(nx, ny, nz, maxPoints, params=params, compute_dtype=self.dtype_policy.compute_dtype,
                            regularizers=self.regularizers)
        self.optimizer, self.loss = None, None
        self._metric_names = []             # "<output>_<metric>" in compile order
        self._compile_args = None           # compile()'s loss / loss_weights / metrics, unless they are the reference's
        self._captured = self._eval_captured = None     # (key, step) of the recorded training / evaluation plan
        self.dp = None
        self.stop_training = False          # set by a callback (EarlyStopping): fit ends after the epoch
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            from .parallel import DataParallel
            self.dp = DataParallel(self.net.device)
            self.dp.broadcast_(self.net.params.theta)
            self.dp.broadcast_(self.net.params.state)
            self.net.params.touch()

    # -- compile / fit / predict / save ------------------------------------------------------------
    def compile(self, optimizer, loss, metrics=None, loss_weights=None, weighted_metrics=None):
        """compile(optimizer=sgd, loss=['mse','mse']) (model_training.py:296); optimizer: optimizers.SGD / optimizers.Adam
        or the string 'sgd' / 'adam'.  A fresh optimizer discards every slot (momentum accumulators, Adam moments) and the
        iteration count, as re-compiling does in the reference (:339-340).
        loss: a tf.keras 2.4 loss (a name or a losses.* object; see lisec_amd/losses.py) for both outputs, a list of two in
        output order or a dict keyed by 'ClassificationLayer' / 'RegressionLayer'; also the project's 'smoothl1_ce' (=
        ['cross_entropy', 'smooth_l1']: sigmoid cross-entropy on labels clamped to [0, 1] + SmoothL1), or -- as the whole
        argument only -- losses.VoxelNetLoss(...) / 'voxelnet', the detection loss the 0/1/2 label code was made for, or
        losses.VoxelNetIoULoss(...) / 'voxelnet_iou', the same with a rotated-box IoU term in its regression part (one
        loss of both outputs; loss_weights apply; metrics: the detection metrics of lisec_amd/metrics.py -- 'anchor_precision',
        'anchor_recall', 'anchor_accuracy', 'positive_mae', 'positive_iou' or their objects -- and only those, a flat list
        routing each to the output it belongs to, unlike Keras).  loss_weights: a list
        or dict of floats (default 1): the step minimises w_c*L_c + w_r*L_r, History's `loss`; the per-output losses are
        logged unweighted.  metrics: a list (for each output), a list of two lists or a dict per output name; logged as
        "<output>_<name>" (see metrics_names).  weighted_metrics: the Keras metrics in the forms metrics= takes, logged
        behind their output's metrics as "<output>_weighted_<name>": under fit / evaluate(sample_weight=) each is
        sum w*v / sum w pooled over the epoch's or evaluation's sweeps (0.0 when the weights sum to 0), without sample
        weights the unweighted metric; the two lists share the cap of 4 per output; with a VoxelNet loss
        NotImplementedError.
        Every refusal (ValueError, NotImplementedError) is raised here, before any launch."""
        optimizer = optimizers.get(optimizer)
        wd = optimizer.decay_spec()
        if wd is not None:
            # a decay_var_list this network cannot serve: KeyError for an unknown name, ValueError for a variable
            # that is not trainable (ops.decay_chunks)
            self.net.decay_table(wd.variables)
        if optimizer.record.layerwise:
            # exclusion lists this network cannot serve are refused here in the same way (ops.lamb_chunks); the tables,
            # the workspace and the ratio buffer get their fixed addresses before any step is recorded
            self.net.lamb_table(*optimizer.spec().lists)
        step_loss, names = losses.compile_weighted_loss(loss, loss_weights, metrics, weighted_metrics)
        self.optimizer, self.loss = optimizer, step_loss
        self._metric_names = names
        # the arguments as given, for the training_config of save() (a legacy step records today's ['mse','mse'])
        self._compile_args = None if isinstance(step_loss, str) else dict(loss=loss, loss_weights=loss_weights,
                                                                         metrics=metrics)
        if self._compile_args is not None and weighted_metrics is not None:
            self._compile_args["weighted_metrics"] = weighted_metrics
        self.net._prepare_training()
        spec, start = optimizer.spec(), optimizer.record.slot_start
        for name in spec.slots:
            self.net.slot(name)
        for t in self.net.slots().values():
            t.zero_()
        if start is not None:                    # Adagrad's accumulators start at initial_accumulator_value
            for name in spec.slots:
                self.net.slot(name).fill_(getattr(optimizer, start))
        self.net.momentum_cache.fill_(1.0)
        self.net.iterations = 0
        self.net.restart_average()               # a fresh averaging wrapper starts from the variables as they then are

    @contextlib.contextmanager
    def average_weights(self, update_bn=None, statistics="mean"):
        """with model.average_weights(): ... -- inside the block the variables ARE their averages (theta <-> average by
        content, LisecNet.swap_average): predict, evaluate and save see the averaged model, with the BatchNormalization
        moving statistics as they stand.  On leaving, also by an exception, they are swapped back: theta, the average
        and every later step are bit for bit those of a run that never entered.  Do not train inside the block.
        update_bn=x (what recalibrate_batch_norm takes; `statistics` its rule): the moving statistics are recalibrated
        for the averages over x before the block runs (torch.optim.swa_utils.update_bn) and put back, bit for bit, on
        leaving -- also when the recalibration itself or the block raises.  None: the method does what it always did.
        ValueError on a model whose optimizer is not optimizers.MovingAverage / SWA, or for an unknown `statistics`."""
        if not isinstance(self.optimizer, _AveragingOptimizer):
            raise ValueError("average_weights() needs a model compiled with optimizers.MovingAverage or optimizers.SWA")
        if update_bn is None:
            self.net.swap_average()
            try:
                yield self
            finally:
                self.net.swap_average()
            return
        ops.bn_statistics(statistics)
        net = self.net
        net.swap_average()
        try:
            own = net.params.state.clone()
            try:
                self.recalibrate_batch_norm(update_bn, statistics=statistics)
                yield self
            finally:
                net.params.state.copy_(own)
                net.state_version += 1
        finally:
            net.swap_average()

    def recalibrate_batch_norm(self, x, steps=None, statistics="mean"):
        """Replaces the BatchNormalization moving statistics by statistics of the current variables over the sweeps of
        x (LisecNet.recalibrate_batchnorm): 'mean' -- torch.optim.swa_utils.update_bn with momentum=None --, or 'pooled'
        ("precise BN": plus the variance of the sweeps' means).  x: anything predict takes, or a Sequence as fit(x=...)
        takes one (its labels are ignored; an augmenting Sequence is read at its current epoch); steps: at most that
        many sweeps, from the front.  Data parallel: the sweeps are shared out over the ranks and every rank ends with
        the same statistics.  Changes no variable, optimizer slot, iteration count or weight average; a recorded
        training step stays valid for sweeps no larger than the training sweeps.  ValueError: no sweep, an unknown
        `statistics`."""
        ops.bn_statistics(statistics)
        if _is_sequence(x):
            n = len(x) if steps is None else min(len(x), int(steps))
            rank, world = (0, 1) if self.dp is None else (self.dp.rank, self.dp.world)
            # only this rank's share is voxelised; the others' places are never read (samples[rank::world])
            samples = [self._sequence_item(x, i, False)[0] if i % world == rank else None for i in range(n)]
        else:
            samples = self._as_samples(x)
            if steps is not None:
                samples = samples[:int(steps)]
        self.net.recalibrate_batchnorm(samples, statistics=statistics, dp=self.dp)

    @property
    def metrics_names(self):
        """['loss', 'ClassificationLayer_loss', 'RegressionLayer_loss', <"<output>_<metric>" in compile order>]: the keys of
        History and of evaluate(return_dict=True), the order of evaluate()'s list.  Unlike Keras, which fills it after the
        first batch, it is set by compile() ([] before)."""
        if self.optimizer is None:
            return []
        return list(_LOSS_NAMES) + list(self._metric_names)

    def _as_samples(self, x):
        if isinstance(x, SparseVoxels):
            return [x.sample]
        if isinstance(x, VoxelSample):
            return [x]
        if isinstance(x, (list, tuple)):
            return [s for item in x for s in self._as_samples(item)]
        arr = np.asarray(x)
        if arr.ndim == 5:
            arr = arr[None]
        if arr.ndim != 6:
            raise ValueError("expected SparseVoxels / list of them / dense (n,D,H,W,T,6) array")
        return [dense_to_sample(a, self.net.device) for a in arr]

    def fit(self, x, y=None, batch_size=1, verbose=1, epochs=1, steps_per_epoch=None, shuffle=True, callbacks=None,
            validation_split=0.0, validation_data=None, validation_steps=None, validation_freq=1, sample_weight=None,
            class_weight=None):
        """fit(x=trainPoints, y=[outClass, outRegress], batch_size=1, epochs=1, steps_per_epoch=180)
        (model_training.py:299).  batch_size=B (an integer >= 1; anything else is a ValueError before any launch): every
        update is made with the mean gradient of B sweeps, each run at batch 1 -- BatchNormalization statistics and
        moving averages stay per sweep, the loss is normalised per sweep and then averaged: Keras' MirroredStrategy over
        B replicas at per-replica batch 1 without SyncBatchNorm, NOT one replica's batch of B with pooled statistics
        (INTEGRATION.md).  An epoch is ceil(n / B) updates over order[k*B : (k+1)*B] (the last batch may be shorter and is
        divided by its own size); steps_per_epoch counts updates of B sweeps, sweep j of batch k being
        order[(k*B + j) % n].  iterations, learning-rate schedules and decay count updates.  The epoch logs are Keras'
        batch-size-weighted means: sums over sweeps divided by the sweeps trained on, a batch's weight penalty weighted
        by its size.  batch_size=1 is the reference's setting and the step as it always was.
        With WORLD_SIZE > 1 whole samples are sharded over the ranks, each rank forms its batches from its own shard
        (global batch B * world) and the gradients are averaged with one exchange per update.
        callbacks: a list of callbacks.Callback (LearningRateScheduler, or one's own), called as Keras does.  With
        callbacks the update kernels read the learning rate from the device descriptor, so that a rate set between
        epochs reaches the recorded step without recording it again.
        validation_data=(x_val, [y_cls, y_reg]), or validation_split=f (the last floor-split fraction of x / y, taken
        before shuffling; validation_data takes precedence): after the steps of an epoch that validation_freq selects (an
        int: every validation_freq-th epoch; a container: those 1-based epochs), evaluate() runs on the validation sweeps
        (validation_steps of them at most) with on_test_begin / on_test_end, and val_loss, val_ClassificationLayer_loss and
        val_RegressionLayer_loss join the logs of on_epoch_end and History.  The metrics of compile() are logged as epoch
        means under metrics_names, and with validation as val_<name>; the detection metrics as the ratio of their two sums
        pooled over the epoch's sweeps, summed on the device in float64 and divided once.  fit ends after any epoch whose callbacks set
        model.stop_training.
        x may be a keras.utils.Sequence-like object (__len__, __getitem__(i) -> (points (n, >= 3), [y_cls, y_reg]),
        on_epoch_end()), e.g. augment.AugmentedSweeps, with y=None: step st trains on item order[st], made when the step
        stages its sweep, and on_epoch_end() is called after every epoch.  y given with it is a ValueError, as in Keras;
        validation_split is refused (pass validation_data).  Everything else works as for lists.
        sample_weight: one array for both outputs, a list of two or a dict by output name (None entries allowed), each
        (n,) -- a weight per sweep -- or (n, Ho, Wo) -- a weight per cell of the output grid: every sweep's loss is
        1/(M*C) sum_m w[m] sum_c v(m,c) per output (the divisor stays the element count: Keras' SUM_OVER_BATCH_SIZE at
        batch 1), for a VoxelNet loss the weighted sums over its positives and negatives with the unweighted counts; the
        weights are applied inside the loss pass on the device (lisec_*_loss_weighted).  An epoch's `loss` stays the
        mean of the sweeps' weighted losses and batch_size=B divides by B; metrics= stay unweighted, weighted_metrics= are
        sum w*v / sum w pooled over the epoch.  An array without any row is NotImplementedError.  validation_split splits the weights with the labels, validation_data
        may be (x, y, sample_weight), a Sequence item may be (points, [y_cls, y_reg], sample_weight) with a number or an
        (Ho, Wo) map per output -- every item in the form of item 0 --, and sample_weight= together with a Sequence is a
        ValueError, as in Keras.  Another shape, fewer rows than samples or a value that is not finite: ValueError before
        any launch.  class_weight: ValueError unless None (Keras supports it for single-output models only)."""
        B = _check_batch_size(batch_size)        # first of all: nothing of the model or the GPU is touched before it
        _refuse_mixed_training(self.dtype_policy)
        if self.optimizer is None:
            raise RuntimeError("compile() the model first")
        if class_weight is not None:
            raise ValueError("`class_weight` is only supported for Models with a single output.")
        _refuse_empty_sample_weight(sample_weight)
        if validation_data is not None and len(validation_data) > 2:
            _refuse_empty_sample_weight(validation_data[2])
        grid = (self.net.Ho, self.net.Wo)
        seq = x if _is_sequence(x) else None
        if seq is not None:
            if y is not None:
                raise ValueError("`y` argument is not supported when using `keras.utils.Sequence` as input.")
            if sample_weight is not None:
                raise ValueError("`sample_weight` argument is not supported when using `keras.utils.Sequence` as input.")
            if validation_split:
                raise ValueError("`validation_split` is only supported for lists and arrays: pass validation_data")
            samples, ycls, yreg, n = None, None, None, len(seq)
        else:
            if y is None:
                raise ValueError("y=[outClass, outRegress] is required unless x is a Sequence")
            samples = self._as_samples(x)
            ycls = np.asarray(y[0], dtype=np.float32)
            yreg = np.asarray(y[1], dtype=np.float32)
            n = len(samples)
            if len(ycls) < n or len(yreg) < n:
                raise ValueError("fewer label maps than samples")
        sw = None if seq is not None else _sample_weight_arrays(sample_weight, n, grid)
        val = None
        if validation_data is not None:
            val_samples = self._as_samples(validation_data[0])
            val_y = validation_data[1]
            val_w = validation_data[2] if len(validation_data) > 2 else None
        elif validation_split:
            at = _validation_split_at(n, validation_split)
            val_samples, val_y = samples[at:], (ycls[at:n], yreg[at:n])
            val_w = None if sw is None else [None if a is None else a[at:n] for a in sw]
            samples, n = samples[:at], at
        if validation_data is not None or validation_split:
            vn = len(val_samples) if validation_steps is None else min(len(val_samples), int(validation_steps) * B)
            val = (val_samples[:vn],) + self._labels(val_y, vn) + (_sample_weight_arrays(val_w, vn, grid,
                                                                                        "validation sample_weight"),)
            _should_validate(0, validation_freq)           # a malformed validation_freq is refused before any step
        if seq is not None and not hasattr(seq, "staged") and len(seq):
            # a Sequence of (points, labels, sample_weight) items: item 0 says in which form every item brings its weights
            first = seq[0]
            wform = weight_form(_item_weights(first[2], grid, dev=self.net.device) if len(first) > 2 else None)
        else:
            wform = _weight_form(sw)
        weighted = wform is not None
        self.stop_training = False
        idx = list(range(n))
        if self.dp is not None:
            idx = self.dp.shard(idx)
        steps = steps_per_epoch if steps_per_epoch is not None else -(-len(idx) // B)     # updates per epoch
        if self.dp is not None and steps_per_epoch is not None:
            steps = max(1, steps_per_epoch // self.dp.world)
        batches = _epoch_batches(len(idx), B, None if steps_per_epoch is None else steps)
        sweeps = sum(len(b) for b in batches)               # sweeps trained on per epoch
        dev = self.net.device
        hist = History()
        callbacks = list(callbacks or [])
        for cb in callbacks:
            cb.set_model(self)
            cb.set_params(dict(verbose=verbose, epochs=epochs, steps=steps))
        target = _targets(ycls, yreg, range(n), dev) if seq is None else None
        weight = _weights_at(sw, range(n), dev)
        seq_req = self._sequence_request(seq) if seq is not None else None
        nm = loss_acc_len(self.loss, weighted) - 4          # metric words of the compiled loss (loss_acc_len's layout)
        for cb in callbacks:
            cb.on_train_begin()
        for epoch in range(epochs):
            for cb in callbacks:
                cb.on_epoch_begin(epoch, {})
            opt = self.optimizer.spec(device_lr=bool(callbacks))
            if opt.average is not None:
                self.net.average                 # started from the variables as they are now, if compile() asked for it
            # the same plan every epoch (a rate from the descriptor is not part of its key); a new rate is copied into
            # the descriptor on this stream, behind the previous epoch's last update
            captured = self._captured_step(samples, opt, seq_req, batch=B, wform=wform)
            self.net._sync_lr(opt)               # (and the coefficient of a decoupled weight decay)
            order = list(np.random.permutation(idx)) if shuffle else list(idx)
            # the running loss stays on the device: reading it back every step would stall the host behind the GPU and
            # expose the time it needs to enqueue the next step; the progress line is refreshed ~20 times per epoch
            tot_dev = torch.zeros(3, dtype=torch.float64, device=dev)
            met_dev = torch.zeros(nm, dtype=torch.float64, device=dev) if nm else None
            met_step = self.net.step_metrics(self.loss, weighted)     # where a step leaves its metric words, if any
            every = max(1, steps // 20)
            t0 = time.time()

            def sweep(t, points=captured is not None):
                """What sweep t of the epoch trains on: (points of the sweep for a recorded step, else its voxel sample,
                y_cls, y_reg, and under sample weights the sweep's).  The batches are consecutive runs of the order, so
                sweep t is order[t % n]."""
                i = int(order[t % len(order)])
                if seq is not None:
                    return self._sequence_item(seq, i, points, weighted)
                item = (samples[i]._keepalive if points else samples[i], *target(i))
                return item + (weight(i),) if weighted else item

            penalty = self.net.reg_penalty if self.net.regularized else None
            t = 0                                           # sweeps trained on so far in this epoch
            for st, batch in enumerate(batches):
                b = len(batch)
                if b > 1:
                    self.net.set_batch_divisor(b)           # the short last batch of an epoch is divided by its own size
                for position in LisecNet.batch_positions(b):
                    if captured is not None:
                        # the whole step (voxelise + forward + backward + update) re-issued from its recorded plan: one C
                        # call (PipelinedStep: it also voxelises the next sweep, on the second stream)
                        captured.fit_step(sweep, t, sweeps, position=position)
                    else:
                        item = sweep(t)
                        self.net.train_micro_step(*item[:3], position, loss=self.loss, opt=opt,
                                                  allreduce=self.dp.bucketed() if self.dp is not None else None,
                                                  weights=item[3] if weighted else None)
                    _add_sweep_logs(tot_dev, self.net.loss_out, b, position in ("single", "last"), penalty)
                    if nm:
                        met_dev += met_step
                    t += 1
                if verbose and ((st + 1) % every == 0 or st + 1 == steps):
                    print(f"\r{st + 1}/{steps} - loss: {float(tot_dev[0].item()) / t:.4f}", end="", flush=True)
            tot = tot_dev.cpu().numpy()
            if verbose:
                print(f" - {time.time() - t0:.1f}s")
            if nm:
                tot = np.concatenate([tot, met_dev.cpu().numpy()])
            logs = dict(zip(self.metrics_names, loss_acc_logs(self.loss, tot, max(sweeps, 1), weighted)))
            if val is not None and _should_validate(epoch, validation_freq):
                vlogs = self._evaluate(*val, callbacks=callbacks, verbose=0)
                logs.update({"val_" + key: v for key, v in vlogs.items()})
                if verbose:
                    print(" - ".join(f"val_{key}: {v:.4f}" for key, v in vlogs.items()))
            for cb in callbacks:
                cb.on_epoch_end(epoch, logs)
            for key, v in logs.items():
                hist.history.setdefault(key, []).append(v)
            if seq is not None:
                seq.on_epoch_end()
            if self.stop_training:
                break
        for cb in callbacks:
            cb.on_train_end()
        return hist

    def _sequence_grid(self):
        """The voxel grid of this model's input under the reference's voxel edges (what _preprocess voxelises with)."""
        return (float(Constants.voxelx), float(Constants.voxely), float(Constants.voxelz), int(self.maxPoints),
                self.nx // 2, self.ny // 2, self.nz)

    def _sequence_request(self, seq):
        """_plan_request for a Sequence of raw sweeps: the capacity is its largest row count (`max_points`; augmentation
        keeps the count, object sampling adds its bound), the point dtype its `dtype`; a Sequence without them is walked
        once to find them."""
        need, dtype = getattr(seq, "max_points", None), getattr(seq, "dtype", None)
        if need is None or dtype is None:
            pts = [torch.as_tensor(seq[i][0]) for i in range(len(seq))]
            need = max((int(p.shape[0]) for p in pts), default=0)
            dtype = torch.float64 if any(p.dtype == torch.float64 for p in pts) else torch.float32
        grid = self._sequence_grid()
        mode = _sequence_subsample(seq)
        key = (grid, dtype, self.loss, id(self.net), torch.cuda.current_stream().cuda_stream, self.net.compute_dtype, mode)
        return key, grid, dtype, int(need), max(1024, -(-int(need) // 4096) * 4096), mode

    def _sequence_item(self, seq, i, recorded, weighted=None):
        """What a step trains on when x is a Sequence: for a recorded step the item as something that stages itself into
        the step's buffers (AugmentedSweeps.staged) or its (points, y_cls, y_reg); for the Python schedule the voxelised
        sweep and its targets.  weighted=True: the item is (points, [y_cls, y_reg], sample_weight) and its weights come fourth
        (_item_weights; a step recorded for another form refuses them); False: an item that brings weights is refused;
        None: whatever weights it brings are ignored (recalibrate_batch_norm)."""
        if recorded and hasattr(seq, "staged"):
            return seq.staged(i), None, None
        item = seq[i]
        pts, (y_cls, y_reg) = item[0], item[1]
        w = ()
        if weighted:
            got = _item_weights(item[2] if len(item) > 2 else None, (self.net.Ho, self.net.Wo),
                                dev=None if recorded else self.net.device)
            if got is None:
                raise ValueError(f"item {i} of the Sequence brings no sample_weight, item 0 did")
            w = (got,)
        elif weighted is not None and len(item) > 2 and item[2] is not None:
            raise ValueError(f"item {i} of the Sequence brings a sample_weight, item 0 did not")
        if recorded:
            return (pts, y_cls, y_reg) + w
        dev = self.net.device
        draw = {}
        if _sequence_subsample(seq) == "random":       # the draw the recorded step's buffer set is given
            draw = dict(seed=seq.seed, item=i, epoch=seq.epoch)
        vox = VFE_preprocessing(pts, *self._sequence_grid(), **draw).sample
        return (vox, torch.as_tensor(y_cls, dtype=torch.float32).to(dev), torch.as_tensor(y_reg, dtype=torch.float32).to(dev)) + w

    def _plan_request(self, samples):
        """What a recorded plan for these samples takes: (cache key without the optimizer, the one voxel grid, point
        dtype, points of the largest sweep, point capacity to record); None when no plan applies (_grid_key)."""
        grid = _grid_key(samples)
        if grid is None:
            return None
        pts = [s._keepalive for s in samples]
        dtype = torch.float64 if any(p.dtype == torch.float64 for p in pts) else torch.float32
        need = max(int(p.shape[0]) for p in pts)
        key = (grid, dtype, self.loss, id(self.net), torch.cuda.current_stream().cuda_stream, self.net.compute_dtype)
        return key, grid, dtype, need, max(1024, -(-need // 4096) * 4096), "first"     # a little head-room for later calls

    def _captured_step(self, samples, opt, seq_req=None, batch=1, wform=None):
        """The recorded form of the step (lisec_amd.network.RecordedStep: the eager schedule re-issued by
        lisec_step_plan_run, one C call per step), when it applies: one GPU, every sample a voxelised sweep that still
        holds its device points, one grid (data parallel included: the gradient exchange is recorded with the step).
        Otherwise (None) the Python schedule issues every step."""
        req = None
        if _lib.knob("step_plan", True):
            req = self._plan_request(samples) if seq_req is None else seq_req
        if req is None:
            return None
        key, grid, dtype, need, capacity, mode = req
        # the full optimizer config: a re-compile with another optimizer records a new plan; the batch size: a fit with
        # another one records its own plans (those of a batch's micro-steps exist for batch_size > 1 only)
        # the form of the sample weights per output (none, one per sweep, one per cell): a weighted step records the
        # weighted loss launches and owns weight buffers; an unweighted one is keyed as it always was
        key += (opt.config, int(batch)) + (() if wform is None else (wform,))
        step = _reusable(self._captured, key, need)
        if step is None:
            cls = PipelinedStep if _lib.knob("pipeline_voxels", True) else RecordedStep
            step = cls(self.net, Voxelizer(*grid, device=self.net.device, subsample=mode), capacity, dtype=dtype, loss=self.loss,
                       opt=opt, allreduce=self.dp.bucketed() if self.dp is not None else None, batch=batch, wform=wform)
            self._captured = (key, step)
        return step

    def _eval_step(self, samples, wform=None):
        """The recorded evaluation sweep (lisec_amd.network.EvalStep: voxelise + forward(training=False) + eval loss, one
        C call per sweep) when it applies -- as for _captured_step: every sample a voxelised sweep that still holds its
        device points, one grid -- and LISEC_TUNING=eval_plan=1 asks for it.  Otherwise (None) the eager forward evaluates
        each sweep: the default, as the inference forward is GPU-bound (~1.3 ms per Lyft-grid sweep) and the plan, which
        voxelises every sweep again from its points, measured 3-4 % slower (tools/bench_eval.py)."""
        req = self._plan_request(samples) if _lib.knob("eval_plan", False) else None
        if req is None:
            return None
        key, grid, dtype, need, capacity, _ = req
        key += () if wform is None else (wform,)
        step = _reusable(self._eval_captured, key, need)
        if step is None:
            # the training step's voxeliser, whose workspace already holds a training sweep: a validation sweep no
            # larger than the training ones then allocates nothing, and the recorded training step stays valid
            train = self._captured
            if train is not None and train[0][0] == grid and train[1].plans and train[1].vox.subsample == "first":
                vox = train[1].vox
            else:
                vox = Voxelizer(*grid, device=self.net.device)
            step = EvalStep(self.net, vox, capacity, dtype=dtype, loss=self.loss, wform=wform)
            self._eval_captured = (key, step)
        return step

    def _labels(self, y, n):
        """[y_cls, y_reg] -> float32 arrays holding at least n label maps of the model's output grid each."""
        ycls = np.asarray(y[0], dtype=np.float32)
        yreg = np.asarray(y[1], dtype=np.float32)
        if len(ycls) < n or len(yreg) < n:
            raise ValueError("fewer label maps than samples")
        hw = self.net.Ho * self.net.Wo
        if n and (ycls[0].size != hw * 2 or yreg[0].size != hw * 14):
            raise ValueError(f"label maps must be ({self.net.Ho},{self.net.Wo},2) and ({self.net.Ho},{self.net.Wo},14)")
        return ycls, yreg

    def evaluate(self, x, y, batch_size=None, verbose=1, sample_weight=None, steps=None, callbacks=None,
                 return_dict=False):
        """model.evaluate(x, [y_cls, y_reg]) -> [loss, ClassificationLayer_loss, RegressionLayer_loss, metrics...] in the
        order of metrics_names (a dict with those keys with return_dict=True): the compiled loss and metrics with inference BatchNormalization (the moving statistics), as a mean
        over the evaluated sweeps (the detection metrics of loss='voxelnet': the ratio of their two sums pooled over the sweeps).  The sweeps are independent, so every batch_size gives that value -- Keras' mean
        weighted by batch size; batch_size (Keras' default 32) only sets what `steps` counts: steps * batch_size sweeps.
        callbacks get on_test_begin / on_test_end.  Each sweep runs the eager forward(training=False), or, with
        LISEC_TUNING=eval_plan=1 and voxelised sweeps, the recorded evaluation step (EvalStep), which pads every sweep to
        its point capacity: the values of the eager path bit for bit on sweeps already padded to that capacity, and
        equal within rounding on others (kernels that plan per capacity may sum in another order).  Data parallel: every
        rank evaluates its share samples[rank::world] with the rank-mean moving statistics (what save() writes) and all
        ranks return the same values.  Changes no variable, slot or iteration count.  With weight regularizers `loss`
        includes their penalty P (the per-output losses do not), computed once per evaluation on the device.
        sample_weight: as for fit() -- the losses are the means over the sweeps of the weighted losses, weighted_metrics=
        are sum w*v / sum w pooled over the sweeps, metrics= stay unweighted.  A sample_weight array without any row is
        refused (NotImplementedError) in front of everything else: it weighs no sweep."""
        if self.optimizer is None:
            raise RuntimeError("compile() the model first")
        _refuse_empty_sample_weight(sample_weight)
        samples = self._as_samples(x)
        n = len(samples)
        if steps is not None:
            n = min(n, int(steps) * (32 if batch_size is None else int(batch_size)))
        ycls, yreg = self._labels(y, n)
        sw = _sample_weight_arrays(sample_weight, n, (self.net.Ho, self.net.Wo))
        callbacks = list(callbacks or [])
        for cb in callbacks:
            cb.set_model(self)
            cb.set_params(dict(verbose=verbose, epochs=1, steps=steps))
        logs = self._evaluate(samples[:n], ycls, yreg, sw, callbacks=callbacks, verbose=verbose)
        return dict(logs) if return_dict else [logs[k] for k in self.metrics_names]

    def _evaluate(self, samples, ycls, yreg, sw=None, callbacks=(), verbose=0):
        for cb in callbacks:
            cb.on_test_begin()
        t0 = time.time()
        weighted = sw is not None
        sums, count = loss_acc_split(self.loss, self._eval_sums(samples, ycls, yreg, sw), weighted)
        logs = dict(zip(self.metrics_names, loss_acc_logs(self.loss, sums, count, weighted)))
        if verbose:
            print(f"{int(count)}/{int(count)} - {time.time() - t0:.1f}s - " +
                  " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()))
        for cb in callbacks:
            cb.on_test_end(logs)
        return logs

    def _eval_sums(self, samples, ycls, yreg, sw=None):
        """The float64 accumulator of loss_acc_len's layout summed over the sweeps, read back once.  Data parallel: rank r takes
        samples[r::world] (every sweep is evaluated once; DataParallel.shard would drop the tail), evaluates with the
        rank-mean BatchNormalization moving statistics (copy, average, evaluate, restore) and the sums are all-reduced."""
        net, dev = self.net, self.net.device
        idx = range(len(samples))
        own = None
        if self.dp is not None:
            idx = idx[self.dp.rank::self.dp.world]
            own = net.params.state.clone()
            self.dp.average_(net.params.state)
            net.state_version += 1                  # the folds of the replica's own statistics are stale
        try:
            weighted = sw is not None
            step = self._eval_step([samples[i] for i in idx], _weight_form(sw)) if idx else None
            if step is not None:
                step.reset()
                acc = step.acc
            else:
                acc = torch.zeros(loss_acc_len(self.loss, weighted), dtype=torch.float64, device=dev)
            if idx:
                target = _targets(ycls, yreg, idx, dev)
                weight = _weights_at(sw, idx, dev)
                for i in idx:
                    w = weight(i) if weighted else None
                    if step is not None:
                        step(samples[i]._keepalive, *target(i), w)
                    else:
                        net.forward(samples[i], training=False)
                        net.loss_eval(self.loss, *target(i), acc, w)
            if self.dp is not None:
                self.dp.sum_(acc)
            # the weight penalty, once per evaluation and enqueued behind the sweeps: every sweep's `loss` includes it
            # (theta is the same on every rank), so the sum over the sweeps gains sweeps * P
            pen = net.penalty()
            out = acc.cpu().numpy().copy()
            if pen is not None:
                out[0] += loss_acc_split(self.loss, out, weighted)[1] * float(pen.item())
            return out
        finally:
            if own is not None:
                net.params.state.copy_(own)
                net.state_version += 1

    def _snapshot_weights(self):
        """theta and the BatchNormalization moving statistics (what Keras' get_weights holds; no optimizer slots), as
        device copies (EarlyStopping(restore_best_weights=True))."""
        p = self.net.params
        return p.theta.clone(), p.state.clone()

    def _restore_weights(self, w):
        p = self.net.params
        torch.cuda.current_stream().wait_stream(self.net.side)   # behind what the last update left there to read theta
        p.theta.copy_(w[0])
        p.state.copy_(w[1])
        p.touch()                                   # every packed copy and fold is stale

    def predict(self, x):
        """predict(testVFEPointsDense) -> [prob (n,Ho,Wo,2), regress (n,Ho,Wo,14)] (Predict.py:38);
        BatchNormalization uses the moving statistics."""
        probs, regs = [], []
        for s in self._as_samples(x):
            cls, reg = self.net.forward(s, training=False)
            probs.append(cls.cpu().numpy().copy())
            regs.append(reg.cpu().numpy().copy())
        return [np.concatenate(probs), np.concatenate(regs)]

    def save(self, path):
        """model.save(save_path) (model_training.py:302): a Keras-layout HDF5 file (model_config, model_weights/<layer>/
        <layer>/<weight>:0 with Keras' automatic layer names, training_config and the optimizer's iteration count + slots
        -- SGD momentum accumulators, Adam moments, ..., Nadam's momentum_cache -- under optimizer_weights), written by lisec_amd.hdf5_lite -- see
        lisec_amd/keras_h5.py.  A path ending in .npz gets a plain numpy archive with the names of
        lisec_amd.params.param_specs() instead.  The weight regularizers go into the layer configs of the .h5, where
        load_model finds them; an .npz does not carry them (a model loaded from one has none)."""
        p = self.net.params
        if self.dp is not None:
            # data parallel: theta is identical on every rank, the BatchNormalization moving statistics are per
            # replica (each rank saw its own samples).  The checkpoint carries their MEAN over the ranks and is
            # written by rank 0 alone; the replicas' own statistics are left as they are.
            own = p.state.clone()
            self.dp.average_(p.state)
            d = p.to_dict() if self.dp.rank == 0 else None
            p.state.copy_(own)
            if self.dp.rank != 0:
                self.dp.barrier()
                return
        else:
            d = p.to_dict()
        try:
            self._write(path, d)
        finally:
            if self.dp is not None:
                self.dp.barrier()          # nobody reads the file before rank 0 has closed it

    def _write(self, path, d):
        os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
        if str(path).endswith(".npz"):
            meta = dict(format="lisec_amd-npz-1", nx=self.nx, ny=self.ny, nz=self.nz, maxPoints=self.maxPoints,
                        iterations=self.net.iterations)
            average = None
            if isinstance(self.optimizer, _AveragingOptimizer):
                # (only then: the archive of a model without a wrapper keeps its bytes)
                meta["optimizer"] = optimizers.serialize(self.optimizer)
                average = self._average_arrays()
            _npz_write(path, meta, d, average)
            return
        from . import keras_h5
        opt, slots, wrapper = None, {}, {}
        if isinstance(self.optimizer, _AveragingOptimizer):
            own = {k: v for k, v in self.optimizer.get_config().items() if k != "optimizer"}
            wrapper = dict(wrapper={"class_name": type(self.optimizer).__name__, "config": own},
                           average=self._average_arrays())
        if self.optimizer is not None:
            o, scalar = self.optimizer, self.optimizer.record.scalar
            opt = o.record.as_dict(_serialize_rate(o.lr), o.decay, o.hyper)
            opt.update(o.lists)                                    # (LAMB's exclusion lists; no key for any other class)
            inner = o._optimizer if isinstance(o, _AveragingOptimizer) else o
            if isinstance(inner, _DecoupledWeightDecay):
                # (only then: the file of an optimizer without decoupled decay keeps its bytes)
                opt.update(class_name=type(inner).__name__, weight_decay=_serialize_rate(inner.weight_decay))
                if inner.decay_var_list is not None:
                    opt["decay_var_list"] = list(inner.decay_var_list)
            opt.update(inner._clip_config())                       # (the clipping keys that are set; usually none)
            if scalar is not None:                                # Nadam's momentum_cache
                slots[scalar] = float(getattr(self.net, scalar).item())
            p = self.net.params
            for name in o.spec().slots:
                buf = self.net.slot(name)
                slots[name] = {n: p.view(n, buf=buf).detach().cpu().numpy() for n in p.trainable_names()}
        compiled = self._compile_args or {}
        keras_h5.save_model(path, d, self.nx, self.ny, self.nz, self.maxPoints, optimizer=opt,
                            iterations=self.net.iterations, regularizers=self.regularizers or None, **compiled, **slots,
                            **wrapper)

    def _average_arrays(self):
        """{trainable ParamStore name: array} of the weight average, as the slots travel."""
        p, buf = self.net.params, self.net.average
        torch.cuda.current_stream().wait_stream(self.net.side)       # behind the last update's averaging pass
        return {n: p.view(n, buf=buf).detach().cpu().numpy() for n in p.trainable_names()}

    def summary(self):
        n = self.net.params.n_trainable()
        print(f"LisecNet grid ({self.nz},{self.nx},{self.ny},{self.maxPoints},6) -> "
              f"({self.nx // 2},{self.ny // 2},2) / ({self.nx // 2},{self.ny // 2},14); trainable params: {n:,}")


_NPZ_AVERAGE = "__average__/"              # the key of a variable's average in an .npz archive: this, then its name


def _npz_write(path, meta, params, average=None):
    """The .npz form of a checkpoint: __meta__ (JSON), the variables by their ParamStore names and, for a model with an
    averaging wrapper, {trainable name: array} of the average under "__average__/<name>"."""
    extra = {_NPZ_AVERAGE + n: a for n, a in (average or {}).items()}
    with open(path, "wb") as f:
        np.savez(f, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **params, **extra)


def _npz_read(path):
    """-> (meta, {name: array} of the variables, {name: array} of the average: empty without one)."""
    z = np.load(path, allow_pickle=False)
    meta = json.loads(bytes(z["__meta__"]).decode())
    params = {k: z[k] for k in z.files if k != "__meta__" and not k.startswith(_NPZ_AVERAGE)}
    average = {k[len(_NPZ_AVERAGE):]: z[k] for k in z.files if k.startswith(_NPZ_AVERAGE)}
    return meta, params, average


def _deserialize_nested(x, deserialize):
    """training_config's loss / metrics -> compile() arguments: {"class_name", "config"} dicts become objects, the rest
    keeps its structure (Keras' _deserialize_nested_config)."""
    if isinstance(x, dict) and "class_name" in x:
        return deserialize(x)
    if isinstance(x, dict):
        return {k: _deserialize_nested(v, deserialize) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_deserialize_nested(v, deserialize) for v in x]
    return x


def _compile_saved(m, opt, ck):
    """Compiles a loaded model with the optimizer and the loss, loss_weights and metrics of its training_config."""
    saved = {k: ck.get(k) for k in ("loss", "loss_weights", "metrics", "weighted_metrics")}
    try:
        loss = _deserialize_nested(saved["loss"], losses.deserialize) if saved["loss"] is not None else ['mse', 'mse']
        m.compile(optimizer=opt, loss=loss, loss_weights=saved["loss_weights"],
                  metrics=_deserialize_nested(saved["metrics"], metrics.deserialize),
                  weighted_metrics=_deserialize_nested(saved["weighted_metrics"], metrics.deserialize))
    except (ValueError, NotImplementedError, TypeError) as e:
        warnings.warn(f"load_model: could not restore the compiled loss={saved['loss']!r}, "
                      f"loss_weights={saved['loss_weights']!r}, metrics={saved['metrics']!r}, "
                      f"weighted_metrics={saved['weighted_metrics']!r} ({e}); "
                      "compiled with loss=['mse', 'mse']", stacklevel=3)
        m.compile(optimizer=opt, loss=['mse', 'mse'])


def createModel(nx, ny, nz, maxPoints, kernel_regularizer=None, bias_regularizer=None, gamma_regularizer=None,
                beta_regularizer=None, activity_regularizer=None):
    """createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints) (model_training.py:222-257).
    kernel_regularizer / bias_regularizer / gamma_regularizer / beta_regularizer: a tf.keras 2.4 weight regularizer
    (lisec_amd/regularizers.py: regularizers.l2(1e-4), 'l1', ...) for every variable of that kind, as if each layer of
    the reference's createModel had been given it; see Model.  activity_regularizer: NotImplementedError."""
    return Model(nx, ny, nz, maxPoints, kernel_regularizer=kernel_regularizer, bias_regularizer=bias_regularizer,
                 gamma_regularizer=gamma_regularizer, beta_regularizer=beta_regularizer,
                 activity_regularizer=activity_regularizer)


def load_model(path, custom_objects=None):
    """load_model(model_path, custom_objects={'RepeatLayer':…, 'MaxPoolingVFELayer':…}) (:337-338, Predict.py:51-52).
    Reads Keras HDF5 files (the reference's own checkpoints or Model.save's) and the .npz variant.  Like Keras, a file
    that carries a training_config (SGD, Adam, RMSprop, Adagrad, Adadelta, Adamax or Nadam) comes back compiled, with the saved iteration count and optimizer slots;
    a learning-rate schedule in it is rebuilt, and continues from that iteration count.  The loss, loss_weights and metrics
    of the training_config are compiled again when compile() accepts them; otherwise the model is compiled with
    loss=['mse','mse'] and a warning names what could not be restored."""
    with open(path, "rb") as f:
        magic = f.read(8)
    dev = _lib.require_gpu()
    if magic[:4] != b"\x89HDF":
        meta, variables, average = _npz_read(path)
        params = ParamStore(dev, init=variables)
        m = Model(meta["nx"], meta["ny"], meta["nz"], meta["maxPoints"], params=params)
        m.net.iterations = int(meta.get("iterations", 0))
        if meta.get("optimizer") is not None:
            # an averaging wrapper (the only optimizer an archive carries): compiled with the reference's loss, and the
            # average restored; the wrapped optimizer's slots do not travel in an .npz and start at zero
            m.compile(optimizer=optimizers.deserialize(meta["optimizer"]), loss=['mse', 'mse'])
            m.net.iterations = int(meta.get("iterations", 0))
            _load_average(m, average)
        return m
    from . import keras_h5
    ck = keras_h5.load_model(path)
    m = Model(ck["nx"], ck["ny"], ck["nz"], ck["maxPoints"], params=ParamStore(dev, init=ck["params"]),
              variable_regularizers=ck["regularizers"])
    o = ck["optimizer"]
    if o is not None:
        lr = o["lr"]
        if isinstance(lr, dict):
            lr = lr_schedules.deserialize(lr)
        rec = optimizer_table.record_of(o)
        given = dict(learning_rate=lr, decay=o["decay"], **{h.name: o[h.name] for h in rec.hyper},
                     **{k: o.get(k) for k in rec.lists})
        if o.get("weight_decay") is None:
            opt = getattr(optimizers, rec.class_name)(**given)
        else:                                                        # <Base>W: decoupled weight decay
            wd = o["weight_decay"]
            if isinstance(wd, dict):
                wd = lr_schedules.deserialize(wd)
            opt = optimizers.extend_with_decoupled_weight_decay(getattr(optimizers, rec.class_name))(
                wd, decay_var_list=o.get("decay_var_list"), **given)
        optimizers.clip_gradients(opt, **{k: o.get(k) for k in _CLIP_KINDS})       # the clipping it was saved with
        w = ck.get("wrapper")
        if w is not None:
            if w["class_name"] not in optimizers.WRAPPERS:
                raise ValueError(f"{path}: optimizer wrapper class {w['class_name']!r} is not implemented")
            opt = getattr(optimizers, w["class_name"])(opt, **w["config"])
        _compile_saved(m, opt, ck)
        m.net.iterations = ck["iterations"]
        p = m.net.params
        for name in opt.spec().slots:
            saved = ck.get(name)
            if saved is None:
                continue
            buf = m.net.slot(name)
            for n in p.trainable_names():
                if n in saved:
                    p.view(n, buf=buf).copy_(torch.from_numpy(np.ascontiguousarray(saved[n])))
        if rec.scalar is not None and ck.get(rec.scalar) is not None:
            getattr(m.net, rec.scalar).fill_(float(ck[rec.scalar]))
        if w is not None and ck.get("average") is not None:
            _load_average(m, ck["average"])
    return m


def _load_average(m, saved):
    """Restores the weight average of a loaded model from {trainable ParamStore name: array}; a variable the file lacks
    keeps the copy of theta the average starts from."""
    p, buf = m.net.params, m.net.average
    for n in p.trainable_names():
        if n in saved:
            p.view(n, buf=buf).copy_(torch.from_numpy(np.ascontiguousarray(saved[n], dtype=np.float32)))


# ---------------------------------------------------------------------------------------------------
def _preprocess(samples, level5Data, dataDir):
    points = []
    for i in range(len(samples)):
        sampleLidarPoints = combine_lidar_data(samples[i], dataDir, level5Data)
        startTime = time.time()
        vfe_points = VFE_preprocessing(sampleLidarPoints, Constants.voxelx, Constants.voxely, Constants.voxelz,
                                       Constants.maxPoints, Constants.nx // 2, Constants.ny // 2, Constants.nz)
        points.append(vfe_points)       # stays sparse on the GPU: no to_dense, no 500 GB tf.stack (:279-285)
        print(time.time() - startTime)
        print('finished ' + str(i))
    return points


def _load_labels(labels_dir='labels3'):
    print('loading labels')
    outClass = np.load(os.path.join(labels_dir, 'labelsClass.npy'), allow_pickle=False)      # :289
    outRegress = np.load(os.path.join(labels_dir, 'regressClass.npy'), allow_pickle=False)   # :290
    return outClass, outRegress


def _train(samples, level5Data, save_path, model_path=None):
    """train and train_with_model: one epoch of 180 steps of the reference's SGD on a new model, or on the one saved at
    model_path."""
    _refuse_mixed_training(mixed_precision.global_policy())      # before the sweeps are voxelised, not at fit()
    trainPoints = _preprocess(samples, level5Data, Constants.lyft_data_dir)
    outClass, outRegress = _load_labels()
    if model_path is None:
        model = createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    else:
        model = load_model(model_path, custom_objects={'RepeatLayer': RepeatLayer,
                                                       'MaxPoolingVFELayer': MaxPoolingVFELayer})
    sgd = optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True)
    model.compile(optimizer=sgd, loss=['mse', 'mse'])
    history = model.fit(x=trainPoints, y=[outClass, outRegress], batch_size=1, verbose=1, epochs=1,
                        steps_per_epoch=180)
    if model.dp is None or model.dp.rank == 0:
        print(history.history)
    model.save(save_path)
    return model


def train(samples, level5Data, save_path):
    """train(samples, level5Data, save_path) (model_training.py:260-302)."""
    return _train(samples, level5Data, save_path)


def train_with_model(samples, level5Data, model_path, save_path):
    """train_with_model(samples, level5Data, model_path, save_path) (model_training.py:305-346)."""
    return _train(samples, level5Data, save_path, model_path)


def train_augmented(samples, level5Data, save_path, epochs=1, seed=0, sample_to=0, subsample='first', balance=True,
                    loss=None, batch_size=1):
    """OURS, not the reference's: train() on sweeps that are augmented anew at every step (augment.AugmentedSweeps: per-box
    noise with collision rejection, one global scale and rotation, VoxelNet section 3.3) with the label maps of the moved
    boxes made on the device (boxes.rpnTargets) instead of the precomputed labels3/*.npy.  The sweeps come from
    combine_lidar_data_gpu, the boxes from boxes.annotationBoxes; one pass over the samples per epoch, the reference's
    SGD.  sample_to > 0: ground-truth object sampling (augment.ObjectDatabase, built from the same sweeps and boxes) fills
    every sweep up towards that many boxes before the noise.  subsample='random': a voxel holding more than maxPoints
    points keeps the reference's random subsample, drawn anew per (seed, item, epoch), instead of the lowest point indices
    (AugmentedSweeps).  loss: compile()'s (None: the reference's ['mse','mse']); with loss='voxelnet' (losses.VoxelNetLoss, which normalises positives and
    negatives separately) balance=False is the natural setting: the label maps then keep every negative instead of a
    sample of them.  batch_size: fit()'s (the mean gradient of that many augmented sweeps per update; 1: the reference's).
    Returns the model, saved at save_path."""
    from . import augment, boxes
    batch_size = _check_batch_size(batch_size)
    _refuse_mixed_training(mixed_precision.global_policy())
    points = [combine_lidar_data_gpu(s, Constants.lyft_data_dir, level5Data) for s in samples]
    rows = [boxes.annotationBoxes(s, level5Data) for s in samples]
    model = createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    sgd = optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True)
    model.compile(optimizer=sgd, loss=['mse', 'mse'] if loss is None else loss)
    database = augment.ObjectDatabase(points, rows) if sample_to > 0 else None
    seq = augment.AugmentedSweeps(points, rows, seed=seed, database=database, sample_to=sample_to, subsample=subsample,
                                  balance=balance)
    history = model.fit(x=seq, batch_size=batch_size, verbose=1, epochs=epochs)
    if model.dp is None or model.dp.rank == 0:
        print(history.history)
    model.save(save_path)
    return model


def _lyft_dataset():
    """The driver blocks of the reference build a LyftDataset from a hard-coded Windows path (model_training.py:349-355,
    Predict.py:43-49); here the root comes from Constants.lyft_data_dir ($LISEC_LYFT_DATA_DIR)."""
    try:
        from lyft_dataset_sdk.lyftdataset import LyftDataset
    except ImportError as e:                       # the SDK is not a dependency of the hot path
        raise SystemExit("the command-line driver needs lyft_dataset_sdk (pip install lyft-dataset-sdk): " + str(e))
    return LyftDataset(data_path=Constants.lyft_data_dir, json_path=os.path.join(Constants.lyft_data_dir, 'train_data'),
                       verbose=True)


if __name__ == '__main__':
    # python -m lisec_amd.model_training [save_path]      (model_training.py:349-364)
    import sys
    level5Data = _lyft_dataset()
    save_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join('models', '180SampleEpoch0.h5')
    samples = [level5Data.get('sample', scene['first_sample_token']) for scene in level5Data.scene]
    print('Training on ' + str(len(samples)))
    train(samples[:], level5Data, save_path)
