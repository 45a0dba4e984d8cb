"""The Lisec network (createModel, reference model_training.py:222-257) as a static schedule of
C-ABI calls on one HIP stream.

There is no graph tracer and no autograd: the layer order is fixed, so forward and backward are
explicit launch sequences over pre-allocated device buffers.  BatchNormalization(+ReLU) of a layer
is never materialised: every consumer applies scale/shift(+ReLU) while staging its input tile, so
only the raw convolution outputs ("y") live in HBM.  Per sample (batch 1, as model.fit(batch_size=1),
model_training.py:299):

    voxel sample -> VFE (sparse-exact) -> grid (D,H,W,64)
    mid_i : y_i = conv3d(u_{i-1}) ; stats ; u_i = relu(bn(y_i) @ Wd_i)              i = 1..3
    rpn_b : y_{b,j} = conv2d(relu(bn(y_{b,j-1}))) ; stats                           j = 0..q_b
    up_b  : concat[..., 256b:256(b+1)] = deconv(relu(bn(y_{b,q})))
    head  : (M,16) = concat @ [W_cls | W_reg] + bias     (cls = [:, :2], reg = [:, 2:])
"""
import ctypes
import json
import math
import os

import numpy as np
import torch

from . import _lib, lr_schedules, ops, optimizer_table
from .losses import DetectionIoULossSpec, DetectionLossSpec, LossSpec
from .params import DECONVS, MID, RPN_BLOCKS, ParamStore, fold_depth
from .vfe import VFEStack


LEGACY_LOSS_KINDS = {"mse": 0, "smoothl1_ce": 1}        # the `kind` of lisec_rpn_loss / lisec_rpn_loss_eval


def weight_form(weights):
    """The form of a step's sample weights, per output: None (no weights at all), or a pair of None (that output has
    weight 1), 'sweep' (one float) or 'cell' (one per cell of the output grid).  weights: None, or a pair of float32
    device tensors / None.  The form is part of the key of a recorded plan; the values are device data."""
    if weights is None:
        return None
    return tuple(None if w is None else ("sweep" if w.numel() == 1 else "cell") for w in weights)


def _paired(loss, weighted):
    """Do the metric words of this step loss's accumulator hold {num, den} pairs behind a sweep count in acc[3]?  The
    detection losses always; a LossSpec where the step is weighted (lisec_head_loss_weighted*)."""
    return isinstance(loss, DetectionLossSpec) or (weighted and isinstance(loss, LossSpec))


def loss_acc_len(loss, weighted=False):
    """Length of the evaluation accumulator of a step loss; KeyError for a string that names no legacy loss.  The layout:
        legacy string      [total, class, regression, sweeps]
        LossSpec           [total, class, regression, metrics..., sweeps]     (per-sweep values, summed)
        DetectionLossSpec  [total, class, regression, sweeps, num0, den0, num1, den1, ...]
        weighted LossSpec  the layout of the DetectionLossSpec (lisec_head_loss_weighted_eval)
    A DetectionLossSpec keeps the sweep count in acc[3], where lisec_detection_loss_eval writes it, and appends the
    {num, den} pairs of its metrics (lisec_detection_metrics with accumulate): sums pooled over the sweeps.  weighted: the
    step runs under sample weights; a legacy string then runs as its LossSpec without metrics, whose layout is its own."""
    if _paired(loss, weighted):
        return 4 + 2 * loss.n_metrics
    if isinstance(loss, LossSpec):
        return 4 + loss.n_metrics
    LEGACY_LOSS_KINDS[loss]                 # refuses an unknown name
    return 4


def pair_values(pairs):
    """[num0, den0, num1, den1, ...] -> [num/den, ...]; 0.0 where den == 0 (Keras' div_no_nan)."""
    return [float(n / d) if d != 0 else 0.0 for n, d in zip(pairs[0::2], pairs[1::2])]


def loss_acc_logs(loss, sums, count, weighted=False):
    """[total, class, regression, metrics...] in the order of Model.metrics_names from sums, laid out as [total, class,
    regression, the metric words of loss_acc_len's layout...] (numpy float64), over `count` sweeps: the losses and an
    unweighted LossSpec's metrics are means over the sweeps (NaN without any); metrics kept as pairs (a
    DetectionLossSpec's, a weighted LossSpec's) are num/den of the pooled pairs, 0.0 when den == 0 (Keras' div_no_nan)."""
    mean = [float(v / count) if count else float("nan") for v in sums[:3]]
    if _paired(loss, weighted):
        return mean + pair_values(sums[3:3 + 2 * loss.n_metrics])
    return mean + [float(v / count) if count else float("nan") for v in sums[3:]]


def loss_acc_split(loss, acc, weighted=False):
    """An evaluation accumulator (numpy, loss_acc_len's layout) -> (sums as loss_acc_logs takes them, sweeps)."""
    if _paired(loss, weighted):
        return np.concatenate([acc[:3], acc[4:]]), acc[3]
    return acc[:-1], acc[-1]


class AverageSpec:
    """The weight averaging of a step (optimizers.MovingAverage / optimizers.SWA; csrc/weight_average.hip): after every
    update one pass folds theta into LisecNet.average.  kind 'ema': a <- a - (a - w)*(1 - decay_s), decay_s = 0 before
    iteration `start`, then `decay`, or with `dynamic` min(decay, (1 + k)/(10 + k)), k = iterations - start; kind
    'swa': a <- (a*m + w)/(m + 1) at the iterations start + m*period, nothing at the others.  Every refusal of the
    library (include/lisec_hip.h) is a ValueError here, before any launch."""

    KINDS = {"ema": _lib.AVG_EMA, "swa": _lib.AVG_SWA}

    def __init__(self, kind, decay=0.0, dynamic=False, start=0, period=1):
        if kind not in self.KINDS:
            raise ValueError(f"unknown averaging kind {kind!r}")
        for name, v in (("start", start), ("period", period)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"the averaging {name} must be an integer, not {v!r}")
        self.kind, self.decay, self.dynamic = kind, float(decay), bool(dynamic)
        self.start, self.period = int(start), int(period)
        if kind == "ema" and not 0.0 <= self.decay <= 1.0:       # (NaN fails both comparisons)
            raise ValueError(f"average_decay must lie in [0, 1], not {decay!r}")
        if self.start < 0:
            raise ValueError(f"averaging cannot start at the negative iteration {start}")
        if kind == "swa" and self.period < 1:
            raise ValueError(f"average_period must be >= 1, not {period}")
        self.descriptor = _lib.WeightAverage(self.KINDS[kind], int(self.dynamic), self.start, self.period, self.decay)

    @property
    def config(self):
        """Hashable; part of OptimizerSpec.config, the key of the recorded plans (the descriptor is a launch argument)."""
        if self.kind == "ema":
            return ("ema", self.decay, self.dynamic, self.start)
        return ("swa", self.start, self.period)

    def __eq__(self, other):
        return isinstance(other, AverageSpec) and self.config == other.config

    def __hash__(self):
        return hash(self.config)

    def __repr__(self):
        return f"AverageSpec{self.config}"


class DecaySpec:
    """The decoupled weight decay of a step (optimizers.AdamW / SGDW / extend_with_decoupled_weight_decay;
    csrc/weight_decay.hip): directly in front of every optimizer update, w <- w - wd_t*w on the decayed variables, wd_t
    the coefficient at the iteration count before the update -- NOT multiplied by the learning rate.
    weight_decay: a number (finite, >= 0, finite in float32; else ValueError) or one of the built-in
    LearningRateSchedules (one of the user's own: NotImplementedError, from lr_schedules.descriptor).
    variables: None -- every trainable variable, tfa's default --, or an iterable of ParamStore names and / or the kinds
    'kernel', 'bias', 'gamma', 'beta'; the names are resolved by the network that runs the step (ops.decay_chunks)."""

    def __init__(self, weight_decay, variables=None):
        self.schedule = weight_decay if isinstance(weight_decay, lr_schedules.LearningRateSchedule) else None
        if self.schedule is None:
            try:
                value = None if isinstance(weight_decay, bool) else float(weight_decay)
            except (TypeError, ValueError):
                value = None
            if value is None or not 0 <= value <= float(np.finfo(np.float32).max):       # (NaN fails both comparisons)
                raise ValueError(f"weight_decay must be a finite number >= 0 (finite in float32) or a "
                                 f"LearningRateSchedule, not {weight_decay!r}")
            weight_decay = value
        self.weight_decay = weight_decay
        if variables is not None:
            if isinstance(variables, str):
                variables = (variables,)
            variables = tuple(variables)
            if not all(isinstance(v, str) for v in variables):
                raise ValueError(f"the decayed variables must be given by name or kind, not {variables!r}")
        self.variables = variables
        # validates a schedule: NotImplementedError for one of the user's own, ValueError past the device's limits
        self.descriptor = lr_schedules.descriptor(weight_decay, 0.0)

    @property
    def is_zero(self):
        """The constant number 0: no decay at all."""
        return self.schedule is None and self.weight_decay == 0

    @property
    def config(self):
        """Hashable; part of OptimizerSpec.config.  A schedule enters with its whole Keras config; a number does not
        enter at all -- ("device",), as with device_lr: it is data of the step, not of its launches."""
        if self.schedule is not None:
            rate = ("schedule", json.dumps(lr_schedules.serialize(self.schedule), sort_keys=True))
        else:
            rate = ("device",)
        return (rate, self.variables)

    def __eq__(self, other):
        return isinstance(other, DecaySpec) and self.config == other.config

    def __hash__(self):
        return hash(self.config)

    def __repr__(self):
        return f"DecaySpec({self.weight_decay!r}, variables={self.variables!r})"


class ClipSpec:
    """The gradient clipping of a step (optimizers.clip_gradients; csrc/grad_clip.hip): behind the penalty pass and in
    front of the decoupled weight decay and the optimizer entry, the gradient is bounded in place.
    kind 'value': every element clamped to [-value, value]; 'norm': every variable scaled so that its L2 norm is at most
    value; 'global_norm': the whole gradient scaled so that its L2 norm over all trainable variables is at most value.
    value: a finite number > 0, finite in float32 (else ValueError; a bool is refused).  It is a kernel argument and
    part of the config: a changed threshold is another recorded plan."""

    KINDS = ("value", "norm", "global_norm")

    def __init__(self, kind, value):
        if kind not in self.KINDS:
            raise ValueError(f"unknown clipping kind {kind!r}: one of {', '.join(self.KINDS)}")
        try:
            number = None if isinstance(value, bool) else float(value)
        except (TypeError, ValueError):
            number = None
        if number is None or not 0 < number <= float(np.finfo(np.float32).max):       # (NaN fails both comparisons)
            raise ValueError(f"a clipping threshold must be a finite number > 0 (finite in float32), not {value!r}")
        self.kind, self.value = kind, number

    @property
    def config(self):
        """Hashable; part of OptimizerSpec.config, the key of the recorded plans (the threshold is a launch argument)."""
        return (self.kind, self.value)

    def __eq__(self, other):
        return isinstance(other, ClipSpec) and self.config == other.config

    def __hash__(self):
        return hash(self.config)

    def __repr__(self):
        return f"ClipSpec{self.config}"


class OptimizerSpec:
    """One optimizer of the step: its kind, the tf.keras 2.4 hyper-parameters and the names of the slots it keeps --
    per-variable state buffers of LisecNet shaped like theta (LisecNet.slot).  The default is the reference's
    SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True) (model_training.py:295).  What a kind has is read from its
    record in lisec_amd/optimizer_table.py (`record`); in short:

        sgd       momentum == 0: no slot;  momentum > 0: "velocity" (v <- m*v - lr_t*g, then w <- w + v, or Nesterov)
        adam      "m", "v", and "vhat" with amsgrad
        rmsprop   "rms"; "momentum" with momentum > 0 (a buffer of its own: not SGD's velocity); "mg" when centered
        adagrad   "accumulator" (Model.compile starts it at initial_accumulator_value)
        adadelta  "accum_grad", "accum_var"
        adamax    "m", "v"
        nadam     "m", "v", and LisecNet.momentum_cache (a device scalar next to the iteration count)

    lr is a number or a LearningRateSchedule (lisec_amd.lr_schedules).  With a schedule, or with device_lr=True (a
    number that may change between steps, e.g. from a LearningRateScheduler callback), the update kernels read lr_t from
    LisecNet's device descriptor (lisec_lr_schedule), which holds `lr_descriptor`; otherwise (lr, decay) are kernel
    arguments, as they always were.  Nadam's `decay` is its momentum-schedule decay (schedule_decay): its rate is not
    divided by 1 + decay*it, its descriptor is built with decay = 0, and a schedule is refused as in tf.keras 2.4.
    average: an AverageSpec, or None (no averaging: the step issues exactly the launches it always did, and `config`
    is the tuple it always was).
    weight_decay: a DecaySpec, or None; the constant number 0 is the same as None (no decay: no launch, and the base
    optimizer's `config`).
    kind "lamb" (layer-wise: csrc/lamb.hip) keeps "m" and "v", has weight_decay_rate -- its own decay, inside the
    step -- and the two lists exclude_from_weight_decay / exclude_from_layer_adaptation (None, or ParamStore names and /
    or kinds; the second None: the first), which enter `config` for this kind alone, behind the hyper-parameters; the
    network that runs the step resolves them (ops.lamb_chunks).  A DecaySpec is refused.
    clip: a ClipSpec, or None (no clipping: the step issues exactly the launches it always did, and `config` is the
    tuple it always was)."""

    KINDS = tuple(optimizer_table.BY_KIND)

    def __init__(self, kind="sgd", lr=0.01, decay=1e-6, momentum=0.9, nesterov=True, beta_1=0.9, beta_2=0.999,
                 epsilon=None, amsgrad=False, device_lr=False, rho=0.9, centered=False, initial_accumulator_value=0.1,
                 average=None, weight_decay=None, weight_decay_rate=0.0, exclude_from_weight_decay=None,
                 exclude_from_layer_adaptation=None, clip=None):
        rec = self.record = optimizer_table.BY_KIND.get(kind)
        if rec is None:
            raise ValueError(f"unknown optimizer kind {kind!r}")
        if average is not None and not isinstance(average, AverageSpec):
            raise ValueError(f"average must be an AverageSpec or None, not {average!r}")
        self.average = average
        if clip is not None and not isinstance(clip, ClipSpec):
            raise ValueError(f"clip must be a ClipSpec or None, not {clip!r}")
        self.clip = clip
        if weight_decay is not None and not isinstance(weight_decay, DecaySpec):
            raise ValueError(f"weight_decay must be a DecaySpec or None, not {weight_decay!r}")
        self.weight_decay = None if weight_decay is None or weight_decay.is_zero else weight_decay
        self.schedule = lr if isinstance(lr, lr_schedules.LearningRateSchedule) else None
        if self.schedule is not None and not rec.takes_schedule:
            raise ValueError(f"The {rec.class_name} optimizer does not support tf.keras.optimizers.LearningRateSchedules "
                             f"as the learning rate.")
        self.kind, self.lr, self.decay = kind, (lr if self.schedule is not None else float(lr)), float(decay)
        self.device_lr = bool(device_lr) or self.schedule is not None
        # validates a schedule: NotImplementedError for one of the user's own, ValueError past the device's limits
        self.lr_descriptor = (lr_schedules.descriptor(self.lr, 0.0 if rec.schedule_decay else self.decay)
                              if self.device_lr else None)
        given = dict(momentum=momentum, nesterov=nesterov, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon, amsgrad=amsgrad,
                     rho=rho, centered=centered, initial_accumulator_value=initial_accumulator_value,
                     weight_decay_rate=weight_decay_rate)
        for h in rec.hyper:                     # a spec carries the hyper-parameters of its own kind, and no others
            # (epsilon None: the default of the kind's record -- 1e-7 for the Keras optimizers, 1e-6 for LAMB)
            value = h.coerce(h.default if given[h.name] is None else given[h.name])
            if not h.valid(value):
                raise ValueError(h.error)
            setattr(self, h.name, value)
        if rec.schedule_decay and self.decay < 0:
            raise ValueError("schedule_decay must be >= 0")
        if rec.layerwise and weight_decay is not None:
            raise ValueError(f"{rec.class_name} carries its own weight decay (weight_decay_rate): it takes no DecaySpec")
        lists = dict(exclude_from_weight_decay=exclude_from_weight_decay,
                     exclude_from_layer_adaptation=exclude_from_layer_adaptation)
        for name in rec.lists:                  # (of a layer-wise kind alone: no other spec has the attributes)
            value = lists[name]
            if value is not None:
                value = (value,) if isinstance(value, str) else tuple(value)
                if not all(isinstance(x, str) for x in value):
                    raise ValueError(f"{name} takes variable names and kinds, not {lists[name]!r}")
            setattr(self, name, value)
        # (ops entry, slot names, argument names) of LisecNet._update, worked out once: it runs twice in every eager step
        self.launch = rec.launch(self.hyper, self.device_lr)

    @property
    def hyper(self):
        """{name: value} of the kind's hyper-parameters after the rate and decay, in Keras' order."""
        return {h.name: getattr(self, h.name) for h in self.record.hyper}

    @property
    def config(self):
        """Every hyper-parameter, hashable: two specs with equal configs issue the same launches.  A schedule enters with
        its whole Keras config; a number read from the device descriptor (device_lr) does not enter at all -- like the
        iteration count, it is data of the step, not of its launches.  The averaging joins only when there is one, and
        so do the decoupled weight decay and the clipping."""
        if self.schedule is not None:
            rate = ("schedule", json.dumps(lr_schedules.serialize(self.schedule), sort_keys=True))
        elif self.device_lr:
            rate = ("device",)
        else:
            rate = self.lr
        base = (self.kind, rate, self.decay, *self.hyper.values(), *self.lists)
        if self.average is not None:
            base += (("average",) + self.average.config,)
        if self.weight_decay is not None:
            base += (("weight_decay",) + self.weight_decay.config,)
        if self.clip is not None:
            base += (("clip",) + self.clip.config,)
        return base

    @property
    def lists(self):
        """The variable lists of a layer-wise kind (exclude_from_weight_decay, exclude_from_layer_adaptation), each a
        tuple or None; () for every other kind."""
        return tuple(getattr(self, name) for name in self.record.lists)

    @property
    def slots(self):
        return tuple(s.name for s in self.record.active_slots(self.hyper))

    def __eq__(self, other):
        return isinstance(other, OptimizerSpec) and self.config == other.config

    def __hash__(self):
        return hash(self.config)

    def __repr__(self):
        return f"OptimizerSpec{self.config}"


class _DeviceDescriptor:
    """A lisec_lr_schedule at a fixed device address (`dev`) and the host descriptor last written into it (`host`)."""

    def __init__(self, device):
        self.dev = torch.zeros(ctypes.sizeof(_lib.LrSchedule), dtype=torch.uint8, device=device)
        self.host = None

    def sync(self, desc):
        """Makes `dev` hold desc: a copy on the current stream, behind every update already enqueued, when the contents
        differ from the last ones written."""
        if self.host is None or bytes(self.host) != bytes(desc):
            ops.lr_schedule_set(self.dev, desc)
            self.host = desc                                  # kept alive: the source of the copy


class ConvLayer:
    """One dense contraction: geometry + packed-weight slot + (optional) BatchNormalization."""

    def __init__(self, name, g, wname, pack, bias=None, bn=None, in_bn=None, in_relu=False, out_relu=False):
        self.name, self.g, self.wname, self.pack = name, g, wname, pack
        self.bias, self.bn, self.in_bn, self.in_relu, self.out_relu = bias, bn, in_bn, in_relu, out_relu
        self.M = g.Do * g.Ho * g.Wo
        self.nmb = ops.num_mblocks(g)


class _SideQueue:
    """The fork protocol between the stream a pass is issued on (main) and the net's second stream (side).  Closures are
    queued (defer) and cross to the second stream together, behind ONE event of the main stream (flush; run = defer +
    flush).  Events are made, recorded and waited for through the net (_new_event, _record, _wait): a step plan sees
    them, and tools/ override those three."""

    def __init__(self, net, main, side):
        self.net, self.main, self.side = net, main, side
        self.events = []                       # fork events, reused pass after pass: recorded step plans hold them
        self.nfork = 0                         # how many of them this pass has recorded
        self.pending = []                      # (closure, torch_ops) that the next flush() runs
        self.marked = []                       # events recorded ahead of the flush() that waits for them

    def begin(self, main=None):
        """Starts a pass, on `main` if given: the pool's events are handed out from the first again."""
        if main is not None:
            self.main = main
        self.nfork = 0
        del self.pending[:], self.marked[:]

    def mark_fork(self, ev=None):
        """Records the fork event NOW (ev; None: the pool's next); the next flush() waits for this one instead of recording
        its own.  Lets the chain's next kernel be ENQUEUED before the second stream's work although that work does not
        depend on it."""
        if ev is None:
            if self.nfork == len(self.events):
                self.events.append(self.net._new_event())
            ev = self.events[self.nfork]
            self.nfork += 1
        self.net._record(ev, self.main)
        self.marked.append(ev)

    def defer(self, fn, torch_ops=False):
        """Queues fn for the next flush().  C-ABI launches take the pinned handle; only a fn that also issues torch /
        torch.distributed work (torch_ops) needs torch's (slow) stream context."""
        self.pending.append((fn, torch_ops))

    def flush(self):
        """Records ONE event on the main stream (unless one is marked) and runs every pending closure on the second
        stream behind it.  Nothing pending: nothing happens, and a mark stays for the next flush."""
        if not self.pending:
            return
        if not self.marked:
            self.mark_fork()
        self.net._wait(self.marked.pop(), self.side)
        pin = _lib.pin_stream(self.side.cuda_stream)
        try:
            for fn, torch_ops in self.pending:
                if torch_ops:
                    with torch.cuda.stream(self.side):
                        fn()
                else:
                    fn()
        finally:
            _lib.pin_stream(pin)
            del self.pending[:]

    def run(self, fn, torch_ops=False):
        """Runs fn's launches on the second stream after everything issued so far on the main one."""
        self.defer(fn, torch_ops)
        self.flush()

    def join(self, ev):
        """The main stream waits for everything issued so far on the second one."""
        self.net._record(ev, self.side)
        self.net._wait(ev, self.main)


class _BackwardPass:
    """One call of LisecNet._backward: what the pass has done so far, and one method per layer kind, called last layer
    first.  The data-gradient chain runs on the main stream; the leaves (weight and bias gradients, the early upsampling
    branches) go through the _SideQueue `q`.  With collapsed heads, heads() and early_branches() only queue (q.defer):
    the first q.run of the chain, in deconv(), carries them across behind its one event.  finish() queues the late
    reduces and flushes them itself.  Every other leaf crosses where it is issued (q.run)."""

    def __init__(self, net, q, sample, rpn_grads_ready, side_filler):
        self.net, self.q, self.sample = net, q, sample
        self.rpn_grads_ready, self.side_filler = rpn_grads_ready, side_filler
        self.rcap = max(sample.cap, 1)         # an empty sweep still needs a non-zero row-list capacity
        self.branches_left = len(DECONVS)      # collapsed branches whose rows of the head-kernel gradient are still missing
        self.batched_convs = set().union(*[names for _, names in net.wgrad_batches.values()])
        self.first_write = set()               # gradient buffers that already hold a contribution
        self.writes = {}                       # gradient buffer -> contributions stored so far
        self.bwd_ready = {}                    # gradient buffer -> partial rows of its BN-backward statistics
        self.early_dst = {}                    # gradient buffer -> event behind a contribution made on the second stream
        self.fused_dense = {}                  # middle block -> backward sink of a Dense data gradient that rode on a tile
        self.late_reduces = []                 # slab sums of the carried Dense weight gradients
        self.early_layers = set()              # upsampling branches that early_branches() has already differentiated

    def dgrad_into(self, c, dy, dst_name, ws_tag="main"):
        net, a, d = self.net, self.net.act, self.net.dact
        ev = self.early_dst.pop(dst_name, None) if ws_tag == "main" else None
        if ev is not None:
            net._wait(ev, self.q.main)         # the branch's contribution is stored before this one accumulates onto it
        flags = ops.ACCUMULATE if dst_name in self.first_write else 0
        # the output of a middle block went through Dense(relu) (model_training.py:195): its gradient is gated
        # by that activation while the data gradient is stored (single consumer, so no ACCUMULATE there)
        mask = a[dst_name] if dst_name.endswith(".u") else None
        # the LAST contribution to the gradient of a conv output also reduces the statistics its
        # BatchNormalization backward needs (pass 1 of bn_backward folded into the store)
        self.writes[dst_name] = self.writes.get(dst_name, 0) + 1
        bwd = sink = tail = None
        if dst_name in net.bn_of and self.writes[dst_name] == net.consumers[dst_name]:
            bn_name, C = net.bn_of[dst_name]
            bwd, sink = (a[dst_name], net.bnstate[bn_name], True), net._bwd_sink(bn_name, C, a[dst_name].numel() // C)
            self.bwd_ready[dst_name] = sink
        use_w = c.name in net.packed_wu_t
        if mask is not None and not use_w and net._tail_supported(c, dst_name):
            # the Dense(64, relu) of the block BELOW (model_training.py:195) rides on this tile: its data gradient
            # dz = (gated gradient) @ Wd^T and the statistics of the BatchNormalization under it come out of the same
            # launch (lisec_conv_extras.tail_w); the separate Dense data-gradient launch is skipped further down
            n = dst_name[:-2]
            Ln = next(L for L in net.layers if L["name"] == n)
            cn, dn = Ln["conv"], Ln["dense"]
            sink = net._bwd_sink(cn.bn, 64, cn.M)
            bwd = (a[n + ".y"], net.bnstate[cn.bn], False)
            tail = (net.packed_t[dn.name][0], d[n + ".z"])
            self.fused_dense[n] = sink
        if use_w:
            ops.conv_forward_winograd(net.dgeom[c.name], dy, net.packed_wu_t[c.name], d[dst_name], flags=flags,
                                      out_mask=mask, bwd=bwd, sink=sink, tail=tail)
        else:
            ops.conv_forward(net.dgeom[c.name], dy, net.packed_t[c.name][0], d[dst_name], flags=flags | ops.SMALL_TILE,
                             out_mask=mask, bwd=bwd, sink=sink, ws_tag=ws_tag, tail=tail)
        self.first_write.add(dst_name)

    def branch_dy(self, L):
        """The gradient a branch's contraction produced: a concat slice, or (collapsed form) the head gradient / its
        (tap, j) columns."""
        d = self.net.dact
        if not self.net.compose_head:
            return d["concat"][:, :, 256 * L["slot"]:]
        return d["head"] if L["dT"] is None else L["dT"]

    def deconv_wgrad(self, L):
        net, a, p, G = self.net, self.net.act, self.net.params, self.net.grad
        c = L["conv"]
        if net.compose_head:
            b, (ts, cs) = L["slot"], L["wc_strides"]
            ops.conv_wgrad(c.g, a[L["src"]], self.branch_dy(L), L["G"], net.wgrad_ws, in_bn=net.bnstate[c.in_bn],
                           flags=ops.IN_RELU)
            ops.head_compose_backward(L["G"], ts, cs, p.view(L["up_kernel"]), p.view(L["up_bias"]),
                                      net.head_w[256 * b:256 * (b + 1)],
                                      net.head_db, L["k"] * L["k"], L["cin"], 256, p.grad_view(G, L["up_kernel"]),
                                      p.grad_view(G, L["up_bias"]), net.head_dw[256 * b:256 * (b + 1)])
            self.branches_left -= 1
            if self.branches_left == 0:
                net._head_split.run()          # every row of dH is final: merged (768,16) -> the Keras-shaped slots
            return
        dy = self.branch_dy(L)
        if "wgeom" in L:
            ops.conv_wgrad(L["wgeom"], dy, a[L["src"]], p.grad_view(G, c.wname), net.wgrad_ws,
                           flags=ops.DY_RELU, dy_bn=net.bnstate[c.in_bn])
        else:
            ops.conv_wgrad(c.g, a[L["src"]], dy, p.grad_view(G, c.wname), net.wgrad_ws,
                           in_bn=net.bnstate[c.in_bn], flags=ops.IN_RELU, transpose_out=True)

    def heads(self):
        """The 1x1 heads (model_training.py:254-255).  Only the data gradient is on the way to the rest of the backward
        pass: the heads' weight and bias gradients and the deconv bias gradients (column sums of the concat gradient) are
        leaves and go to the second stream."""
        net, q, a, d = self.net, self.q, self.net.act, self.net.dact
        M = net.Ho * net.Wo
        if net.compose_head:
            # collapsed branches + heads: the head gradient feeds the three 16-channel contractions directly; its column
            # sums (the heads' bias gradient, and through H the branch biases) are the only pass over it
            net._dshuffle.run(d["head"], backward=True)
            # (queued, not flushed: the leaves and branches that hang off the head gradient cross to the second stream
            # behind ONE event, with the first of them that is issued through q.run)
            q.defer(lambda: ops.colsum(d["head"], 16, M, 16, net.head_db, ws_tag="side"))
            return

        def head_leaves():
            ops.conv_wgrad(net.head_geom, a["concat"], d["head"], net.head_dw, net.wgrad_ws)
            ops.colsum(d["head"], 16, M, 16, net.head_db, ws_tag="side")
            net._head_split.run()

        def concat_leaves():
            # the three deconv bias gradients are the column sums of the concat gradient: one pass over it
            ops.colsum(d["concat"], 768, M, 768, net.up_db, ws_tag="side")
            net._up_bias_split.run()

        q.run(head_leaves)
        ops.conv_forward(net.head_dgeom, d["head"], net.packed_t["head"][0], d["concat"])
        q.run(concat_leaves)

    def early_branches(self):
        """The Conv2DTranspose branches of blocks 1 and 2 hang off the concat gradient, which is complete now: both of
        their gradients go to the second stream at once, beside the small layers of blocks 3 and 2, instead of waiting
        on the chain for their turn; the chain picks their contribution up where it reaches the block's last conv."""
        net, q = self.net, self.q
        for L in net.layers:
            if L["kind"] == "deconv" and L["slot"] < len(DECONVS) - 1:
                ev = net._event("bwd_branch%d" % L["slot"])

                def branch(L=L, ev=ev):
                    self.deconv_wgrad(L)
                    self.dgrad_into(L["conv"], self.branch_dy(L), L["src"], ws_tag="side")
                    net._record(ev, q.side)
                q.defer(branch)
                if not net.compose_head:
                    q.flush()
                self.early_dst[L["src"]] = ev
                self.early_layers.add(L["name"])

    def deconv(self, L):
        q = self.q
        if L["name"] in self.early_layers:
            return
        # the chain's contraction goes into its queue BEFORE the leaves that hang off the same gradient: the
        # second stream's queue is served first (priority) and its kernels fill every CU's LDS, so a chain
        # kernel enqueued behind them waited for the whole leaf sequence (r03 timeline: 214 us)
        q.mark_fork()
        self.dgrad_into(L["conv"], self.branch_dy(L), L["src"])
        q.run(lambda: self.deconv_wgrad(L))
        if self.side_filler is not None:
            q.run(self.side_filler)
            self.side_filler = None

    def conv(self, L):
        net, q, a, d, p, G = self.net, self.q, self.net.act, self.net.dact, self.net.params, self.net.grad
        c, dst = L["conv"], L["dst"]
        C = c.g.Cout
        if dst in self.bwd_ready:
            # dgamma / dbeta / coefficients were finalised inside the data-gradient call that stored d[dst]
            ops.bn_backward_apply_coef(d[dst], C, a[dst], net.bnstate[c.bn], c.M, C, True,
                                       self.bwd_ready.pop(dst).coef, d[dst])
        else:
            ops.bn_backward(d[dst], C, a[dst], net.bnstate[c.bn], c.M, C, True,
                            p.grad_view(G, c.bn + ".gamma"), p.grad_view(G, c.bn + ".beta"), d[dst])
        # the bias of a conv feeding a training-mode BN has gradient sum(dy) == 0 identically (BN removes
        # the mean); Keras' autograd returns rounding noise there -- the exact 0 stays in net.grad
        if L["name"] in self.batched_convs:
            # one launch for the block's stride-1 convolutions, issued when the LAST of their output gradients
            # (conv1's: the layers are walked back to front) is final
            if L["name"] in net.wgrad_batches:
                q.run(lambda: net.wgrad_batches[L["name"]][0].run(net.wgrad_ws))
        else:
            q.run(lambda: ops.conv_wgrad(
                c.g, a[L["src"]], d[dst], p.grad_view(G, c.wname), net.wgrad_ws,
                in_bn=net.bnstate[c.in_bn] if c.in_bn else None, flags=ops.IN_RELU if c.in_relu else 0))
        if L["name"] == "rpn1.conv0" and self.rpn_grads_ready is not None:
            lo = p.offsets["rpn1.conv0.kernel"][1]
            q.run(lambda: self.rpn_grads_ready(lo, p.n_theta), torch_ops=True)
        self.dgrad_into(c, d[dst], L["src"])
        if L["src"] == "fold":
            # back through Permute + Reshape, gated by the ReLU of the last middle block's Dense (:195)
            ops.fold_depth(d["fold"], d[net.fold_src], net.dprime, net.H * net.W, 64, inverse=True,
                           mask=a[net.fold_src])

    def mid(self, L):
        """A middle block: conv3d -> BN -> Dense(relu)."""
        net, q, a, d, p, G = self.net, self.q, self.net.act, self.net.dact, self.net.params, self.net.grad
        c, n, dn = L["conv"], L["name"], L["dense"]

        def dense_wg():
            ops.conv_wgrad(dn.g, a[n + ".y"], d[n + ".u"], p.grad_view(G, dn.wname), net.wgrad_ws,
                           in_bn=net.bnstate[dn.in_bn])
        # the Dense weight gradient (HBM-bound, 52 granules of LDS) finds no room beside three data-gradient
        # workgroups per CU and waited 474 us in the queue IN FRONT of the block's ring weight gradient: behind it
        # the ring kernel starts as soon as its gradient exists
        late_dense = L["src"] != "grid"
        # the Dense data gradient below reads both operands of the Dense weight gradient: it carries it
        # (lisec_conv_extras.dense_dw)
        carried = n not in self.fused_dense and n in net.dense_dw_slabs
        if carried:
            late_dense = False
        elif not late_dense:
            q.run(dense_wg)
        # Dense data gradient; its store also reduces the statistics of the BatchNormalization under it
        if n in self.fused_dense:
            msink = self.fused_dense.pop(n)    # done inside the data gradient of the block above (dgrad_into)
        else:
            msink = net._bwd_sink(c.bn, 64, c.M)
            ops.conv_forward(net.dgeom[dn.name], d[n + ".u"], net.packed_t[dn.name][0], d[n + ".z"],
                             bwd=(a[n + ".y"], net.bnstate[c.bn], False), sink=msink,
                             dense_dw=net.dense_dw_slabs[n] if carried else None)
            if carried:
                # the 8 MB slab sum finds no registers beside the Winograd workgroups (46 - 60 us in the step for 6 us of
                # work) and the second stream is in order: enqueued right here it held the block's weight gradient back;
                # nothing reads the result before the optimizer, so the three sums go behind the last weight gradient
                self.late_reduces.append(lambda: ops.dense_dw_reduce(net.dense_dw_slabs[n], p.grad_view(G, dn.wname)))
        if L["src"] == "grid":
            self.first_conv3d(L, msink)
            return
        ops.bn_backward_apply_coef(d[n + ".z"], 64, a[n + ".y"], net.bnstate[c.bn], c.M, 64, False, msink.coef,
                                   d[n + ".z"])
        # the weight gradient (second stream) is enqueued BEFORE the block's data gradient: measured 1 % faster
        # than the other order
        if c.name in net.wino_wgrad_ws:
            # Winograd-domain weight gradient (csrc/wino_wgrad.hip): 4 / 9 of the ring kernel's MFMAs
            q.run(lambda: ops.conv_wgrad_winograd(c.g, a[L["src"]], d[n + ".z"], p.grad_view(G, c.wname),
                                                  net.wino_wgrad_ws[c.name]))
        else:
            q.run(lambda: ops.conv_wgrad(c.g, a[L["src"]], d[n + ".z"], p.grad_view(G, c.wname), net.wgrad_ws))
        if late_dense:
            q.run(dense_wg)
        self.dgrad_into(c, d[n + ".z"], L["src"])

    def first_conv3d(self, L, msink):
        """The sparse first Conv3D.  The grid is a constant on the empty cells + V voxel rows: both gradients reduce to
        V-row contractions plus sums of dy over boundary-trimmed boxes (exact; csrc/sparse_grid.hip)."""
        net, a, p, sample = self.net, self.net.act, self.net.params, self.sample
        c, n = L["conv"], L["name"]
        dz = net.dact[n + ".z"]
        rows = (sample.coords, sample.info, self.rcap)
        dg = net.dgeom[c.name]
        dW = p.grad_view(net.grad, c.wname)
        # the apply pass of this block's BatchNormalization backward runs inside the line sums (one pass
        # over the 82 MB gradient instead of two)
        ops.tap_sums_bn(c.g, dz, a[n + ".y"], net.bnstate[c.bn], msink.coef, dz, net.mid1_S, net.tapsum_ws)
        ops.const_field_grads(p.view(c.wname), net.mid1_S, None, 27, 64, 64, g_all=net.g_all)
        vout, delta = net.vfe.saved_field("vout"), net.vfe.saved_field("delta")

        def sparse_wgrad():
            ops.conv_wgrad(dg, dz, delta, dW, net.wgrad_ws, transpose_out=True, rows=rows)
            ops.const_field_grads(None, net.mid1_S, vout, 27, 64, 64, dW=dW, cvec_row=sample.info,
                                  cvec_row_max=sample.cap)
        self.q.run(sparse_wgrad)
        ops.conv_forward(dg, dz, net.packed_t[c.name][0], net.dout_rows, rows=rows, queue=net.rows_queue)

    def finish(self):
        """The late reduces behind the last weight gradient, the VFE, and the join of the two streams."""
        net, q = self.net, self.q
        net._mark("bwd:before vfe")
        for fn in self.late_reduces:
            q.defer(fn)
        q.flush()
        net.vfe.backward(None, net.grad, dout_rows=net.dout_rows, g_all=net.g_all)
        net._mark("bwd:vfe done")
        q.join(net._event("bwd_join"))         # every weight gradient has landed before the optimizer reads G
        net._mark("bwd:joined")


class LisecNet:
    def __init__(self, nx, ny, nz, maxPoints, params=None, device=None, compose_head=True, compute_dtype="float32",
                 regularizers=None):
        """regularizers: {ParamStore name: (l1, l2)} (lisec_amd.regularizers.coefficients), the weight penalties of the
        training step (see _regularize); None or empty: no penalty, and not one launch more than before.
        compute_dtype: 'float32', or 'bfloat16' (the 'mixed_bfloat16' policy of lisec_amd.mixed_precision): the inference
        forward then runs the Conv3D blocks behind the first and the Conv2Ds of the RPN with bf16 operands
        (csrc/igemm_bf16.hip), and training is refused.
        compose_head: the three Conv2DTranspose branches and the 1x1 heads run as 16-channel contractions with composite
        kernels (csrc/head_fused.hip; exact by linearity, the (Ho,Wo,768) concat is never formed).  False keeps the
        layer-by-layer form (256-channel upsampling into the concat, then the 768 -> 16 heads) -- what the tests compare
        the collapsed form against."""
        if compute_dtype not in ("float32", "bfloat16"):
            raise ValueError(f"compute_dtype must be 'float32' or 'bfloat16', not {compute_dtype!r}")
        self.compute_dtype = compute_dtype
        self.device = device or _lib.require_gpu()
        self.compose_head = bool(compose_head)
        self.lib = _lib.load()
        if nx % 8 or ny % 8:
            raise ValueError("nx and ny must be multiples of 8 (three stride-2 RPN blocks)")
        self.H, self.W, self.D, self.T = nx, ny, nz, maxPoints
        self.dprime = fold_depth(nz)
        self.params = params if params is not None else ParamStore(self.device, dprime=self.dprime)
        if self.params.dprime != self.dprime:
            raise ValueError(f"variables are for a depth fold of {self.params.dprime}, nz={nz} folds to {self.dprime}")
        self.vfe = VFEStack(self.params, self.device)
        dev, f32 = self.device, torch.float32
        D, H, W = self.D, self.H, self.W
        self.act = {}          # name -> device tensor (raw conv outputs, mid outputs, grid, concat, head)
        self.bnstate = {}      # bn prefix -> float[4*C]
        self.layers = []

        def buf(name, *shape):
            self.act[name] = torch.empty(shape, dtype=f32, device=dev)
            return self.act[name]

        # the dense VFE output: only the dense form of the first Conv3D reads it (allocated on first use, 164 MB)
        self.grid_shape = (D, H, W, 64)
        # field form of the first Conv3D (csrc/field_conv.hip): sweeps with a voxel capacity (= min(points, cells)) up to
        # this never form the grid -- beyond ~40 % occupancy the dense contraction is the cheaper one
        # (LISEC_TUNING=field_conv=0 keeps the dense contraction for every sweep)
        self.field_conv = _lib.knob("field_conv", True)
        self.field_max_voxels = _lib.knob("field_max_voxels", 262144)
        self.field_ws = None
        self._used_field = False
        # ---- middle layers (model_training.py:236-238) ----------------------------------------
        d_in, prev = D, "grid"
        for i, (stride, pad) in enumerate(MID):
            d_out = (d_in + 2 * pad[0] - 3) // stride[0] + 1
            n = f"mid{i+1}"
            buf(n + ".y", d_out, H, W, 64)
            buf(n + ".u", d_out, H, W, 64)
            g = ops.geom(0, (d_in, H, W), (d_out, H, W), (3, 3, 3), stride, pad, 64, 64)
            self.layers.append(dict(kind="mid", name=n, src=prev, conv=ConvLayer(
                n + ".conv", g, n + ".conv.kernel", (27, 64, 64, 64 * 64, 64, 1), bias=n + ".conv.bias", bn=n + ".bn"),
                dense=ConvLayer(n + ".dense", ops.geom(0, (d_out, H, W), (d_out, H, W), (1, 1, 1), (1, 1, 1),
                                                       (0, 0, 0), 64, 64),
                                n + ".dense.kernel", (1, 64, 64, 0, 64, 1), in_bn=n + ".bn", out_relu=True)))
            d_in, prev = d_out, n + ".u"
        # Permute((2,3,4,1)) + Reshape (model_training.py:242-243): (D',H,W,64) -> (H,W,64*D'), channel c*D' + d.
        # D' = 1 (Constants.nz = 8): a view, nothing to do; otherwise one permuting copy ("fold") each way
        h, w, cin = H, W, 64 * d_in
        if d_in != 1:
            buf("fold", H, W, cin)
            self.fold_src, prev = prev, "fold"
        else:
            self.fold_src = None
        src, src_bn = prev, None
        Ho, Wo = H // 2, W // 2
        if not self.compose_head:
            buf("concat", Ho, Wo, 768)
        for b, (cout, q) in enumerate(RPN_BLOCKS):
            for j in range(q + 1):
                s = 2 if j == 0 else 1
                ho, wo = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
                n = f"rpn{b+1}"
                buf(f"{n}.y{j}", ho, wo, cout)
                g = ops.geom(0, (1, h, w), (1, ho, wo), (1, 3, 3), (1, s, s), (0, 1, 1), cin, cout)
                self.layers.append(dict(kind="conv", name=f"{n}.conv{j}", src=src, dst=f"{n}.y{j}", conv=ConvLayer(
                    f"{n}.conv{j}", g, f"{n}.conv{j}.kernel", (9, cin, cout, cin * cout, cout, 1),
                    bias=f"{n}.conv{j}.bias", bn=f"{n}.bn{j}", in_bn=src_bn, in_relu=src_bn is not None)))
                src, src_bn, h, w, cin = f"{n}.y{j}", f"{n}.bn{j}", ho, wo, cout
            k, s = DECONVS[b]
            pad = (k - s) // 2
            if (h * s, w * s) != (Ho, Wo):
                raise ValueError("deconv output does not match the concat map")
            if k == s:
                # kernel == stride: no overlap -> a 1x1 GEMM whose columns (tap, n) are pixel-shuffled on store
                g = ops.geom(0, (1, h, w), (1, h, w), (1, 1, 1), (1, 1, 1), (0, 0, 0), cin, k * k * 256,
                             out_stride=768, ps=s, ps_channels=256)
                pack = (1, cin, k * k * 256, 0, 1, cin)
            else:
                g = ops.geom(1, (1, h, w), (1, h * s, w * s), (1, k, k), (1, s, s), (0, pad, pad), cin, 256,
                             out_stride=768)
                pack = (k * k, cin, 256, 256 * cin, 1, cin)
            L = dict(kind="deconv", name=f"up{b+1}", src=src, slot=b, k=k, s=s, pad=pad, hw=(h, w),
                     cin=cin, conv=ConvLayer(f"up{b+1}", g, f"up{b+1}.kernel", pack,
                                             bias=f"up{b+1}.bias", in_bn=src_bn, in_relu=True))
            if self.compose_head:
                # the branch and the heads as ONE contraction to 16 channels: Wc[tap][c][j] = sum_n W[tap][n][c] H[256b+n][j]
                taps = k * k
                L["Wc"] = torch.empty(taps * cin * 16, dtype=f32, device=dev)
                if k == s:
                    # kernel == stride: a 1x1 contraction with columns (tap, j), pixel-shuffled into the head afterwards
                    gf = ops.geom(0, (1, h, w), (1, h, w), (1, 1, 1), (1, 1, 1), (0, 0, 0), cin, taps * 16)
                    L["wc_strides"] = (16, taps * 16)                # Wc[c][tap*16 + j]
                    fpack = (1, cin, taps * 16, 0, taps * 16, 1)
                    L["T"] = torch.empty((h * w, taps * 16), dtype=f32, device=dev)
                else:
                    gf = ops.geom(1, (1, h, w), (1, h * s, w * s), (1, k, k), (1, s, s), (0, pad, pad), cin, 16)
                    L["wc_strides"] = (cin * 16, 16)                 # Wc[tap][c][j]
                    fpack = (taps, cin, 16, cin * 16, 16, 1)
                    L["T"] = None                                    # written straight into the head map
                L["conv"] = ConvLayer(f"up{b+1}.fused", gf, None, fpack, in_bn=src_bn, in_relu=True)
                L["up_kernel"], L["up_bias"] = f"up{b+1}.kernel", f"up{b+1}.bias"
            self.layers.append(L)
        buf("head", Ho, Wo, 16)
        self.Ho, self.Wo = Ho, Wo
        self.head_geom = ops.geom(0, (1, Ho, Wo), (1, Ho, Wo), (1, 1, 1), (1, 1, 1), (0, 0, 0), 768, 16)
        # ---- packed weights + BN state + stats scratch ---------------------------------------------
        self.packed = {}
        max_parts = 1
        for L in self.layers:
            for key in ("conv", "dense"):
                if key in L:
                    c = L[key]
                    self.packed[c.name] = torch.empty(ops.packed_floats(c.pack[0], c.pack[1], c.pack[2]),
                                                      dtype=f32, device=dev)
                    if c.bn:
                        self.bnstate[c.bn] = torch.zeros(4 * c.g.Cout, dtype=f32, device=dev)
                        max_parts = max(max_parts, c.nmb * 2 * c.g.Cout)
        self.packed["head"] = torch.empty(ops.packed_floats(1, 768, 16), dtype=f32, device=dev)
        # Winograd F(2x2, 3x3) form (csrc/wino.hip) of the stride-1 3x3 contractions that fill the chip in it (>= 128 blocks of
        # 8 x 8 tiles x 64 channels: the Conv3D blocks behind the first and the stride-1 Conv2Ds of RPN block 1): 4 / 9 of the
        # multiplications.  LISEC_TUNING winograd: bit 0 = forward calls, bit 1 = data gradients of the Conv2Ds, bit 2 = data gradients of the Conv3D
        # blocks (their Dense(64) gradient then runs as a launch of its own), bit 3 = weight gradients of the Conv3D blocks
        # (csrc/wino_wgrad.hip); 0 keeps the direct kernels
        self.winograd = _lib.knob("winograd", 15)
        self.packed_wu, self.packed_wu_t = {}, {}
        for L in self.layers:
            c = L["conv"]
            g = c.g
            if L["kind"] == "deconv" or L["src"] == "grid" or not self.winograd:
                continue
            blocks = g.Do * ((g.Ho + 15) // 16) * ((g.Wo + 15) // 16) * ((g.Cout + 63) // 64)
            if blocks >= 128 and ops.winograd_supported(g, in_bn=c.in_bn is not None, flags=ops.IN_RELU if c.in_relu else 0):
                if self.winograd & 1:
                    self.packed_wu[c.name] = torch.empty(ops.winograd_packed_floats(g.KD, g.Cin, g.Cout), dtype=f32, device=dev)
                # data gradient: kept on the direct kernel where the Dense(64) gradient of the block below rides on its tile
                # (lisec_conv_extras.tail_w: the middle blocks) -- measured equal there, and the tail would cost a launch
                if (self.winograd & 2 and L["kind"] == "conv") or (self.winograd & 4 and L["kind"] == "mid"):
                    self.packed_wu_t[c.name] = torch.empty(ops.winograd_packed_floats(g.KD, g.Cout, g.Cin), dtype=f32,
                                                           device=dev)
        # bf16 packs of the layers the bf16 kernel runs in inference (a bf16 net only): the 3x3(x3) contractions behind the
        # first Conv3D.  The first Conv3D (field form), the Dense(64)s and the composed heads stay fp32
        self.packed_bf16 = {}
        if self.compute_dtype == "bfloat16":
            for L in self.layers:
                c = L["conv"]
                if L["kind"] != "deconv" and L["src"] != "grid":
                    self.packed_bf16[c.name] = torch.empty(ops.packed_bf16_bytes(c.pack[0], c.pack[1], c.pack[2]),
                                                           dtype=torch.uint8, device=dev)
        self.bf16_launches = 0                           # calls of the bf16 kernel so far (tests: the feature is on)
        self.head_w = torch.empty(768, 16, dtype=f32, device=dev)
        self.head_b = torch.empty(16, dtype=f32, device=dev)
        self.fused_bias = torch.empty(16, dtype=f32, device=dev)     # b' = head bias + the branch biases through H
        if self.compose_head:
            self._shuffle = ops.HeadShuffle(Ho, Wo, [(L["T"], L["s"]) for L in self.layers
                                                     if L["kind"] == "deconv" and L["T"] is not None])
        self.parts = torch.empty(max_parts, dtype=torch.float64, device=dev)
        self._sinks, self._bsinks = {}, {}
        # The second HIP stream.  Backward: weight gradients are leaves of the graph and run beside the BN-backward /
        # data-gradient chain (the RPN layers are too small to fill 256 CUs on their own).  Forward and backward: the
        # Conv2DTranspose branches of RPN blocks 1 and 2 (model_training.py:246,249) only meet the rest of the network at the
        # concat, so they run beside the next block's small convolutions instead of in front of them.
        # ROCm multiplexes same-priority streams onto a few hardware queues round-robin, so a plain second stream
        # can land on the main stream's queue (it does once RCCL has made its own streams) and then nothing
        # overlaps; a different priority level always gets its own hardware queue.
        # (Round 4: with GPU_MAX_HW_QUEUES=8 -- set when lisec_amd is imported -- a stream of the SAME priority gets a queue
        # of its own, and that is the faster arrangement: the high-priority queue was served first whenever it held a ready
        # packet, which starved the chain during the head phase; one rank through RCCL 5.13 -> 4.25 ms, one GPU +0.8 %.)
        self.side = torch.cuda.Stream(device=dev, priority=0)
        self.side_queue = _SideQueue(self, None, self.side)     # each pass names its main stream (begin)

        self._tail_ok = {}
        self._loss_descs = {}                            # LossSpec / DetectionLossSpec -> its descriptor (_loss_descriptor)
        self._early = None                               # (lo, OptimizerSpec) of the pending early_update()
        # mini-batches (train_micro_step): the gradient accumulator, shaped like theta, and the device float 1/b the
        # kernel that ends a batch reads; made by _batch_buffers() when a batch larger than 1 is first used
        self._acc = self._acc_scale = None
        self._acc_div = 1
        # weight averaging (OptimizerSpec.average): the average, shaped like theta, made by `average` when first used;
        # not live: it is to be started again as a copy of theta at its next use (Model.compile)
        self._average = None
        self._average_live = False
        self.dense_dw_slabs = {}                         # middle block -> slabs of lisec_conv_extras.dense_dw
        self._fwd_events = {}
        # a repack enqueued on the second stream is pending (_arm_repack, apply_gradients): the forward waits for
        # _pack_done before its first contraction, for _pack_late before the first reader of the rest
        self._pack_pending = self._late_pending = False
        self._pack_done = self._pack_late = None
        self._packed_version = -1
        self.params_version = 0
        self.state_version = 0
        self._folded = {}
        self._train_ready = False
        # optimizer iteration count: the device copy drives the learning-rate decay (lisec_sgd_nesterov_step_dev), so
        # that a captured step can be replayed; the host mirror is what save()/load_model() and the tests read
        self._iter_dev = torch.zeros(2, dtype=torch.int64, device=dev)
        self._iterations = 0
        # Nadam's momentum_cache (the product of its momentum schedule so far; 1 before the first step), next to the
        # iteration count: the Nadam kernels read it and the call that ends a step writes the step's product back
        self.momentum_cache = torch.ones(1, dtype=torch.float32, device=dev)
        # learning-rate descriptor (lisec_lr_schedule) of the OptimizerSpecs with device_lr, at a fixed address like the
        # iteration count; _sync_lr rewrites it, stream-ordered, when a step needs other contents
        self._lr = _DeviceDescriptor(dev)
        # the coefficient of the decoupled weight decay (OptimizerSpec.weight_decay; csrc/weight_decay.hip): a second
        # descriptor of the same type, written likewise; and the chunk tables of the decayed variables, made when a
        # selection is first used and kept for the net's life (recorded plans point at them):
        # {DecaySpec.variables: ops.ChunkTable}
        self._wd = _DeviceDescriptor(dev)
        self._decay_tables = {}
        # a layer-wise optimizer (LAMB; csrc/lamb.hip): the ops.LambTable per pair of exclusion lists, kept for the
        # net's life like the decay tables, and -- made with the first table, every table has the same rows -- the
        # per-chunk workspace and the trust ratios of the last update, one per trainable variable
        self._lamb_tables = {}
        self._lamb_ws = self._lamb_ratios = None
        # gradient clipping (OptimizerSpec.clip; csrc/grad_clip.hip): the table of every trainable variable (LAMB's
        # records, no exclusions), the per-chunk workspace, and the scales and norms of the last update, one per
        # variable (the global norm: slot 0), all made with the first clipped update and kept for the net's life;
        # _clip_kind is the kind of the last update that left norms ('norm' / 'global_norm'), for gradient_norms()
        self._clip_table = self._clip_ws = self._clip_scales = self._clip_norms = self._clip_kind = None
        # BatchNormalization recalibration (recalibrate_batchnorm; csrc/bn_recalibrate.hip): the table of the layers'
        # moving statistics and the fp64 accumulator, made when first used (bn_recal_table)
        self._bn_recal = None
        self.loss_out =torch.zeros(3, dtype=f32, device=dev)
        # the metrics of a LossSpec loss (lisec_head_loss), class output's first; fixed address, like loss_out
        self.metric_out = torch.zeros(2 * _lib.LOSS_MAX_METRICS, dtype=f32, device=dev)
        # [N_pos, N_neg] of a DetectionLossSpec loss (lisec_detection_loss); fixed address, like loss_out
        self.loss_counts = torch.zeros(2, dtype=torch.int64, device=dev)
        # [num0, den0, num1, den1, ...] of a DetectionLossSpec's metrics (lisec_detection_metrics); fixed address
        self.metric_pairs = torch.zeros(2 * _lib.DET_MAX_METRICS, dtype=torch.float64, device=dev)
        # weight regularizers (csrc/regularize.hip): the chunk table (an ops.ChunkTable; None without regularizers), the
        # per-chunk partials and the penalty of the step, at fixed addresses like loss_out; fixed for the net's life
        # (id(net) keys the recorded plans)
        self.regularizers = {n: (float(a), float(b)) for n, (a, b) in (regularizers or {}).items() if a != 0 or b != 0}
        # the bias of a convolution that feeds a training-mode BatchNormalization has an identically zero gradient, and
        # the backward pass never writes its slot of grad (_BackwardPass.conv): the penalty pass must store its term
        # there, or the slot would carry the terms of every step so far
        self.unwritten_grads = tuple(L["conv"].bias for L in self.layers
                                     if L["kind"] in ("mid", "conv") and L["conv"].bias and L["conv"].bn)
        rows = ops.reg_chunks(self.params, self.regularizers, unwritten=self.unwritten_grads)
        self._reg = None
        if rows:
            self._reg = ops.reg_table(rows, dev)
            self._reg_ws = ops.reg_workspace(len(rows), dev)
            self.reg_penalty = torch.zeros(1, dtype=torch.float64, device=dev)

    @property
    def regularized(self):
        """Does a step of this net add weight penalties (reg_penalty exists and the update passes over a chunk table)?"""
        return self._reg is not None

    @property
    def iterations(self):
        return self._iterations

    @iterations.setter
    def iterations(self, k):
        self._iterations = int(k)
        self._iter_dev.copy_(torch.tensor([int(k), 0], dtype=torch.int64))

    # ------------------------------------------------------------------------------------------------
    def _pack_all(self, after_main=None):
        """Repack theta into the kernels' [tap][K/4][N][4] layout (after every optimizer step)."""
        if self._packed_version == (self.params_version, self.params.version):
            if after_main is not None:
                after_main()
            return
        p = self.params
        if getattr(self, "_head_merge", None) is None:     # Keras-shaped head variables -> the merged (768,16) layout
            self._head_merge = ops.CopyTable([(p.view("cls.kernel")[0, 0], self.head_w[:, :2]),
                                              (p.view("reg.kernel")[0, 0], self.head_w[:, 2:]),
                                              (p.view("cls.bias"), self.head_b[:2]),
                                              (p.view("reg.bias"), self.head_b[2:])], self.device)
        self._head_merge.run()
        if getattr(self, "_pack_table", None) is None:
            entries, rest, late = [], [], []
            for L in self.layers:
                for key in ("conv", "dense"):
                    if key in L:
                        c = L[key]
                        (late if not c.wname else entries if L["kind"] == "mid" else rest).append(
                            ((p.view(c.wname) if c.wname else L["Wc"]), self.packed[c.name]) + tuple(c.pack))
            self._pack_table = ops.PackTable(entries, self.device)
            self._pack_table_rest = ops.PackTable(rest, self.device)
            self._pack_table_wc = ops.PackTable(late, self.device) if late else None

        def wino_packs(mid):
            for L in self.layers:
                c = L["conv"]
                if c.name in self.packed_wu and (L["kind"] == "mid") == mid:
                    g = c.g
                    ops.pack_weights_winograd(p.view(c.wname), g.KD, g.Cin, g.Cout, g.Cin * g.Cout, g.Cout, 1,
                                              out=self.packed_wu[c.name])
        # the kernels of the middle blocks first: the first contraction of the forward pass waits for these only (after_main
        # records that point when the repack runs early on the second stream: 6 small kernels, done before the VFE is -- with
        # every variable kernel in front of that point the main stream stood 22 us per step).  The RPN's kernels, the composite
        # kernels of the collapsed heads -- three compose launches in front of their pack -- and the transposed set follow;
        # the first Conv2D of the RPN, ~0.5 ms into the step, waits for all of them (_pack_late)
        self._pack_table.run()
        wino_packs(True)
        if after_main is not None:
            after_main()
        self._pack_table_rest.run()
        wino_packs(False)
        for L in self.layers:                            # (empty unless the net computes in bf16)
            c = L["conv"]
            if c.name in self.packed_bf16:
                ops.pack_weights_bf16(p.view(c.wname), *c.pack, out=self.packed_bf16[c.name])
        if self.compose_head:
            self._compose_all()
        if self._pack_table_wc is not None:
            self._pack_table_wc.run()
        if not self.compose_head:
            ops.pack_weights(self.head_w, 1, 768, 16, 0, 16, 1, out=self.packed["head"])
        self._packed_version = (self.params_version, self.params.version)

    def _compose_all(self):
        """Composite kernels of the three upsampling branches with the heads, and the composite bias (head_fused.hip)."""
        p = self.params
        bias_in = self.head_b
        for L in self.layers:
            if L["kind"] != "deconv":
                continue
            b, ts, cs = L["slot"], *L["wc_strides"]
            ops.head_compose(p.view(L["up_kernel"]), p.view(L["up_bias"]), self.head_w[256 * b:256 * (b + 1)], L["k"] * L["k"],
                             L["cin"], 256, L["Wc"], ts, cs, bias_in=bias_in, bias_out=self.fused_bias)
            bias_in = self.fused_bias

    def _fwd_sink(self, c):
        """BnSink of a conv layer's BatchNormalization: batch statistics summed and finalised inside the conv call."""
        s = self._sinks.get(c.bn)
        if s is None:
            p = self.params
            s = self._sinks[c.bn] = ops.BnSink(c.g.Cout, c.M, self.device, gamma=p.view(c.bn + ".gamma"),
                                               beta=p.view(c.bn + ".beta"), moving_mean=p.view(c.bn + ".moving_mean"),
                                               moving_var=p.view(c.bn + ".moving_variance"), unbiased=True,
                                               bnstate=self.bnstate[c.bn])
        return s

    def _bn_after(self, c, training):
        p = self.params
        C = c.g.Cout
        if training:
            # the statistics were finalised by the last workgroup of the conv call (lisec_bn_sink): nothing to launch
            self.state_version += 1               # moving statistics moved, bnstate holds batch statistics
        elif self._folded.get(c.bn) != (self.params_version, self.state_version, p.version):
            # inference: scale/shift from the moving statistics, folded once per weight version (not per sweep)
            ops.bn_fold(p.view(c.bn + ".gamma"), p.view(c.bn + ".beta"), p.view(c.bn + ".moving_mean"),
                        p.view(c.bn + ".moving_variance"), C, self.bnstate[c.bn])
            self._folded[c.bn] = (self.params_version, self.state_version, p.version)

    def _fold_inference(self):
        """Issues, on the current stream, every BatchNormalization fold (_bn_after) that is stale for the current weights
        and moving statistics: a forward(training=False) then launches none of its own (EvalStep)."""
        for L in self.layers:
            for key in ("conv", "dense"):
                c = L.get(key)
                if c is not None and c.bn:
                    self._bn_after(c, False)

    def _run_conv(self, c, x, out, training, ws_tag="main"):
        p = self.params
        flags = (ops.IN_RELU if c.in_relu else 0) | (ops.OUT_RELU if c.out_relu else 0)
        sink = self._fwd_sink(c) if (c.bn and training) else None
        if not training and c.name in self.packed_bf16:
            ops.conv_forward_bf16(c.g, x, self.packed_bf16[c.name], out, bias=p.view(c.bias) if c.bias else None,
                                  in_bn=self.bnstate[c.in_bn] if c.in_bn else None, flags=flags, ws_tag=ws_tag)
            self.bf16_launches += 1
        elif c.name in self.packed_wu:
            ops.conv_forward_winograd(c.g, x, self.packed_wu[c.name], out, bias=p.view(c.bias) if c.bias else None,
                                      in_bn=self.bnstate[c.in_bn] if c.in_bn else None, flags=flags, sink=sink)
        else:
            ops.conv_forward(c.g, x, self.packed[c.name], out, bias=p.view(c.bias) if c.bias else None,
                             in_bn=self.bnstate[c.in_bn] if c.in_bn else None, flags=flags | ops.SMALL_TILE, sink=sink,
                             ws_tag=ws_tag)
        if c.bn:
            self._bn_after(c, training)

    def _event(self, name):
        ev = self._fwd_events.get(name)
        if ev is None:
            ev = self._fwd_events[name] = self._new_event()
        return ev

    def _new_event(self):
        """Fork / join events: device-scope release, recorded and waited for through the library (lisec_event_record),
        so that a step plan sees them."""
        return _lib.DeviceEvent()

    @staticmethod
    def _record(ev, stream):
        ev.record(stream.cuda_stream)

    @staticmethod
    def _wait(ev, stream):
        ev.wait(stream.cuda_stream)

    def _mark(self, name):
        """Diagnostic (tools/phase_times.py): with self.phase_marks a dict, a timing event is recorded on the main stream
        here -- through the library, so that a step plan replays it -- and in-step phase durations can be read back
        WITHOUT a profiler (rocprofv3's kernel trace makes the host the bottleneck wherever many small kernels are launched
        and shows gaps that a plain run does not have)."""
        marks = getattr(self, "phase_marks", None)
        if marks is None:
            return
        ev = marks.get(name)
        if ev is None:
            ev = marks[name] = _lib.DeviceEvent(timing=True)
        ev.record(_lib.current_stream())

    def dense_grid(self, rewrite=True):
        """The dense (D,H,W,64) VFE output; rewrite: fill it from the last forward's per-voxel values (the field form
        of the first Conv3D never writes it)."""
        if "grid" not in self.act:
            self.act["grid"] = torch.empty(self.grid_shape, dtype=torch.float32, device=self.device)
        if rewrite:
            self.vfe.rewrite_grid(self.act["grid"])
        return self.act["grid"]

    def forward(self, sample, training=False):
        """sample: VoxelSample of one lidar sweep.  Returns (cls (1,Ho,Wo,2), reg (1,Ho,Wo,14)) device views."""
        if sample.grid_shape != (self.D, self.H, self.W) or sample.cfg.sampleSize != self.T:
            raise ValueError("voxel sample does not match the model's grid")
        if training:
            self._refuse_bf16_training()
        prev_pin = _lib.pin_stream(torch.cuda.current_stream().cuda_stream)   # one stream query for the whole schedule
        try:
            return self._forward(sample, training)
        finally:
            _lib.pin_stream(prev_pin)

    def _forward(self, sample, training):
        self._mark("step:begin")
        pending = self._pack_pending
        if pending and (self._packed_version != (self.params_version, self.params.version)):
            self._wait(self._pack_late, torch.cuda.current_stream())     # variables changed since the early repack
            self._pack_pending = pending = False
            self._late_pending = False
        if not pending:
            self._pack_all()
        a = self.act
        use_field = self._used_field = self.field_conv and sample.cap <= self.field_max_voxels
        if use_field:
            first = self.layers[0]["conv"]
            need = ops.conv_field_forward_workspace_bytes(first.g, sample.cap)
            if self.field_ws is None or self.field_ws.numel() < need:
                self.field_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                _lib.bump_alloc_generation()       # recorded step plans hold the old address
            self.vfe.forward(sample, training, dense=False)
        else:
            self.vfe.forward(sample, training, out=self.dense_grid(rewrite=False))
        self._mark("step:vfe done")
        if pending:
            # the repack of this step's weights was enqueued on the second stream right after the last optimizer step
            # and ran under this sweep's voxeliser and VFE; the first contraction is the first reader
            self._wait(self._pack_done, torch.cuda.current_stream())
            self._pack_pending = False
        side_used = False
        q = self.side_queue
        q.begin(torch.cuda.current_stream())
        self._mark("fwd:start")
        for L in self.layers:
            self._mark("fwd:before " + L["name"])
            if L["kind"] == "mid":
                n = L["name"]
                if L["src"] == "grid" and use_field:
                    c = L["conv"]
                    ops.conv_field_forward(c.g, self.vfe.saved_field("vout"), self.vfe.saved_field("delta"), sample,
                                           self.packed[c.name], a[n + ".y"], self.field_ws, bias=self.params.view(c.bias),
                                           sink=self._fwd_sink(c) if training else None)
                    self._bn_after(c, training)
                else:
                    self._run_conv(L["conv"], a[L["src"]], a[n + ".y"], training)
                self._run_conv(L["dense"], a[n + ".y"], a[n + ".u"], training)
            elif L["kind"] == "conv":
                if self._late_pending:
                    # first reader of a kernel repacked behind the middle blocks' (see _pack_all)
                    self._wait(self._pack_late, torch.cuda.current_stream())
                    self._late_pending = False
                if L["src"] == "fold":
                    ops.fold_depth(a[self.fold_src], a["fold"], self.dprime, self.H * self.W, 64)
                self._run_conv(L["conv"], a[L["src"]], a[L["dst"]], training)
            else:
                b = L["slot"]
                if self.compose_head:
                    # 16-channel contraction: straight into the head map (with the composite bias) or into the branch's
                    # (tap, j) columns, added to the head by the shuffle pass below
                    c = L["conv"]
                    dst = a["head"] if L["T"] is None else L["T"]

                    def run(ws_tag, c=c, L=L, dst=dst):
                        ops.conv_forward(c.g, a[L["src"]], self.packed[c.name], dst,
                                         bias=self.fused_bias if L["T"] is None else None, in_bn=self.bnstate[c.in_bn],
                                         flags=ops.IN_RELU, ws_tag=ws_tag)
                else:
                    def run(ws_tag, L=L, b=b):
                        self._run_conv(L["conv"], a[L["src"]], a["concat"][:, :, 256 * b:], training, ws_tag=ws_tag)
                if b < len(DECONVS) - 1:
                    # an upsampling branch that is not the last: beside the next block, on the second stream
                    q.mark_fork(self._event("fwd_fork%d" % b))
                    q.run(lambda: run("side"))
                    side_used = True
                else:
                    if self._late_pending:
                        # first reader on THIS stream of a kernel repacked late on the second one (composite kernels, and
                        # the transposed set the backward reads)
                        self._wait(self._pack_late, torch.cuda.current_stream())
                        self._late_pending = False
                    run("main")
        if self._late_pending:
            self._wait(self._pack_late, torch.cuda.current_stream())
            self._late_pending = False
        if side_used:
            q.join(self._event("fwd_join"))
        if self.compose_head:
            self._shuffle.run(a["head"])
        else:
            ops.conv_forward(self.head_geom, a["concat"], self.packed["head"], a["head"], bias=self.head_b)
        head = a["head"]
        return head[None, :, :, :2], head[None, :, :, 2:]

    # ------------------------------------------------------------------------------------------------
    # training: explicit backward schedule (what Keras' fit() derives by autograd, model_training.py:299)
    def _refuse_bf16_training(self):
        if self.compute_dtype != "float32":
            raise NotImplementedError("a bfloat16-compute network serves inference only: training in mixed precision is not "
                                      "implemented (build the network with compute_dtype='float32')")

    def _prepare_training(self):
        if self._train_ready:
            return
        dev, f32 = self.device, torch.float32
        p = self.params
        self.grad = torch.zeros_like(p.theta)
        self.velocity = torch.zeros_like(p.theta)     # the SGD momentum slot; the Adam slots are made by slot() when asked for
        self._slots = {"velocity": self.velocity}
        self.dact = {}
        for name, t in self.act.items():
            if name.endswith(".u") or name in ("concat", "head", "fold") or ".y" in name:
                self.dact[name] = torch.empty_like(t)
        self.packed_t = {}
        self.dgeom = {}
        ws_bytes = ops.wgrad_workspace_bytes(self.head_geom)
        Ho, Wo = self.Ho, self.Wo
        for L in self.layers:
            c = L["conv"]
            g = c.g
            ntaps = g.KD * g.KH * g.KW
            ws_bytes = max(ws_bytes, ops.wgrad_workspace_bytes(g))
            if L["kind"] == "deconv" and self.compose_head:
                # the 16-channel contraction's gradients: G = dL/dWc by the ordinary weight gradient, the data gradient with
                # the composite kernel transposed; dy is the head gradient itself or its (tap, j) columns (dT)
                k, sd, pad, (h, w), cin = L["k"], L["s"], L["pad"], L["hw"], L["cin"]
                taps = k * k
                L["G"] = torch.empty(taps * cin * 16, dtype=f32, device=dev)
                if k == sd:
                    L["dT"] = torch.empty_like(L["T"])
                    self.dgeom[c.name] = ops.geom(0, (1, h, w), (1, h, w), (1, 1, 1), (1, 1, 1), (0, 0, 0), taps * 16, cin)
                    spec = (1, taps * 16, cin, 0, 1, taps * 16)
                else:
                    L["dT"] = None
                    self.dgeom[c.name] = ops.geom(0, (1, Ho, Wo), (1, h, w), (1, k, k), (1, sd, sd), (0, pad, pad), 16, cin)
                    spec = (taps, 16, cin, cin * 16, 1, 16)
                self.packed_t[c.name] = (torch.empty(ops.packed_floats(spec[0], spec[1], spec[2]), dtype=f32, device=dev),
                                         spec)
            elif L["kind"] == "deconv":
                # data gradient of a transposed conv = plain strided conv over dY (K = out, N = in)
                k, sd, pad, (h, w), cin = L["k"], L["s"], L["pad"], L["hw"], L["cin"]
                ntaps = k * k
                self.dgeom[c.name] = ops.geom(0, (1, Ho, Wo), (1, h, w), (1, k, k), (1, sd, sd), (0, pad, pad),
                                              256, cin, in_stride=768)
                self.packed_t[c.name] = (torch.empty(ops.packed_floats(ntaps, 256, cin), dtype=f32, device=dev),
                                         (ntaps, 256, cin, 256 * cin, cin, 1))
                if k == sd:
                    # weight gradient with swapped roles: gather dY (stride s), contract against the input rows
                    L["wgeom"] = self.dgeom[c.name]
                    ws_bytes = max(ws_bytes, ops.wgrad_workspace_bytes(L["wgeom"]))
            else:
                self.dgeom[c.name] = ops.geom(1, (g.Do, g.Ho, g.Wo), (g.Di, g.Hi, g.Wi), (g.KD, g.KH, g.KW),
                                              (g.sd, g.sh, g.sw), (g.pd, g.ph, g.pw), g.Cout, g.Cin)
                self.packed_t[c.name] = (torch.empty(ops.packed_floats(ntaps, g.Cout, g.Cin), dtype=f32, device=dev),
                                         (ntaps, g.Cout, g.Cin, g.Cin * g.Cout, 1, g.Cout))
            if "dense" in L:
                d = L["dense"]
                ws_bytes = max(ws_bytes, ops.wgrad_workspace_bytes(d.g))
                self.dgeom[d.name] = d.g          # 1x1: the data gradient is the same geometry with W^T
                self.packed_t[d.name] = (torch.empty(ops.packed_floats(1, 64, 64), dtype=f32, device=dev),
                                         (1, 64, 64, 0, 1, 64))
                self.dact[L["name"] + ".z"] = torch.empty_like(self.act[L["name"] + ".y"])
        # first middle layer: exact sparse backward (csrc/sparse_grid.hip) -- never forms the 164 MB grid gradient
        first = self.layers[0]["conv"]
        self.mid1_S = torch.empty(27 * 64, dtype=f32, device=dev)
        self.g_all = torch.empty(64, dtype=f32, device=dev)
        self.tapsum_ws = torch.empty(ops.tap_sums_workspace_bytes(first.g), dtype=torch.uint8, device=dev)
        self.dout_rows = None
        self.rows_queue = torch.zeros(2, dtype=torch.int32, device=dev)      # tile counter of the row-list data gradient
        self.head_dgeom = ops.geom(0, (1, Ho, Wo), (1, Ho, Wo), (1, 1, 1), (1, 1, 1), (0, 0, 0), 16, 768)
        if not self.compose_head:
            self.packed_t["head"] = (torch.empty(ops.packed_floats(1, 16, 768), dtype=f32, device=dev), None)
        else:
            self._dshuffle = ops.HeadShuffle(Ho, Wo, [(L["dT"], L["s"]) for L in self.layers
                                                      if L["kind"] == "deconv" and L["dT"] is not None])
        self.head_dw = torch.empty(768, 16, dtype=f32, device=dev)
        self.up_db = torch.empty(768, dtype=f32, device=dev)
        # conv outputs that sit under a BatchNormalization(+ReLU), and how many layers read each of them
        self.bn_of, self.consumers = {}, {}
        nparts = 1
        for L in self.layers:
            self.consumers[L["src"]] = self.consumers.get(L["src"], 0) + 1
            if L["kind"] == "conv":
                self.bn_of[L["dst"]] = (L["conv"].bn, L["conv"].g.Cout)
        for L in self.layers:
            if L["src"] in self.bn_of:
                nparts = max(nparts, ops.num_mblocks_bwd(self.dgeom[L["conv"].name]) * 2 * self.bn_of[L["src"]][1])
            if "dense" in L:
                nparts = max(nparts, ops.num_mblocks_bwd(self.dgeom[L["dense"].name]) * 2 * 64)
        self.bparts = torch.empty(nparts, dtype=torch.float64, device=dev)
        self.head_db = torch.empty(16, dtype=f32, device=dev)
        # merged head gradients -> the Keras-shaped slots of the gradient buffer.  Made here and not in the pass: a table is
        # uploaded where it is made, which must not happen while a plan records -- _TrainingPlans prepares the net first
        G = self.grad
        self._head_split = ops.CopyTable([(self.head_dw[:, :2], p.grad_view(G, "cls.kernel")[0, 0]),
                                          (self.head_dw[:, 2:], p.grad_view(G, "reg.kernel")[0, 0]),
                                          (self.head_db[:2], p.grad_view(G, "cls.bias")),
                                          (self.head_db[2:], p.grad_view(G, "reg.bias"))], self.device)
        if not self.compose_head:
            self._up_bias_split = ops.CopyTable(
                [(self.up_db[256 * L["slot"]:256 * (L["slot"] + 1)], p.grad_view(G, L["conv"].bias))
                 for L in self.layers if L["kind"] == "deconv"], self.device)
        # the stride-1 convolutions of an RPN block (model_training.py:210-214) share ONE weight-gradient launch: maps of
        # 1 250 - 20 000 positions fill a fraction of the chip each, and as leaves of the backward pass they can wait for each
        # other (lisec_conv_wgrad_batched)
        self.wgrad_batches = {}
        for b in range(len(RPN_BLOCKS)):
            convs = [L for L in self.layers if L["kind"] == "conv" and L["name"].startswith(f"rpn{b+1}.conv")
                     and L["name"] != f"rpn{b+1}.conv0"]
            items = [(L["conv"].g, self.act[L["src"]], self.dact[L["dst"]], p.grad_view(self.grad, L["conv"].wname),
                      self.bnstate[L["conv"].in_bn], ops.IN_RELU, False) for L in convs]
            if 2 <= len(items) <= 6:
                batch = ops.WgradBatch(items)
                ws_bytes = max(ws_bytes, batch.workspace_bytes())
                self.wgrad_batches[convs[0]["name"]] = (batch, {L["name"] for L in convs})
        # zero-filled: the head of the workspace holds the arrival counters of the slab-combining kernels
        self.wgrad_ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        # weight gradients of the Conv3D blocks behind the first in the Winograd form (winograd bit 3): one slab workspace for
        # all of them (they run one after the other on the second stream)
        self.wino_wgrad_ws = {}
        if self.winograd & 8:
            mids = [L["conv"] for L in self.layers if L["kind"] == "mid" and L["src"] != "grid"
                    and ops.wgrad_winograd_supported(L["conv"].g)]
            if mids:
                shared = torch.empty(max(ops.wgrad_winograd_workspace_bytes(c.g) for c in mids), dtype=torch.uint8, device=dev)
                self.wino_wgrad_ws = {c.name: shared for c in mids}
        # Dense(64) weight gradients carried by the Dense data gradients (lisec_conv_extras.dense_dw): one slab buffer per
        # middle block -- the sum runs on the second stream, possibly after the next block's data gradient has started
        # writing its own
        self.dense_dw_slabs = {}
        nslabs = ops.dense_dw_slabs()
        for L in self.layers:
            if L["kind"] == "mid" and (L["conv"].M + 127) // 128 >= nslabs:
                self.dense_dw_slabs[L["name"]] = torch.empty(nslabs * 4096, dtype=torch.float32, device=dev)
        self._packed_t_version = -1
        self._train_ready = True

    def _bwd_sink(self, bn_name, C, n_rows):
        """BnSink of the backward of one BatchNormalization: (sum dz, sum dz*yhat) -> dgamma, dbeta, coefficients."""
        s = self._bsinks.get(bn_name)
        if s is None:
            p = self.params
            s = self._bsinks[bn_name] = ops.BnSink(C, n_rows, self.device, dgamma=p.grad_view(self.grad, bn_name + ".gamma"),
                                                   dbeta=p.grad_view(self.grad, bn_name + ".beta"))
        return s

    def _pack_all_t(self):
        if self._packed_t_version == (self.params_version, self.params.version):
            return
        p = self.params
        if self.compose_head and self._packed_version != (self.params_version, self.params.version):
            self._pack_all()                 # the composite kernels (Wc) are made there
        if getattr(self, "_pack_table_t", None) is None:
            entries = []
            for L in self.layers:
                for key in ("conv", "dense"):
                    if key in L:
                        c = L[key]
                        buf, spec = self.packed_t[c.name]
                        entries.append((p.view(c.wname) if c.wname else L["Wc"], buf) + tuple(spec))
            if not self.compose_head:
                entries.append((self.head_w, self.packed_t["head"][0], 1, 16, 768, 0, 1, 16))
            self._pack_table_t = ops.PackTable(entries, self.device)
        self._pack_table_t.run()
        for L in self.layers:
            c = L["conv"]
            if c.name in self.packed_wu_t:
                g = c.g                          # K = forward Cout, N = forward Cin, taps mirrored
                ops.pack_weights_winograd(p.view(c.wname), g.KD, g.Cout, g.Cin, g.Cin * g.Cout, 1, g.Cout, flip=True,
                                          out=self.packed_wu_t[c.name])
        self._packed_t_version = (self.params_version, self.params.version)

    def backward(self, y_cls, y_reg, loss="mse", grad_scale=1.0, rpn_grads_ready=None, side_filler=None, weights=None):
        """y_cls (Ho,Wo,2), y_reg (Ho,Wo,14): float32 device tensors.  Fills self.grad (layout of theta)
        and self.loss_out = [total, class, regression].  Must follow forward(training=True).
        loss: 'mse' (loss=['mse','mse'], the reference's) or 'smoothl1_ce' -- lisec_rpn_loss -- or a LossSpec (Keras losses,
        loss_weights and metrics: lisec_head_loss, which also fills self.metric_out[:loss.n_metrics]) or a
        DetectionLossSpec (the VoxelNet detection loss: lisec_detection_loss, which also fills self.loss_counts; its
        metrics: lisec_detection_metrics, into self.metric_pairs[:2 * loss.n_metrics]).
        weights: the sample weights of the sweep (see _loss_backward); None: the unweighted launches.
        side_filler: optional callable issued on the second stream behind the head-phase leaves, where that stream has
        nothing to do for ~200 us (the weight gradients of the last RPN block wait for its chain): independent work such as
        the NEXT sweep's voxelisation (PipelinedStep).
        rpn_grads_ready(lo, hi): optional hook, called (inside the second stream's context) as soon as the
        gradients of every RPN/head variable -- theta[lo:hi], 94 % of the parameters -- are final, while the
        middle layers and the VFE are still being differentiated: data parallelism starts its all-reduce there."""
        prev_pin = _lib.pin_stream(torch.cuda.current_stream().cuda_stream)
        try:
            return self._backward(y_cls, y_reg, loss, grad_scale, rpn_grads_ready, side_filler, weights)
        finally:
            _lib.pin_stream(prev_pin)

    def _loss_descriptor(self, spec):
        """The lisec_loss_cfg of a LossSpec / lisec_detection_loss_cfg of a DetectionLossSpec, built once per spec."""
        if spec not in self._loss_descs:
            self._loss_descs[spec] = spec.descriptor()
        return self._loss_descs[spec]

    def _metrics_descriptor(self, spec):
        """The lisec_detection_metrics_cfg of a DetectionLossSpec with metrics, built once per spec."""
        key = ("metrics", spec)
        if key not in self._loss_descs:
            self._loss_descs[key] = spec.metrics_descriptor()
        return self._loss_descs[key]

    def step_metrics(self, loss, weighted=False):
        """What the last training step left of the metrics of its loss, as the words fit() sums over an epoch (the metric
        words of loss_acc_len's layout): a LossSpec's fp32 values in metric_out, a DetectionLossSpec's fp64 pairs -- and
        those of a LossSpec whose step ran under sample weights -- in metric_pairs; None without metrics."""
        if _paired(loss, weighted) and loss.n_metrics:
            return self.metric_pairs[:2 * loss.n_metrics]
        if isinstance(loss, LossSpec) and loss.n_metrics:
            return self.metric_out[:loss.n_metrics]
        return None

    def _sample_weights(self, loss, weights):
        """The lisec_sample_weights of a weighted step: the weight tensors of both outputs (float32, device, one element
        or Ho*Wo; None: weight 1) and the weighted-metric bits of a LossSpec.  It holds their addresses."""
        bits = loss.weighted if isinstance(loss, LossSpec) else (0, 0)
        return ops.sample_weights(weights[0], weights[1], self.Ho * self.Wo, weighted_metrics=bits)

    def _loss_backward(self, loss, y_cls, y_reg, grad_scale, weights=None):
        """The loss of the head map against the targets into loss_out (a LossSpec: and its metrics into metric_out), its
        gradient into dact["head"].  A step loss is a legacy string (lisec_rpn_loss*), a LossSpec (lisec_head_loss*) or a
        DetectionLossSpec (lisec_detection_loss*, or lisec_detection_iou_loss* for the DetectionIoULossSpec among them; its
        counts into loss_counts, and lisec_detection_metrics, its metric pairs into metric_pairs): this, loss_eval(),
        step_metrics() and loss_acc_len() with its two readers (loss_acc_logs,
        loss_acc_split) are the only code that tells them apart.
        weights: None -- the launches above, as they always were -- or the sample weights of the sweep as a pair of float32
        device tensors / None (weight_form): the weighted entry of the same family, a legacy string as the LossSpec of its
        two terms (at unit weights its gradient is lisec_rpn_loss's, bit for bit); the metrics of a LossSpec then leave as
        pairs in metric_pairs, and the detection metrics stay unweighted."""
        head, dhead, M = self.act["head"], self.dact["head"], self.Ho * self.Wo
        if weights is not None:
            if not isinstance(loss, (LossSpec, DetectionLossSpec)):
                loss = self._legacy_spec(loss)
            sw = self._sample_weights(loss, weights)
            if isinstance(loss, LossSpec):
                ops.head_loss_weighted(self._loss_descriptor(loss), sw, head, y_cls, y_reg, M, dhead, self.loss_out,
                                       self.metric_pairs, grad_scale=grad_scale)
            else:
                ops.detection_loss_weighted(self._loss_descriptor(loss), sw, head, y_cls, y_reg, M, dhead, self.loss_out,
                                            self.loss_counts, grad_scale=grad_scale)
                if loss.n_metrics:
                    ops.detection_metrics(self._metrics_descriptor(loss), head, y_cls, y_reg, M, self.metric_pairs)
        elif isinstance(loss, LossSpec):
            ops.head_loss(self._loss_descriptor(loss), head, y_cls, y_reg, M, dhead, self.loss_out, self.metric_out,
                          grad_scale=grad_scale)
        elif isinstance(loss, DetectionLossSpec):
            run = ops.detection_iou_loss if isinstance(loss, DetectionIoULossSpec) else ops.detection_loss
            run(self._loss_descriptor(loss), head, y_cls, y_reg, M, dhead, self.loss_out, self.loss_counts,
                grad_scale=grad_scale)
            if loss.n_metrics:
                ops.detection_metrics(self._metrics_descriptor(loss), head, y_cls, y_reg, M, self.metric_pairs)
        else:
            ops.rpn_loss(head, y_cls, y_reg, M, LEGACY_LOSS_KINDS[loss], dhead, self.loss_out, grad_scale=grad_scale)

    def _legacy_spec(self, name):
        """The LossSpec a legacy string loss runs as under sample weights: its two terms, unit loss weights, no metrics."""
        from .losses import LEGACY
        LEGACY_LOSS_KINDS[name]
        return LossSpec(LEGACY[name])

    def loss_eval(self, loss, y_cls, y_reg, acc, weights=None):
        """Adds the loss (and the metrics of a LossSpec or DetectionLossSpec) of the head map against the targets to acc
        (float64, device, loss_acc_len(loss, weights is not None) long, in the layout stated there) and counts the sweep
        in it.  weights: as for _loss_backward."""
        head, M = self.act["head"], self.Ho * self.Wo
        if weights is not None:
            if not isinstance(loss, (LossSpec, DetectionLossSpec)):
                loss = self._legacy_spec(loss)
            sw = self._sample_weights(loss, weights)
            if isinstance(loss, LossSpec):
                ops.head_loss_weighted_eval(self._loss_descriptor(loss), sw, head, y_cls, y_reg, M, acc)
            else:
                ops.detection_loss_weighted_eval(self._loss_descriptor(loss), sw, head, y_cls, y_reg, M, acc)
                if loss.n_metrics:
                    ops.detection_metrics(self._metrics_descriptor(loss), head, y_cls, y_reg, M, acc[4:], accumulate=True)
        elif isinstance(loss, LossSpec):
            ops.head_loss_eval(self._loss_descriptor(loss), head, y_cls, y_reg, M, acc)
        elif isinstance(loss, DetectionLossSpec):
            run = ops.detection_iou_loss_eval if isinstance(loss, DetectionIoULossSpec) else ops.detection_loss_eval
            run(self._loss_descriptor(loss), head, y_cls, y_reg, M, acc)
            if loss.n_metrics:
                ops.detection_metrics(self._metrics_descriptor(loss), head, y_cls, y_reg, M, acc[4:], accumulate=True)
        else:
            ops.rpn_loss_eval(head, y_cls, y_reg, M, LEGACY_LOSS_KINDS[loss], acc)

    def _tail_supported(self, c, dst_name):
        """Can the Dense data gradient of block dst_name[:-2] ride on the direct data gradient of conv `c`?  (asked of the
        library once per layer: lisec_conv_plan_query refuses geometries the two-line w-halo kernel does not serve.  The
        Winograd form can carry it too (ops.conv_forward_winograd(tail=)), measured 0.5 % slower in the step than the
        separate HBM-bound Dense launch, which hides beside the MFMA-bound weight gradients of the second stream)"""
        ok = self._tail_ok.get(c.name)
        if ok is None:
            n = dst_name[:-2]
            Ln = {L["name"]: L for L in self.layers}.get(n)
            ok = False
            if Ln is not None and "dense" in Ln and self.dgeom[c.name].Cout == 64:
                cn, dn = Ln["conv"], Ln["dense"]
                try:
                    ops.conv_plan(self.dgeom[c.name], out_mask=self.act[dst_name],
                                  bwd=(self.act[n + ".y"], self.bnstate[cn.bn], False), sink=self._bwd_sink(cn.bn, 64, cn.M),
                                  tail=(self.packed_t[dn.name][0], self.dact[n + ".z"]))
                    ok = True
                except _lib.LisecError:
                    ok = False
            self._tail_ok[c.name] = ok
        return ok

    def _size_backward_scratch(self, sample):
        """(Re)sizes the scratch that depends on the cloud's capacity: the weight-gradient workspace and the row-list
        gradient rows of the first Conv3D."""
        first = self.layers[0]["conv"]
        need = ops.wgrad_workspace_bytes(self.dgeom[first.name], max(sample.cap, 1))
        if need > self.wgrad_ws.numel() or self.dout_rows is None or self.dout_rows.shape[0] < sample.cap + 1:
            torch.cuda.synchronize()
            if need > self.wgrad_ws.numel():
                self.wgrad_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
            self.dout_rows = torch.empty((sample.cap + 1, 64), dtype=torch.float32, device=self.device)
            _lib.bump_alloc_generation()           # recorded step plans hold the old addresses

    def _backward(self, y_cls, y_reg, loss, grad_scale, rpn_grads_ready, side_filler=None, weights=None):
        """The driver of the backward schedule: the loss, then the layers last to first (_BackwardPass), the leaves of
        the graph beside the chain on the second stream (_SideQueue)."""
        self._prepare_training()
        self._pack_all_t()
        sample = self.vfe._sample
        self._size_backward_scratch(sample)
        q = self.side_queue
        q.begin(torch.cuda.current_stream())
        bp = _BackwardPass(self, q, sample, rpn_grads_ready, side_filler)
        self._mark("bwd:start")
        self._loss_backward(loss, y_cls, y_reg, grad_scale, weights)
        bp.heads()
        bp.early_branches()
        step = {"deconv": bp.deconv, "conv": bp.conv, "mid": bp.mid}
        for L in reversed(self.layers):            # RPN blocks, then the middle blocks
            self._mark("bwd:before " + L["name"])
            step[L["kind"]](L)
        bp.finish()                                # ... and the VFE
        return self.loss_out

    def slot(self, name):
        """The optimizer slot `name` (one of SLOT_NAMES; see OptimizerSpec): a buffer shaped like theta, zero when first
        asked for, at a fixed address from then on (recorded step plans point at it)."""
        self._prepare_training()
        t = self._slots.get(name)
        if t is None:
            if name not in self.SLOT_NAMES:
                raise KeyError(f"unknown optimizer slot {name!r}")
            t = self._slots[name] = torch.zeros_like(self.params.theta)
            torch.cuda.synchronize(self.device)   # zero before any stream of the step (the second one included) uses it
        return t

    SLOT_NAMES = optimizer_table.SLOT_NAMES

    def slots(self):
        """Every slot made so far, by name (the SGD velocity always among them)."""
        self._prepare_training()
        return dict(self._slots)

    def _sync_lr(self, opt):
        """Makes the device descriptors (_DeviceDescriptor.sync) hold opt.lr_descriptor (nothing for a spec without
        device_lr) and the coefficient of opt's decoupled weight decay (nothing for a spec without decay).  A recorded
        step plan does not re-issue the copies; Model.fit calls this before the steps of an epoch."""
        if opt.device_lr:
            self._lr.sync(opt.lr_descriptor)
        if opt.weight_decay is not None:
            self._wd.sync(opt.weight_decay.descriptor)

    def decay_table(self, variables=None):
        """The chunk table (ops.ChunkTable) of the variables a DecaySpec selects (ops.decay_chunks: None, names and /
        or kinds), made once per selection.  KeyError: a name the network does not have; ValueError: a variable that is
        not trainable."""
        table = self._decay_tables.get(variables)
        if table is None:
            rows = ops.decay_chunks(self.params, variables)
            table = self._decay_tables[variables] = ops.decay_table(rows, self.device)
        return table

    def _decay(self, opt, lo, hi):
        """The decoupled weight decay of the variables in theta[lo:hi] (lo: a variable boundary), on the current
        stream: w <- w - wd_t*w at the device iteration count, which is read and left alone.  Nothing at all for a spec
        without decay."""
        if opt.weight_decay is None:
            return
        table = self.decay_table(opt.weight_decay.variables)
        first, count = table.span(lo, hi)
        self._wd.sync(opt.weight_decay.descriptor)
        ops.weight_decay(self.params.theta, table, count, self._wd.dev, self._iter_dev, first=first)

    def _regularize(self, lo, hi, accumulate=False, fold=False, grad=True):
        """The weight penalties of the variables in theta[lo:hi] (lo: a variable boundary), on the current stream: grad +=
        2*l2*w + l1*sign(w) on the weights as they are now, reg_penalty = P of the range (accumulate: += P), and with fold
        loss_out[0] = float32(loss_out[0] + reg_penalty) -- Keras adds the penalty to `loss` alone.  grad=False: P only.
        Nothing at all for a net without regularizers."""
        if not self.regularized:
            return
        first, count = self._reg.span(lo, hi)
        ops.regularize(self.params.theta, self.grad if grad else None, self._reg, count, self.reg_penalty,
                       self._reg_ws, first=first, accumulate=accumulate, loss_total=self.loss_out if fold else None)

    def penalty(self):
        """Enqueues P = sum over the regularised variables of l1*sum|w| + l2*sum w^2 of the weights as they are now into
        reg_penalty (device float64[1]) and returns it; None for a net without regularizers.  No gradient is touched."""
        if not self.regularized:
            return None
        self._regularize(0, self.params.n_theta, grad=False)
        return self.reg_penalty

    def _update(self, opt, lo, hi, advance, second=False):
        """One optimizer update of theta[lo:hi] on the device iteration count (advance: this call ends the step), by the
        entry of ops that the optimizer's record names: lr_t by value -- (lr, decay) are kernel arguments --, or with
        device_lr from the descriptor (a schedule, or a rate a callback may change).  With regularizers the penalty pass
        over the same range runs directly in front of it, on the same stream (second: the step's other part has stored
        its share of the penalty already); the call that ends the step folds the penalty into loss_out[0].  With a
        decoupled weight decay the decay pass follows it and the optimizer entry updates the decayed variables: the
        gradient term and the penalty are taken on the weights BEFORE the decay, as the regularization loss of Keras sits
        in the tape and tfa's decay follows it.  With clipping (opt.clip) the clip passes sit between the two: the
        regularised gradient is what is bounded, as Keras' penalty gradient is clipped with the rest, and the decay acts
        on the variable, not on the gradient."""
        self._regularize(lo, hi, accumulate=second, fold=advance)
        self._clip(opt, lo, hi)
        self._decay(opt, lo, hi)
        rec = opt.record
        entry, names, args = opt.launch
        if opt.device_lr:
            self._lr.sync(opt.lr_descriptor)
            rate = (self._lr.dev,)
        else:
            rate = (opt.lr,) if rec.schedule_decay else (opt.lr, opt.decay)
        cut, rows = slice(lo, hi), {}
        if rec.layerwise:
            # the entry gets the WHOLE buffers and the rows of the variables whose first float lies in theta[lo:hi]: the
            # tables hold whole variables, so none is split between the two parts of a step, and every chunk and variable
            # has its own slot of the workspace and of the ratio buffer -- the early part and the closing part together
            # leave what one launch over everything leaves
            table = self.lamb_table(*opt.lists)
            (first, n_chunks), (first_var, n_vars) = table.chunks.span(lo, hi), table.variables.span(lo, hi)
            cut, rows = slice(None), dict(table=table, ratios=self._lamb_ratios, workspace=self._lamb_ws, first=first,
                                          n_chunks=n_chunks, first_var=first_var, n_vars=n_vars)
        bufs = [None if name is None else self.slot(name)[cut] for name in names]
        if rec.scalar is not None:
            bufs.append(getattr(self, rec.scalar))
        getattr(ops, entry)(self.params.theta[cut], self.grad[cut], *bufs, *rate, *(getattr(opt, a) for a in args),
                            self._iter_dev, advance=advance, **rows)

    def clip_table(self):
        """The ops.LambTable of the clipping passes (ops.clip_chunks: every trainable variable), made once together
        with the workspace and the scale and norm buffers."""
        if self._clip_table is None:
            table = ops.lamb_table(*ops.clip_chunks(self.params), self.device)
            self._clip_ws = ops.clip_workspace(table.n_chunks, self.device)
            self._clip_scales = torch.ones(max(table.n_vars, 1), dtype=torch.float32, device=self.device)
            self._clip_norms = torch.zeros(max(table.n_vars, 1), dtype=torch.float32, device=self.device)
            self._clip_table = table
            torch.cuda.synchronize(self.device)   # whole before any stream of the step (the second one included) uses them
        return self._clip_table

    def _clip(self, opt, lo, hi):
        """The gradient clipping of the variables in theta[lo:hi] (lo, hi: variable boundaries), on the current stream,
        in place in net.grad.  'value' and 'norm' are per element or per variable: each part of a split update clips the
        variables of its own range, with slots of their own.  'global_norm' needs every gradient, so it only ever runs
        over everything (early_update makes no update with such a spec).  Nothing at all for a spec without clipping."""
        clip = opt.clip
        if clip is None:
            return
        table = self.clip_table()
        first, n_chunks = table.chunks.span(lo, hi)
        self._clip_kind = clip.kind
        if clip.kind == "value":
            ops.grad_clip_value(self.grad, clip.value, table=table, first=first, n_chunks=n_chunks)
            return
        bufs = dict(table=table, scales=self._clip_scales, norms=self._clip_norms, workspace=self._clip_ws)
        if clip.kind == "norm":
            first_var, n_vars = table.variables.span(lo, hi)
            ops.grad_clip_norm(self.grad, clip.value, first=first, n_chunks=n_chunks, first_var=first_var, n_vars=n_vars,
                               **bufs)
        else:
            if (first, n_chunks) != (0, table.n_chunks):
                raise RuntimeError("global_clipnorm needs the gradient of every variable: the update cannot be split")
            ops.grad_clip_global_norm(self.grad, clip.value, **bufs)

    def gradient_norms(self):
        """The L2 norms the last clipped update measured, before clipping: {variable name: norm} of every trainable
        variable for clipnorm, {'global': norm} for global_clipnorm (the regularised gradient where the net has
        regularizers).  One device-to-host copy behind everything enqueued so far; never made during a step.
        RuntimeError before the first clipped update, and when the last one clipped by value: it measures no norm.
        The counterpart of trust_ratios()."""
        if self._clip_kind not in ("norm", "global_norm"):
            raise RuntimeError("gradient_norms(): the last update did not clip by clipnorm or global_clipnorm")
        torch.cuda.current_stream().wait_stream(self.side)
        norms = self._clip_norms.cpu().tolist()
        if self._clip_kind == "global_norm":
            return {"global": norms[0]}
        return dict(zip(self._clip_table.names, norms))

    def lamb_table(self, exclude_from_weight_decay=None, exclude_from_layer_adaptation=None):
        """The ops.LambTable of a layer-wise optimizer with these exclusion lists (ops.lamb_chunks), made once per pair;
        the workspace and the ratio buffer are made with the first.  KeyError: a name the network does not have;
        ValueError: a variable that is not trainable."""
        key = (exclude_from_weight_decay, exclude_from_layer_adaptation)
        table = self._lamb_tables.get(key)
        if table is None:
            table = self._lamb_tables[key] = ops.lamb_table(*ops.lamb_chunks(self.params, *key), self.device)
            if self._lamb_ws is None:
                self._lamb_ws = ops.lamb_workspace(table.n_chunks, table.n_vars, self.device)
                self._lamb_ratios = torch.ones(max(table.n_vars, 1), dtype=torch.float32, device=self.device)
            torch.cuda.synchronize(self.device)   # whole before any stream of the step (the second one included) uses them
        return table

    def trust_ratios(self):
        """{variable name: r} of the last update of a layer-wise optimizer (LAMB): the trust ratio ||w|| / ||u|| each
        trainable variable's step was scaled by, 1.0 for a variable excluded from layer adaptation or with a zero norm.
        One device-to-host copy behind everything enqueued so far; never made during a step.  RuntimeError before the
        first such update."""
        if not self._lamb_tables:
            raise RuntimeError("trust_ratios(): no update by a layer-wise optimizer (optimizers.LAMB) has run")
        torch.cuda.current_stream().wait_stream(self.side)
        names = next(iter(self._lamb_tables.values())).names
        return dict(zip(names, self._lamb_ratios.cpu().tolist()))

    def early_update(self, lo, hi, opt=None):
        """`opt` (an OptimizerSpec; None: the reference's SGD-Nesterov) of theta[lo:hi] AHEAD of the rest of the step
        (backward's rpn_grads_ready hook, on the second stream): the RPN + head variables -- 94 % of the parameters -- have
        final gradients while the middle layers and the VFE are still being differentiated, and nothing in the rest of the
        backward pass reads theta itself (the contractions read the packed copies), so their 26 MB update runs under the
        MFMA-bound kernels instead of at the serial end of the step.  Elementwise, hence the same values whichever call
        updates an element -- for every optimizer of OptimizerSpec, as both calls read the same iteration count: this one
        on the second stream, which the main stream joins before apply_gradients() updates theta[:lo] and advances the
        count.  The update stays pending until that apply_gradients(), which must be given the same spec; a second early
        update before it raises RuntimeError.  A spec that clips by the GLOBAL norm needs every gradient before any
        variable moves: with it this call makes no update and leaves nothing pending, and apply_gradients() updates
        everything in one part behind the backward pass."""
        if self._early is not None:
            raise RuntimeError("early_update() while an early update is pending: apply_gradients() ends the step first")
        if lo % 4 or hi != self.params.n_theta:
            return
        opt = OptimizerSpec() if opt is None else opt
        if opt.clip is not None and opt.clip.kind == "global_norm":
            return
        if opt.average is not None:
            self.average                         # started from theta BEFORE any part of it is updated
        self._update(opt, lo, lo + (hi - lo) // 4 * 4, advance=False)
        self._early = (lo, opt)

    def apply_gradients(self, opt=None):
        """`opt` (an OptimizerSpec; None: optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True),
        model_training.py:295) of every variable that early_update() did not update in this step.  Raises RuntimeError,
        before any launch, when the pending early update was made with another spec.
        A net with regularizers: the update is made with grad + 2*l2*w + l1*sign(w), taken on the weights before the
        update, so after a step net.grad holds the REGULARISED gradient and loss_out[0] includes the penalty, which
        reg_penalty holds on its own.  backward() alone leaves the plain gradient, except in the slots it never writes
        (unwritten_grads: the conv biases in front of a training-mode BatchNormalization, whose gradient is identically
        0): those keep the term the last update stored, which the next update replaces, never adds to.
        A spec with clipping (opt.clip): the clip passes run behind the penalty pass and in front of the decay and the
        update, in place, so after a step net.grad holds the CLIPPED gradient (regularised where the net has
        regularizers), and gradient_norms() the norms measured before clipping."""
        opt = OptimizerSpec() if opt is None else opt
        hi = self.params.theta.numel()
        second = self._early is not None
        avg = self.average if opt.average is not None else None      # (made before the first launch of the update)
        if self._early is not None:
            lo, early_opt = self._early
            if (early_opt != opt or (opt.device_lr and bytes(early_opt.lr_descriptor) != bytes(opt.lr_descriptor))
                    or (opt.weight_decay is not None
                        and bytes(early_opt.weight_decay.descriptor) != bytes(opt.weight_decay.descriptor))):
                raise RuntimeError(f"apply_gradients(opt={opt}) after an early update with {early_opt}: the variables "
                                   f"would be updated by two different optimizers")
            hi = lo                              # the tail of the buffer was updated during the backward pass
            self._early = None
        # lr_t = lr / (1 + decay * iterations), derived on the device from its own iteration counter
        self._update(opt, 0, hi, advance=True, second=second)
        self._mark("step:updated")
        self._iterations += 1
        self.params_version += 1
        if self._train_ready:
            # both repacks (forward and transposed layouts, ~75 us) for the NEXT step go to the second stream now: they
            # only depend on this update, and the next sweep's voxeliser + VFE (~105 us) do not read them
            if self._pack_done is None:
                self._pack_fork, self._pack_done, self._pack_late = self._new_event(), self._new_event(), self._new_event()
            self._record(self._pack_fork, torch.cuda.current_stream())
            self._wait(self._pack_fork, self.side)
            pin = _lib.pin_stream(self.side.cuda_stream)
            try:
                self._pack_all(after_main=lambda: self._record(self._pack_done, self.side))
                self._pack_all_t()
                if avg is not None:
                    # the averaging pass, behind the repacks on the second stream: off the critical path (nothing reads
                    # the average during training), behind the update that advanced the count (state_bias -1), and in
                    # front of _pack_late, which every later writer of theta is ordered behind -- the next early update
                    # through this stream, the next apply_gradients through the forward's wait for _pack_late
                    ops.weight_average(self.params.theta, avg, opt.average.descriptor, self._iter_dev, state_bias=-1)
            finally:
                _lib.pin_stream(pin)
            self._record(self._pack_late, self.side)
            self._pack_pending = True
            self._late_pending = True

    @property
    def average(self):
        """The weight average (OptimizerSpec.average): a buffer shaped like theta that holds a copy of theta when it is
        made -- as a tfa slot starts at the variable's value -- and when it is first used after Model.compile; at a fixed
        address from then on (recorded step plans point at it)."""
        self._prepare_training()
        if not self._average_live:
            torch.cuda.current_stream().wait_stream(self.side)
            if self._average is None:
                self._average = self.params.theta.clone()
            else:
                self._average.copy_(self.params.theta)
            self._average_live = True
            torch.cuda.synchronize(self.device)   # whole before any stream of the step (the second one included) uses it
        return self._average

    def restart_average(self):
        """The average starts again as a copy of theta at its next use (a fresh optimizer: Model.compile)."""
        self._average_live = False

    def _exchange_average(self, swap):
        if self._early is not None:
            raise RuntimeError("the variables cannot be exchanged with their average while an early update is pending: "
                               "apply_gradients() ends the step first")
        avg = self.average
        # behind the repack and the averaging pass that the last update left pending on the second stream
        torch.cuda.current_stream().wait_stream(self.side)
        if swap:
            ops.weight_swap(self.params.theta, avg)
        else:
            self.params.theta.copy_(avg)
        self.params_version += 1
        self.params.touch()                       # the packed and transposed copies, the folds, the composed head, bf16
        if self._pack_done is not None:
            self._arm_repack()                    # a recorded step that follows waits for these events

    def swap_average(self):
        """theta <-> average BY CONTENT (lisec_weight_swap), on the current stream: recorded step plans hold both
        addresses, so the buffers themselves never change places.  Everything keyed on the variables' version -- the
        packed and transposed copies, the folded inference weights, the composed head, the bf16 packs -- is made again
        from the new theta, and the repack events are armed again for a recorded step that follows.  Two swaps restore
        both buffers bit for bit.  RuntimeError while an early update is pending."""
        self._exchange_average(True)

    def assign_average(self):
        """theta <- average (the average is kept); otherwise as swap_average()."""
        self._exchange_average(False)

    def bn_recal_table(self):
        """(ops.BnRecalTable, accumulator) of recalibrate_batchnorm: one record per BatchNormalization layer -- the
        offsets of its moving statistics in params.state (ParamStore.offsets), its channels, and the coefficient of
        the finaliser that updates them (the VFE kernel for vfe1 / vfe2 / fcn, a conv sink for the rest) -- and the
        float64 accumulator of three planes.  Made once."""
        if self._bn_recal is None:
            table = ops.bn_recal_table(ops.bn_recal_rows(self.params))
            self._bn_recal = (table, ops.bn_recal_acc(table, self.device))
        return self._bn_recal

    def recalibrate_batchnorm(self, samples, statistics="mean", dp=None):
        """Replaces every BatchNormalization layer's moving_mean / moving_variance by statistics of the CURRENT variables
        over the given sweeps (VoxelSamples), as torch.optim.swa_utils.update_bn does with momentum=None: the buffer of
        the moving statistics is zeroed, each sweep runs the ordinary forward(training=True) -- whose finalisers then
        leave batch * (1 - momentum) there -- and one launch per sweep adds it to fp64 sums (csrc/bn_recalibrate.hip).
        statistics 'mean': mean of the sweeps' means, mean of the sweeps' variances (update_bn's rule; the conv layers'
        variances Bessel-corrected as training corrects them); 'pooled': the variance of the sweeps' means is added
        ("precise BN").  Every sweep weighs the same.  dp (a DataParallel): rank r takes samples[r::world], the sums are
        all-reduced, and every rank ends with the same statistics.
        ValueError before any launch: no sweep, an unknown `statistics`.  RuntimeError while an early update is pending;
        NotImplementedError for a bfloat16-compute network.  Any exception inside (a sweep of another grid, ...) puts
        the moving statistics back as they were.  Eager, on the current stream.  Nothing of training moves: theta, the
        optimizer slots, the iteration counts, params_version and the weight average keep their bits; only bnstate and
        the activations are overwritten, which every forward rewrites before it reads them.  Sweeps no larger than the
        training sweeps grow no workspace, so a recorded training step stays valid (_lib.alloc_generation())."""
        samples = list(samples)
        ops.bn_statistics(statistics)
        if not samples:
            raise ValueError("recalibrate_batchnorm needs at least one sweep")
        if self._early is not None:
            raise RuntimeError("the BatchNormalization statistics cannot be recalibrated while an early update is "
                               "pending: apply_gradients() ends the step first")
        self._refuse_bf16_training()
        table, acc = self.bn_recal_table()
        state = self.params.state
        own = samples if dp is None else samples[dp.rank::dp.world]
        keep = state.clone()
        done = False
        try:
            state.zero_()
            acc.zero_()
            for sample in own:
                self.forward(sample, training=True)
                ops.bn_recalibrate_take(state, table, acc)
            if dp is not None:
                dp.sum_(acc)
            ops.bn_recalibrate_finish(state, table, acc, len(samples), statistics)
            done = True
        finally:
            if not done:
                state.copy_(keep)
            self.state_version += 1               # the inference folds are stale either way (bnstate was overwritten)

    def _arm_repack(self):
        """Repacks the variables now, on the current stream, and arms the two events the forward of a recorded step waits
        for (a step plan holds no repack of its own: the update of the step before left one pending)."""
        self._pack_pending = self._late_pending = False
        self._pack_all()
        self._pack_all_t()
        self._record(self._pack_done, torch.cuda.current_stream())
        self._record(self._pack_late, torch.cuda.current_stream())
        self._pack_pending = self._late_pending = True

    def _replayed(self):
        """Host bookkeeping of one replayed step plan: the update advanced the iteration count and moved theta, and the plan
        also repacked theta for the next step."""
        self._iterations += 1
        self.params_version += 1
        self.state_version += 1
        self._packed_version = self._packed_t_version = (self.params_version, self.params.version)
        self._pack_pending = self._late_pending = True

    def _replayed_micro(self):
        """Host bookkeeping of one replayed plan of a micro-step that only accumulates: no update, so the iteration
        count, params_version and the packed copies stand; the BatchNormalization statistics moved.  The plan's forward
        waited for the pack events of the last update, which stay signalled, and the next plan's forward will again."""
        self.state_version += 1
        self._pack_pending = self._late_pending = True

    # ------------------------------------------------------------------------------------------------
    # mini-batches: fit(batch_size=B) as B sweeps at batch 1 whose gradients are averaged before ONE update
    BATCH_POSITIONS = ("single", "first", "middle", "last")
    _ACC_MODE = {"first": _lib.ACC_BEGIN, "middle": _lib.ACC_ADD, "last": _lib.ACC_END}

    def _batch_buffers(self):
        """The gradient accumulator (zero when first asked for) and the device divisor (1), at fixed addresses from
        then on: recorded step plans point at them."""
        self._prepare_training()
        if self._acc is None:
            self._acc = torch.zeros_like(self.params.theta)
            self._acc_scale = torch.ones(1, dtype=torch.float32, device=self.device)
            self._acc_div = 1
            torch.cuda.synchronize(self.device)   # zero before any stream of the step (the second one included) uses it
        return self._acc

    def set_batch_divisor(self, b):
        """Makes the device divisor hold float32(1) / float32(b) for the batch that starts now: a fill on the current
        stream, behind every step already enqueued, when b differs from the last one written (as _sync_lr, a recorded
        plan does not re-issue it)."""
        self._batch_buffers()
        b = int(b)
        if b < 1:
            raise ValueError(f"a batch holds at least one sweep, not {b}")
        if b != self._acc_div:
            self._acc_scale.fill_(float(np.float32(1.0) / np.float32(b)))
            self._acc_div = b

    def _accumulate(self, lo, hi, mode):
        ops.grad_accumulate(self.grad[lo:hi], self._acc[lo:hi], mode, self._acc_scale)

    def train_micro_step(self, sample, y_cls, y_reg, position, loss="mse", allreduce=None, opt=None, side_filler=None,
                         weights=None):
        """Sweep `position` ('first', 'middle' or 'last'; 'single': train_step, a batch of one) of a mini-batch whose
        divisor set_batch_divisor() wrote: the forward (batch statistics of THIS sweep; the moving statistics move once
        per sweep, in order) and the backward of train_step, unchanged, then
          first / middle   acc = grad / acc += grad (lisec_grad_accumulate), and nothing else: no penalty, no update,
                           no iteration count, no repack, no gradient exchange;
          last             grad = (acc + grad) * (1/b), the mean in sweep order, and then everything train_step does behind
                           its backward, once: the data-parallel exchange, the penalty pass, the update, iterations += 1,
                           the repack for the next forward.
        The overlap of train_step is kept: the RPN + head tail of theta has final gradients at backward's
        rpn_grads_ready hook, so its pass -- and, in the last sweep, its early update or the start of its exchange --
        runs there on the second stream, under the rest of the backward; the head of theta follows the join.
        The slots of grad no backward pass writes (unwritten_grads) go through the passes like any other: they hold 0,
        or the term the last regularised update stored, which the penalty pass of this batch's update REPLACES (it
        stores into LISEC_REG_GRAD_IS_ZERO chunks), so a regularised bias gets its term once per update."""
        if position == "single":
            return self.train_step(sample, y_cls, y_reg, loss=loss, allreduce=allreduce, opt=opt, side_filler=side_filler,
                                   weights=weights)
        if position not in self._ACC_MODE:
            raise ValueError(f"position must be one of {self.BATCH_POSITIONS}, not {position!r}")
        self._batch_buffers()
        if opt is not None and opt.average is not None:
            self.average                           # made before the first launch of a step that averages
        mode, last, n = self._ACC_MODE[position], position == "last", self.params.n_theta
        bucketed = allreduce is not None and hasattr(allreduce, "start_tail")
        head = [n]                                 # where the range the hook has served starts

        def tail(lo, hi):
            if lo % 4 or hi != n:
                return
            self._accumulate(lo, hi, mode)
            head[0] = lo
            if last and bucketed:
                allreduce.start_tail(self.grad, lo, hi)
            elif last and allreduce is None:
                self.early_update(lo, hi, opt=opt)

        self.forward(sample, training=True)
        self.backward(y_cls, y_reg, loss=loss, side_filler=side_filler, rpn_grads_ready=tail, weights=weights)
        self._accumulate(0, head[0], mode)
        if last:
            if bucketed:
                allreduce.finish(self.grad)
            elif allreduce is not None:
                allreduce(self.grad)
            self.apply_gradients(opt=opt)
        return self.loss_out

    @staticmethod
    def batch_positions(b):
        """The positions of the b sweeps of one batch, in order."""
        return ["single"] if b == 1 else ["first"] + ["middle"] * (b - 2) + ["last"]

    def train_batch(self, samples, y_cls, y_reg, loss="mse", allreduce=None, opt=None, weights=None):
        """One update on the mean gradient of len(samples) sweeps (eager): y_cls[i], y_reg[i] are the targets of
        samples[i].  Returns [total, class, regression] of the batch as a float64 device tensor: the mean of the sweeps'
        losses, the total plus the weight penalty P once.  net.loss_out holds the last sweep's."""
        b = len(samples)
        if b < 1:
            raise ValueError("train_batch needs at least one sweep")
        if b > 1:
            self.set_batch_divisor(b)
        tot = torch.zeros(3, dtype=torch.float64, device=self.device)
        for k, (s_, yc, yr, pos) in enumerate(zip(samples, y_cls, y_reg, self.batch_positions(b))):
            tot += self.train_micro_step(s_, yc, yr, pos, loss=loss, allreduce=allreduce, opt=opt,
                                         weights=None if weights is None else weights[k])
        if self.regularized and b > 1:
            tot[0] += (b - 1) * self.reg_penalty[0]     # the last sweep's total holds P once; the mean keeps it whole
        return tot / b

    def train_step(self, sample, y_cls, y_reg, loss="mse", allreduce=None, opt=None, side_filler=None, weights=None):
        """One fit() step at batch_size=1: forward (batch statistics) + backward + the update by `opt` (an OptimizerSpec;
        None: the reference's SGD-Nesterov).  side_filler: see backward().
        allreduce: optional data-parallel gradient average -- with start_tail (parallel._BucketedAverage) in two buckets,
        otherwise a callable(grad) run after the backward pass.
        opt.average (an AverageSpec): one averaging pass over theta follows the update, on the second stream behind the
        repacks (apply_gradients); the update itself is untouched.
        weights: the sample weights of the sweep, a pair of float32 device tensors / None (one element: the sweep's
        weight; Ho*Wo: one per cell); None: the unweighted step."""
        if opt is not None and opt.average is not None:
            self.average                           # made before the first launch of a step that averages
        self.forward(sample, training=True)
        if allreduce is not None and hasattr(allreduce, "start_tail"):
            # two buckets: the RPN + head gradients (the tail of theta) are reduced under the rest of the backward
            self.backward(y_cls, y_reg, loss=loss, side_filler=side_filler, weights=weights,
                          rpn_grads_ready=lambda lo, hi: allreduce.start_tail(self.grad, lo, hi))
            allreduce.finish(self.grad)
        elif allreduce is not None:
            self.backward(y_cls, y_reg, loss=loss, side_filler=side_filler, weights=weights)
            allreduce(self.grad)
        else:
            # one rank: the RPN + head variables are updated under the rest of the backward
            self.backward(y_cls, y_reg, loss=loss, side_filler=side_filler, weights=weights,
                          rpn_grads_ready=lambda lo, hi: self.early_update(lo, hi, opt=opt))
        self.apply_gradients(opt=opt)
        return self.loss_out


class StalePlanError(RuntimeError):
    """A recorded step plan holds raw addresses of buffers that an eager call has since reallocated."""


class _StepPlans:
    """What everything that records step plans shares (RecordedStep, PipelinedStep, EvalStep): `nbuf` sets of padded
    (points, targets) buffers and the staging of a sweep into one (_load), the recording of a callable's launches as one
    more plan (_record), the checks in front of a replay (stream, allocation generation) and the plans' release."""

    PAD = 1.0e6          # metres: floor(1e6 / 0.5) is far beyond maxVoxelX, the point is dropped like any other outlier

    def __init__(self, net, voxelizer, capacity, nbuf, dtype, loss, wform=None):
        self.net, self.vox, self.capacity, self.loss = net, voxelizer, int(capacity), loss
        self.lib = _lib.load()
        self.plans, self.launches, self.alloc_gen = [], 0, None
        dev = net.device
        self.points = [torch.full((self.capacity, 3), self.PAD, dtype=dtype, device=dev) for _ in range(nbuf)]
        self.ycls = [torch.zeros((net.Ho, net.Wo, 2), dtype=torch.float32, device=dev) for _ in range(nbuf)]
        self.yreg = [torch.zeros((net.Ho, net.Wo, 14), dtype=torch.float32, device=dev) for _ in range(nbuf)]
        # a weighted plan (wform: weight_form's pair): per buffer set one weight buffer per weighted output, (1,) for
        # the sweep's weight or (Ho, Wo) for the map, which the recorded weighted loss launches read when they run
        self.wform = wform
        self.weights = None
        if wform is not None:
            shape = {"sweep": (1,), "cell": (net.Ho, net.Wo)}
            self.weights = [tuple(None if f is None else torch.ones(shape[f], dtype=torch.float32, device=dev)
                                  for f in wform) for _ in range(nbuf)]
        self.stream_handle = torch.cuda.current_stream().cuda_stream

    def _record(self, enqueue):
        """Runs enqueue() eagerly while its launches and event edges are recorded as one more plan."""
        plan = ctypes.c_void_p()
        _lib.check(self.lib.lisec_step_plan_create(ctypes.byref(plan)))
        self.plans.append(plan)
        _lib.check(self.lib.lisec_step_plan_begin(plan))
        try:
            enqueue()
        finally:
            _lib.check(self.lib.lisec_step_plan_end(plan))
        self.launches = self.lib.lisec_step_plan_size(self.plans[0])

    def _seal(self):
        """Ends the constructor: everything it enqueued is done, and the plans hold the addresses of this generation."""
        torch.cuda.synchronize(self.net.device)
        self.alloc_gen = _lib.alloc_generation()

    def _check_stream(self):
        if torch.cuda.current_stream().cuda_stream != self.stream_handle:
            raise RuntimeError(f"a {type(self).__name__} replays on the stream it was recorded on: make that stream current")

    def _check_fresh(self):
        if self.alloc_gen != _lib.alloc_generation():
            raise StalePlanError(
                f"this {type(self).__name__} was recorded before a workspace of the network / VFE / voxeliser was "
                "reallocated (an eager call on a larger sweep or grid): replaying it would write through freed "
                "addresses.  Record a new one (Model.fit and Model.evaluate do so by themselves).")

    def _load(self, j, points, ycls, yreg, weights=None):
        """Stages one sweep into buffer set j: points (n <= capacity, >= 3 columns; device or host tensor / numpy), targets
        (Ho,Wo,2|14) -- or `points` an object with stage_into(points, y_cls, y_reg) -> n that fills the buffers itself.
        weights: the sweep's sample weights in the form the plan was recorded for (weight_form); ValueError otherwise."""
        self._check_stream()
        self._load_weights(j, weights)
        stage = getattr(points, "stage_into", None)
        if stage is not None:
            # an item of a Sequence that makes its sweep on the device (augment.AugmentedSweeps): its kernels write the
            # points and both target maps of this buffer set themselves, on this stream, in front of the replay
            n = stage(self.points[j], self.ycls[j], self.yreg[j])
            if n < self.capacity:
                self.points[j][n:].fill_(self.PAD)
            draw = getattr(points, "draw", None)
            if draw is not None:
                # the per-voxel subsample of this item (a subsample='random' voxeliser): (seed, item, epoch) go into
                # the draw words of THIS buffer set's sample, which the recorded voxeliser launches read when they run
                seed, item, epoch = draw
                self.vox.set_draw(self.samples[j], item, epoch, seed=seed)
            return
        pts = torch.as_tensor(points)
        n = int(pts.shape[0])
        if n > self.capacity:
            raise ValueError(f"sweep of {n} points exceeds the recorded capacity {self.capacity}")
        self.points[j][:n].copy_(pts[:, :3], non_blocking=True)
        if n < self.capacity:
            self.points[j][n:].fill_(self.PAD)
        self.ycls[j].copy_(torch.as_tensor(ycls).reshape(self.ycls[j].shape), non_blocking=True)
        self.yreg[j].copy_(torch.as_tensor(yreg).reshape(self.yreg[j].shape), non_blocking=True)

    def _load_weights(self, j, weights):
        got = None if weights is None else tuple(None if w is None else ("sweep" if torch.as_tensor(w).numel() == 1
                                                                         else "cell") for w in weights)
        if got != self.wform:
            raise ValueError(f"this {type(self).__name__} was recorded for sample weights of the form {self.wform}, the "
                             f"sweep brings {got}")
        if weights is not None:
            for buf, w in zip(self.weights[j], weights):
                if buf is not None:
                    buf.copy_(torch.as_tensor(w, dtype=torch.float32).reshape(buf.shape), non_blocking=True)

    def close(self):
        if self.plans:
            torch.cuda.synchronize(self.net.device)
            for plan in self.plans:
                self.lib.lisec_step_plan_destroy(plan)
            self.plans = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TrainingPlans(_StepPlans):
    """What RecordedStep and PipelinedStep share: one voxel sample and one step plan per buffer set, the eager warm-up
    and recording steps (LisecNet.train_step), the replay and its bookkeeping.  The two differ in the number of sets, in
    where the step of buffer set j voxelises its sweep (_voxelise(j) issues it, or returns it as the side_filler of the
    backward pass) and in how a fit() epoch drives them: fit_step(sweep, st, steps) is step st of an epoch of `steps`
    steps, sweep(k) -> (points, y_cls, y_reg) being what the epoch's step k trains on.
    batch=B > 1 (fit(batch_size=B)): more plans per buffer set, recorded behind the batch-1 plans, which are recorded
    exactly as without it: a micro-step that only accumulates, in its two forms ('first': acc = grad, and for B > 2
    'middle': acc += grad), and the micro-step that ends a batch ('last': the mean, the exchange, the update, the
    repack) -- LisecNet.train_micro_step.  fit_step(..., position=) picks the plan; the divisor 1/b is device data that
    LisecNet.set_batch_divisor rewrites between replays, so one set of plans serves a short last batch too (a batch of
    one is the batch-1 plan)."""

    def __init__(self, net, voxelizer, capacity, dtype=torch.float32, loss="mse", warmup=2, allreduce=None, opt=None,
                 batch=1, wform=None):
        nbuf = self.NBUF                         # the number of buffer sets, and of batch-1 plans
        super().__init__(net, voxelizer, capacity, nbuf, dtype, loss, wform)
        # data parallel: the two-bucket gradient exchange (parallel._BucketedAverage) is part of the recorded schedule --
        # lisec_allreduce_grads and its event edges record themselves, a torch.distributed exchange rides as host calls.
        # Every rank records and replays the same sequence (the warm-up and recording steps exchange gradients for real).
        self.allreduce = allreduce
        dev = net.device
        self.opt = OptimizerSpec() if opt is None else opt      # the optimizer of the recorded step
        torch.cuda.synchronize(dev)
        net._prepare_training()
        for name in self.opt.slots:
            net.slot(name)                       # made before the plan records their addresses
        self.micro = {}                          # (position, buffer set) -> plan of a micro-step of a batch
        batch = int(batch)
        if batch > 1:
            net._batch_buffers()                 # likewise: the accumulator and the divisor
        if self.opt.average is not None:
            net.average                          # likewise: the weight average
        keep = self._snapshot()
        self.samples = [self.vox(pts) for pts in self.points]
        # eager warm-up (lazy workspaces, descriptor tables, events; it leaves the next step's repack pending, which is
        # the state every recorded step starts from), then one more step per buffer set that is recorded while it runs
        for k in range(nbuf * max(1, warmup)):
            self._enqueue(k % nbuf)
        torch.cuda.synchronize(dev)
        for j in range(nbuf):
            self._record(lambda: self._enqueue(j))
        torch.cuda.synchronize(dev)
        if batch > 1:
            self._record_micro_plans(("first", "middle", "last") if batch > 2 else ("first", "last"))
        # those steps trained on the padding: put every variable back and repack the kernels from them
        self._restore(keep)
        net.params_version += 1
        net.state_version += 1
        net.params.touch()
        net._arm_repack()
        self.cur = 0
        self._seal()

    def _snapshot(self):
        """The variables, BN state, every optimizer slot, the iteration count and Nadam's momentum_cache, before the
        warm-up / recording steps."""
        net, p = self.net, self.net.params
        return (p.theta.clone(), p.state.clone(), {k: t.clone() for k, t in net.slots().items()}, net._iter_dev.clone(),
                net._iterations, net.momentum_cache.clone(),
                None if net._acc is None else (net._acc.clone(), net._acc_scale.clone(), net._acc_div),
                net._average.clone() if net._average_live else None)

    def _record_micro_plans(self, positions):
        """The plans of the micro-steps of a batch, per buffer set: one eager batch of len(positions) sweeps (first,
        middle if any batch has one, last) as a warm-up, one more that is recorded while it runs.  Every plan is recorded with the repack of the last
        update pending, as the batch-1 plans are: its forward waits for the two pack events, which an update several
        micro-steps back has signalled long since (LisecNet._replayed_micro keeps the flags set between replays)."""
        net = self.net
        net.set_batch_divisor(len(positions))
        for record in (False, True):
            for j in range(self.NBUF):
                for position in positions:
                    net._pack_pending = net._late_pending = True
                    if record:
                        self._record(lambda: self._enqueue(j, position))
                        self.micro[position, j] = self.plans[-1]
                    else:
                        self._enqueue(j, position)
            torch.cuda.synchronize(net.device)

    def _restore(self, keep):
        net, p = self.net, self.net.params
        p.theta.copy_(keep[0])
        p.state.copy_(keep[1])
        for k, t in keep[2].items():
            net.slot(k).copy_(t)
        net._iter_dev.copy_(keep[3])
        net._iterations = keep[4]
        net.momentum_cache.copy_(keep[5])
        if keep[6] is not None:
            net._acc.copy_(keep[6][0])
            net._acc_scale.copy_(keep[6][1])
            net._acc_div = keep[6][2]
        if keep[7] is not None:
            net._average.copy_(keep[7])

    def _enqueue(self, j, position="single"):
        """One eager step on buffer set j (warm-up, or recorded while it runs)."""
        self.net.train_micro_step(self.samples[j], self.ycls[j], self.yreg[j], position, loss=self.loss,
                                  allreduce=self.allreduce, opt=self.opt, side_filler=self._voxelise(j),
                                  weights=None if self.weights is None else self.weights[j])

    def _run(self, position="single"):
        """Replays the plan of the current buffer set (position: of the micro-step of a batch, see LisecNet.
        train_micro_step); returns net.loss_out (device, [total, class, regression])."""
        self._check_stream()
        self._check_fresh()
        net = self.net
        if position == "single":
            plan = self.plans[self.cur]
        else:
            plan = self.micro.get((position, self.cur))
            if plan is None:
                raise RuntimeError(f"this {type(self).__name__} holds no plan for the {position!r} sweep of a batch: it was "
                                   f"recorded for a smaller batch size (batch=)")
        cur = (net.params_version, net.params.version)
        if net._packed_version != cur or net._packed_t_version != cur or not net._pack_pending:
            # the variables were changed since the last step (params.load_dict / touch, an eager step): the recorded
            # forward contains no repack, so it is made now on the replay stream
            net._arm_repack()
        _lib.check(self.lib.lisec_step_plan_run(plan))
        if position in ("single", "last"):
            net._replayed()
        else:
            net._replayed_micro()
        for s_ in self.samples:
            s_._host_info = None
        self.cur = (self.cur + 1) % self.NBUF
        return net.loss_out


class RecordedStep(_TrainingPlans):
    """One whole fit() step -- voxelise, forward, backward (both streams, fork / join events included), the optimizer
    update (opt: an OptimizerSpec, SGD-Nesterov by default), the weight repack for the next step -- recorded ONCE as a
    step plan of the C ABI (lisec_step_plan_*, csrc/plan.hip) and re-issued by one C call per step: the ~250 launches
    cost the host one ctypes call instead of ~1.5 ms of Python
    (schedule, plan selection, argument marshalling).  It IS the eager schedule -- same kernels, same streams, same
    events, bit-identical variables -- not a HIP graph (a captured graph of this two-stream step replays 2x slower than
    the eager launches on ROCm 7.2).  The schedule is static; what varies from sample to sample lives in device memory:

      points   a fixed-capacity (capacity, 3) buffer; a sweep with fewer points is padded with points far outside
               the grid, which the voxeliser's range test (model_training.py:118-120) drops -- kept points, their
               order and therefore every voxel and feature row are exactly those of the unpadded sweep
      targets  (Ho,Wo,2) / (Ho,Wo,14) static buffers
      lr_t     derived by the optimizer kernels from the device iteration counter (lisec_sgd_nesterov_step_dev,
               lisec_sgd_step_dev, lisec_adam_step_dev) -- and with a learning-rate schedule or a rate that changes
               between epochs, from the descriptor LisecNet._lr.dev (lisec_*_step_sched), which LisecNet._sync_lr
               rewrites between replays

    Record and replay on ONE torch stream (the current stream at construction).  Data parallel (allreduce=): the gradient
    exchange is part of the plan."""

    NBUF = 1

    def _voxelise(self, j):
        self.vox(self.points[0], out=self.samples[0])       # at the head of the step
        return None

    def load(self, points, ycls, yreg, weights=None):
        """Stage one sweep: points (n <= capacity, >= 3 columns; device or host tensor / numpy), targets (Ho,Wo,2|14),
        and the sample weights of a weighted plan."""
        self._load(0, points, ycls, yreg, weights)

    def replay(self, position="single"):
        """Runs the recorded step on what load() staged; returns net.loss_out (device, [total, class, regression])."""
        return self._run(position)

    def __call__(self, points, ycls, yreg, weights=None, position="single"):
        self.load(points, ycls, yreg, weights)
        return self.replay(position)

    def fit_step(self, sweep, st, steps, position="single"):
        return self(*sweep(st), position=position)


class PipelinedStep(_TrainingPlans):
    """RecordedStep with the input pipeline folded in: step k voxelises the sweep of step k + 1 on the second stream, in the
    ~200 us that stream idles at the start of the backward pass, instead of step k + 1 starting with 90 us of seven small
    dependent launches in front of its first contraction.  Two sets of (points, targets, voxel sample) buffers alternate,
    so there are two recorded plans; the variables after every step are bit-identical to the eager schedule's (a sweep's
    voxels do not depend on when they are computed).

        step = PipelinedStep(net, voxelizer, capacity)
        step.prime(points0, ycls0, yreg0)                    # stage + voxelise the first sweep
        for k in range(n):
            loss = step.step(points[k + 1], ycls[k + 1], yreg[k + 1])     # trains on sweep k, prepares sweep k + 1
                                                                          # (no arguments: the staged buffers are reused)
    """

    NBUF = 2

    def _voxelise(self, j):
        # the sweep of this step was voxelised by the step before; this one voxelises the next under its backward pass
        return lambda: self.vox(self.points[1 - j], out=self.samples[1 - j])

    def prime(self, points, ycls, yreg, weights=None):
        """Stages the FIRST sweep and voxelises it (outside the plans); the next step() trains on it."""
        self._load(self.cur, points, ycls, yreg, weights)
        self.vox(self.points[self.cur], out=self.samples[self.cur])

    def stage_next(self, points, ycls, yreg, weights=None):
        """Stages the sweep the next step() voxelises (and the step() after it trains on)."""
        self._load(1 - self.cur, points, ycls, yreg, weights)

    def step(self, next_points=None, next_ycls=None, next_yreg=None, next_weights=None, position="single"):
        """Trains on the current sweep and voxelises the staged next one; returns net.loss_out (device)."""
        if next_points is not None:
            self._load(1 - self.cur, next_points, next_ycls, next_yreg, next_weights)
        return self._run(position)

    def fit_step(self, sweep, st, steps, position="single"):
        """Sweep st of an epoch of `steps` sweeps: the next sweep is voxelised under this one's backward whatever the
        two are to their batches, so the pipeline runs across micro-step and batch boundaries."""
        if st == 0:
            self.prime(*sweep(0))                 # (every epoch draws its own order and primes its first sweep)
        return self.step(*sweep(st + 1), position=position) if st + 1 < steps else self.step(position=position)


class EvalStep(_StepPlans):
    """One evaluation sweep -- voxelise a fixed-capacity padded sweep (as RecordedStep), forward(training=False), add the
    sweep's loss to a device accumulator (lisec_rpn_loss_eval; lisec_head_loss_eval for a LossSpec, lisec_detection_loss_eval for a DetectionLossSpec) -- recorded ONCE as a
    step plan and re-issued by one C call per sweep (Model.evaluate and the validation of Model.fit with
    LISEC_TUNING=eval_plan=1; by default they run the eager forward, measured faster: DESIGN.md).  The accumulator acc = [total, class, regression, sweeps] -- with metrics
    in the layout of loss_acc_len -- (float64, device) is read by the host once per evaluation.  Invariants:

      BN fold   inference scale/shift come from ops.bn_fold (LisecNet._bn_after), cached per (params_version,
                state_version, params.version); a training step overwrites bnstate with batch statistics and moves the
                moving statistics.  The plan holds NO fold: prepare() re-folds eagerly, on the replay stream, whatever is
                stale before the first replay of a new version, and the plan is recorded with every fold current.
      repack    the plan holds no repack and no wait for one.  prepare() makes the packed kernels current: a repack left
                pending on the second stream by a training step (_pack_pending / _late_pending) is waited for through
                _pack_late (the flags stay set: the training plan's own waits for the same events are then already
                satisfied); otherwise a stale pack is redone eagerly by _pack_all(), which leaves _packed_t_version behind,
                so the training plan's _run() guard re-arms its repack.
      training  nothing of training is written: theta, state, the optimizer slots, the iteration counts and
                params_version are untouched (only bnstate, which every training forward rewrites before it reads it,
                and the activations); the sweep is staged into buffers of its own (points, targets, voxel sample).
      workspaces  the shared grow-on-demand buffers (VFE saved state, field and split-K workspaces, the voxeliser's when
                it shares the training step's) only grow for a sweep larger than any before: an evaluation no larger than
                the training sweeps leaves _lib.alloc_generation() -- and so the training plan -- as it is.

    Record and replay on ONE torch stream (the current stream at construction)."""

    def __init__(self, net, voxelizer, capacity, dtype=torch.float32, loss="mse", wform=None):
        self.nacc = loss_acc_len(loss, wform is not None)    # refuses an unknown loss before anything is allocated
        super().__init__(net, voxelizer, capacity, 1, dtype, loss, wform)
        dev = net.device
        self.acc = torch.zeros(self.nacc, dtype=torch.float64, device=dev)
        self._ready = None                        # the (params_version, state_version, params.version) prepare() served
        self.sample = self.vox(self.points[0])
        self.prepare()
        scratch = torch.zeros(self.nacc, dtype=torch.float64, device=dev)
        self._enqueue(scratch)                    # eager warm-up: lazy workspaces, descriptor tables, events
        torch.cuda.synchronize(dev)
        self._record(lambda: self._enqueue(self.acc))
        self.acc.zero_()                          # the recording ran on the padding
        self._seal()

    def _enqueue(self, acc):
        net = self.net
        pending = net._pack_pending, net._late_pending
        net._pack_pending = net._late_pending = False      # prepare() made every packed kernel current: no waits
        try:
            self.vox(self.points[0], out=self.sample)
            net.forward(self.sample, training=False)
        finally:
            net._pack_pending, net._late_pending = pending
        net.loss_eval(self.loss, self.ycls[0], self.yreg[0], acc, None if self.weights is None else self.weights[0])

    def prepare(self):
        """Packed kernels and BatchNormalization folds current for the weights and statistics of now (see the class)."""
        net = self.net
        key = (net.params_version, net.state_version, net.params.version)
        if self._ready == key:
            return                                # nothing moved since the last sweep: the plan's inputs are current
        main = torch.cuda.current_stream()
        if net._pack_pending or net._late_pending:
            net._wait(net._pack_late, main)
            if net._packed_version != (net.params_version, net.params.version):
                net._pack_pending = net._late_pending = False       # variables changed since that repack
        prev_pin = _lib.pin_stream(main.cuda_stream)
        try:
            net._pack_all()
            net._fold_inference()
        finally:
            _lib.pin_stream(prev_pin)
        self._ready = key

    def reset(self):
        """Zeroes the accumulator (stream-ordered)."""
        self.acc.zero_()

    def __call__(self, points, ycls, yreg, weights=None):
        """Stages one sweep (points: n <= capacity rows, >= 3 columns; targets (Ho,Wo,2|14); the sample weights of a
        weighted plan) and replays the plan: its loss is added to self.acc."""
        self._check_fresh()
        self._load(0, points, ycls, yreg, weights)
        self.prepare()
        _lib.check(self.lib.lisec_step_plan_run(self.plans[0]))
        self.sample._host_info = None
        return self.acc
