"""Keras HDF5 checkpoint layout for the Lisec network.

The reference persists its model with Keras: model.save(save_path) (model_training.py:302) and
load_model(path, custom_objects={'RepeatLayer':..., 'MaxPoolingVFELayer':...}) (model_training.py:337-338,
Predict.py:51-52).  A Keras `.h5` holds

    /                   attrs keras_version, backend, model_config (JSON), training_config (JSON)
    /model_weights      attrs layer_names, backend, keras_version
        /<layer>        attr weight_names = [b'<layer>/kernel:0', ...]; datasets at <layer>/<weight>:0
    /optimizer_weights  attr weight_names = [b'SGD/iter:0', b'SGD/<layer>/<weight>/momentum:0', ...] + datasets
                        (Adam: b'Adam/iter:0', every .../m:0, every .../v:0, every .../vhat:0 with amsgrad;
                        RMSprop, Adagrad, Adadelta, Adamax, Nadam: b'<Class>/iter:0', Nadam's
                        b'Nadam/momentum_cache:0', then their slots kind by kind, in the order of optimizer_table)

This module rebuilds the layer list that createModel (model_training.py:222-257) produces -- with the names Keras
assigns automatically (dense, dense_1, batch_normalization_7, conv2d_transpose_2 ...) and the order of
Model.layers (decreasing depth, ties in traversal order) -- maps every Keras variable onto the flat ParamStore
names of lisec_amd.params, and reads / writes the file through lisec_amd.hdf5_lite.  Weight regularizers travel where
Keras keeps them, in the layer configs of model_config (kernel_regularizer / bias_regularizer of Dense, Conv3D, Conv2D and
Conv2DTranspose, beta_regularizer / gamma_regularizer of BatchNormalization), per variable.

PARITY UNPINNED against Keras itself (TensorFlow is not installed here): the HDF5 container is cross-checked
against h5py/libhdf5 in tests/test_hdf5_lite.py; the Keras naming rules are restated from Keras' public behaviour.
"""
import json
import re

import numpy as np

from . import hdf5_lite, optimizer_table
from . import regularizers as regularizers_mod
from .params import DECONVS, MID, RPN_BLOCKS

KERAS_VERSION = "2.4.0"
BN_WEIGHTS = ("gamma", "beta", "moving_mean", "moving_variance")


def _snake(cls):
    s = re.sub("(.)([A-Z][a-z0-9]+)", r"\1_\2", cls)
    return re.sub("([a-z])([A-Z])", r"\1_\2", s).lower()


class _Graph:
    """Records layers as createModel creates them; names follow Keras' per-class counters."""

    def __init__(self):
        self.layers, self.counts = [], {}

    def add(self, cls, inbound, config=None, weights=(), name=None):
        if name is None:
            base = _snake(cls)
            n = self.counts.get(base, 0)
            self.counts[base] = n + 1
            name = base if n == 0 else f"{base}_{n}"
        cfg = {"name": name, "trainable": True, "dtype": "float32"}
        cfg.update(config or {})
        self.layers.append(dict(name=name, class_name=cls, config=cfg,
                                inbound=[inbound] if isinstance(inbound, str) else list(inbound),
                                weights=list(weights)))
        return name


def _glorot():
    return {"class_name": "GlorotUniform", "config": {"seed": None}}


def _zeros():
    return {"class_name": "Zeros", "config": {}}


def keras_layers(nx, ny, nz, maxPoints):
    """[dict(name, class_name, config, inbound, weights=[(keras weight, ParamStore name)])] in Model.layers order,
    plus the output layer names."""
    g = _Graph()
    T = maxPoints
    shape = (nz, nx, ny, T, 6)
    x = g.add("InputLayer", [], {"batch_input_shape": [None] + list(shape), "sparse": False, "ragged": False},
              name="InputVoxel")
    del g.layers[-1]["config"]["trainable"]

    def dense(x, shape, units, act, pname):                              # addDenseLayer :177-185
        flat = (int(np.prod(shape[:-2])),) + tuple(shape[-2:])
        x = g.add("Reshape", x, {"target_shape": list(flat)})
        x = g.add("Dense", x, {"units": units, "activation": act or "linear", "use_bias": False,
                               "kernel_initializer": _glorot(), "bias_initializer": _zeros(),
                               "batch_input_shape": [None] + list(flat)},
                  weights=[("kernel", pname + ".kernel")])
        shape = tuple(shape[:-1]) + (units,)
        x = g.add("Reshape", x, {"target_shape": list(shape)})
        return x, shape

    def bn(x, rank, pname):
        return g.add("BatchNormalization", x, {"axis": [rank], "momentum": 0.99, "epsilon": 0.001, "center": True,
                                               "scale": True},
                     weights=[(w, f"{pname}.{w}") for w in BN_WEIGHTS])

    def fcn(x, shape, units, pname):                                     # addFCN :168-173
        x, shape = dense(x, shape, units, None, pname + ".dense")
        x = bn(x, len(shape), pname + ".bn")
        x = g.add("Activation", x, {"activation": "relu"})
        return x, shape

    def vfe(x, shape, units, pname):                                     # addVFELayer :155-165
        x, shape = fcn(x, shape, units // 2, pname)
        pool = g.add("MaxPoolingVFELayer", x, {"combine": False})
        rep = g.add("RepeatLayer", pool)
        x = g.add("Concatenate", [rep, x], {"axis": -1})
        return x, tuple(shape[:-1]) + (units,)

    x, shape = vfe(x, shape, 32, "vfe1")
    x, shape = vfe(x, shape, 64, "vfe2")
    x, shape = fcn(x, shape, 64, "fcn")
    x = g.add("MaxPoolingVFELayer", x, {"combine": True})
    shape = tuple(shape[:3]) + (64,)
    for i, (stride, pad) in enumerate(MID):                              # addConv3DLayer :190-195
        x = g.add("ZeroPadding3D", x, {"padding": [[p, p] for p in pad], "data_format": "channels_last"})
        x = g.add("Conv3D", x, {"filters": 64, "kernel_size": [3, 3, 3], "strides": list(stride), "padding": "valid",
                                "data_format": "channels_last", "dilation_rate": [1, 1, 1], "groups": 1,
                                "activation": "linear", "use_bias": True, "kernel_initializer": _glorot(),
                                "bias_initializer": _zeros()},
                  weights=[("kernel", f"mid{i+1}.conv.kernel"), ("bias", f"mid{i+1}.conv.bias")])
        shape = tuple((s + 2 * p - 3) // st + 1 for s, p, st in zip(shape[:3], pad, stride)) + (64,)
        x = bn(x, 4, f"mid{i+1}.bn")
        x, shape = dense(x, shape, 64, "relu", f"mid{i+1}.dense")
    x = g.add("Permute", x, {"dims": [2, 3, 4, 1]})
    shape = (shape[1], shape[2], shape[3] * shape[0])
    x = g.add("Reshape", x, {"target_shape": list(shape)})

    def conv2d(x, cout, stride, pname_conv, pname_bn):                   # addConv2DLayer :200-206
        x = g.add("ZeroPadding2D", x, {"padding": [[1, 1], [1, 1]], "data_format": "channels_last"})
        x = g.add("Conv2D", x, {"filters": cout, "kernel_size": [3, 3], "strides": [stride, stride],
                                "padding": "valid", "data_format": "channels_last", "dilation_rate": [1, 1],
                                "groups": 1, "activation": "linear", "use_bias": True,
                                "kernel_initializer": _glorot(), "bias_initializer": _zeros()},
                  weights=[("kernel", pname_conv + ".kernel"), ("bias", pname_conv + ".bias")])
        x = bn(x, 3, pname_bn)
        return g.add("Activation", x, {"activation": "relu"})

    ups = []
    for b, (cout, q) in enumerate(RPN_BLOCKS):                           # addRPNConvLayer :210-214, :245-252
        for j in range(q + 1):
            x = conv2d(x, cout, 2 if j == 0 else 1, f"rpn{b+1}.conv{j}", f"rpn{b+1}.bn{j}")
        k, s = DECONVS[b]
        ups.append(g.add("Conv2DTranspose", x, {
            "filters": 256, "kernel_size": [k, k], "strides": [s, s], "padding": "same",
            "data_format": "channels_last", "dilation_rate": [1, 1], "groups": 1, "activation": "linear",
            "use_bias": True, "output_padding": None, "kernel_initializer": _glorot(), "bias_initializer": _zeros()},
            weights=[("kernel", f"up{b+1}.kernel"), ("bias", f"up{b+1}.bias")]))
    cat = g.add("Concatenate", ups, {"axis": -1})
    outs = []
    for name, filters, p in (("ClassificationLayer", 2, "cls"), ("RegressionLayer", 14, "reg")):
        outs.append(g.add("Conv2D", cat, {"filters": filters, "kernel_size": [1, 1], "strides": [1, 1],
                                          "padding": "same", "data_format": "channels_last", "dilation_rate": [1, 1],
                                          "groups": 1, "activation": "linear", "use_bias": True,
                                          "kernel_initializer": _glorot(), "bias_initializer": _zeros()},
                          weights=[("kernel", p + ".kernel"), ("bias", p + ".bias")], name=name))
    return _model_layers_order(g.layers, outs), outs


def _model_layers_order(layers, outputs):
    """Order of keras Model.layers: decreasing depth (longest path to an output); equal depths in the order a
    depth-first walk from the outputs first completes them (functional.py _map_graph_network)."""
    by_name = {L["name"]: L for L in layers}
    depth, index = {}, {}

    def visit(name):                                   # post-order: inputs before the layer itself
        stack = [(name, iter(by_name[name]["inbound"]))]
        seen = {name}
        while stack:
            cur, it = stack[-1]
            nxt = next(it, None)
            if nxt is None:
                stack.pop()
                if cur not in index:
                    index[cur] = len(index)
            elif nxt not in index and nxt not in seen:
                seen.add(nxt)
                stack.append((nxt, iter(by_name[nxt]["inbound"])))
    for o in outputs:
        visit(o)
    # longest path to an output: relax consumers before producers (reverse creation order is a valid order)
    for L in layers:
        depth[L["name"]] = 0
    for L in reversed(layers):
        for src in L["inbound"]:
            depth[src] = max(depth[src], depth[L["name"]] + 1)
    return sorted(layers, key=lambda L: (-depth[L["name"]], index[L["name"]]))


REGULARIZED_WEIGHTS = ("kernel", "bias", "gamma", "beta")     # Keras' <weight>_regularizer keys of a layer config


def model_config(nx, ny, nz, maxPoints, regularizers=None):
    """regularizers: {ParamStore name: (l1, l2)} or None.  A layer's config gains "<weight>_regularizer" ({"class_name":
    "L2", "config": {"l2": ...}}, the shortest of L1 / L2 / L1L2 that says it) only for a variable with a pair other
    than (0, 0): the config of an unregularised model keeps the bytes it always had.  (Keras itself writes the key
    with null for a layer without one; load_model reads both.)  KeyError: a name the network does not have; ValueError:
    a variable that is not trainable (a moving statistic), as ops.reg_chunks refuses it."""
    layers, outs = keras_layers(nx, ny, nz, maxPoints)
    known = {pname: w for L in layers for w, pname in L["weights"]}
    for name in regularizers or {}:
        if name not in known:
            raise KeyError(f"regularizers: the network has no variable {name!r}")
        if known[name] not in REGULARIZED_WEIGHTS:
            raise ValueError(f"regularizers: {name} is not a trainable variable: it cannot be regularised")
    cfg_layers = []
    for L in layers:
        inbound = [[[src, 0, 0, {}] for src in L["inbound"]]] if L["inbound"] else []
        for w, pname in L["weights"]:
            reg = regularizers_mod.from_pair(*regularizers[pname]) if pname in (regularizers or {}) else None
            if w in REGULARIZED_WEIGHTS and reg is not None:
                L["config"][f"{w}_regularizer"] = regularizers_mod.serialize(reg)
        cfg_layers.append({"class_name": L["class_name"], "config": L["config"], "name": L["name"],
                           "inbound_nodes": inbound})
    return {"class_name": "Functional",
            "config": {"name": "model", "layers": cfg_layers, "input_layers": [["InputVoxel", 0, 0]],
                       "output_layers": [[o, 0, 0] for o in outs]},
            "keras_version": KERAS_VERSION, "backend": "tensorflow"}


def _rate(lr):
    """A learning rate of training_config: a number, or a serialized schedule ({"class_name", "config"}) as is."""
    return lr if isinstance(lr, dict) else float(lr)


def _serialize_nested(x):
    """Keras' _serialize_nested_config: a loss or metric object becomes {"class_name", "config"}, names stay as given,
    lists and dicts keep their structure."""
    if hasattr(x, "get_config"):
        return {"class_name": type(x).__name__, "config": x.get_config()}
    if isinstance(x, dict):
        return {k: _serialize_nested(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_serialize_nested(v) for v in x]
    return x


# the optimizer wrappers that keep a weight average (model_training.optimizers.MovingAverage / SWA): their
# optimizer_config nests the wrapped optimizer's under "optimizer", their one slot kind follows the wrapped optimizer's
WRAPPER_CLASSES = ("MovingAverage", "SWA")
AVERAGE_KIND = "average"
# the gradient-clipping keys of an optimizer dict and of its config (model_training.optimizers.clip_gradients): there
# only when set, so a file without clipping has the bytes it always had; under a wrapper they sit in the nested config
CLIP_KEYS = ("clipnorm", "clipvalue", "global_clipnorm")


def written_class(optimizer):
    """The class name an optimizer dict is written under: its record's (optimizer_table.record_of), or <Base>W for the
    decoupled-weight-decay class of <Base> (model_training.optimizers.extend_with_decoupled_weight_decay), whose record,
    kernels and slot kinds are <Base>'s.  The spelling of that config -- Keras' keys of <Base>, then "weight_decay" and
    "decay_var_list" -- is this project's restatement of tfa's: tfa is not installed, parity unpinned."""
    rec, cls = optimizer_table.record_of(optimizer), optimizer.get("class_name")
    return cls if cls != rec.class_name and optimizer_table.base_class(cls) == rec.class_name else rec.class_name


def _training_config(optimizer, loss=None, loss_weights=None, metrics=None, wrapper=None, weighted_metrics=None):
    """The training_config attribute.  loss / loss_weights / metrics: compile()'s arguments as given (None: the reference's
    loss=['mse','mse'], no weights, no metrics -- the bytes every earlier version wrote).  optimizer_config holds Keras'
    keys in Keras' order, a key the dict lacks at Keras' default (optimizer_table)."""
    o = optimizer or {}
    rec = optimizer_table.record_of(o)
    cls = written_class(o)
    oc = {"class_name": cls, "config": {
        "name": cls, "learning_rate": _rate(o.get("lr", rec.lr)), "decay": float(o.get("decay", rec.decay)),
        **rec.values(o),
        # a layer-wise optimizer's exclusion lists (LAMB; names and kinds of this project, not tfa's regular expressions)
        **{k: (None if o.get(k) is None else list(o[k])) for k in rec.lists}}}
    if cls != rec.class_name:                     # <Base>W: the coefficient (a number or a serialized schedule) and,
        oc["config"]["weight_decay"] = _rate(o.get("weight_decay", 0.0))          # only when given, the decayed variables
        if o.get("decay_var_list") is not None:
            oc["config"]["decay_var_list"] = list(o["decay_var_list"])
    for k in CLIP_KEYS:                           # as in Keras, a clipping key is written only when it is set
        if o.get(k) is not None:
            oc["config"][k] = float(o[k])
    if wrapper is not None:
        c = dict(wrapper["config"])
        oc = {"class_name": wrapper["class_name"], "config": {"name": c.pop("name", wrapper["class_name"]),
                                                              "optimizer": oc, **c}}
    return {"loss": ["mse", "mse"] if loss is None else _serialize_nested(loss), "metrics": _serialize_nested(metrics),
            "weighted_metrics": _serialize_nested(weighted_metrics), "loss_weights": _serialize_nested(loss_weights), "optimizer_config": oc}


# the slot arguments of save_model and slot keys of load_model: LisecNet's slot names, so Keras' "momentum" is "velocity"
# in an SGD file and "momentum", a buffer of its own, in an RMSprop file
SLOT_KEYS = optimizer_table.SLOT_NAMES


# ---------------------------------------------------------------------------------------------------
def save_model(path, params, nx, ny, nz, maxPoints, optimizer=None, iterations=0, loss=None, loss_weights=None,
               metrics=None, momentum_cache=1.0, regularizers=None, wrapper=None, average=None, weighted_metrics=None,
               **given):
    """params: dict ParamStore name -> array.  optimizer: dict(lr, decay, momentum, nesterov) for SGD,
    dict(class_name="Adam", lr, decay, beta_1, beta_2, epsilon, amsgrad) for Adam (lr: a number, or a learning-rate
    schedule serialized as Keras does, {"class_name", "config"}), or None (a model that was never
    compiled: no training_config / optimizer_weights, like Keras).  The slots, each a dict of trainable ParamStore
    name -> array: velocity (SGD momentum accumulators, momentum > 0), m and v (Adam moments), vhat (AMSGrad); rms,
    momentum (momentum > 0) and mg (centered) of RMSprop; accumulator of Adagrad; accum_grad and accum_var of Adadelta;
    m and v of Adamax and Nadam.  Other optimizers: dict(class_name=<Keras class>, lr, decay, <their config keys>)
    (Nadam's decay: schedule_decay); momentum_cache: Nadam's scalar.  optimizer_weights is written when every slot the optimizer keeps is given (SGD without momentum keeps none).
    loss, loss_weights, metrics, weighted_metrics: Model.compile's arguments as given, written into training_config as Keras 2.4 does (names
    as they are, loss / metric objects as {"class_name", "config"}); None: loss ['mse','mse'], no weights, no metrics.
    regularizers: {ParamStore name: (l1, l2)} or None, written into the layer configs (model_config).
    wrapper: {"class_name": "MovingAverage" | "SWA", "config": its own keys, without "optimizer"} or None: the
    optimizer_config becomes the wrapper's, with the optimizer's nested under "optimizer"; average: the weight average,
    a dict like a slot, written as <wrapper class>/<variable>/average:0 behind the optimizer's own slot kinds.  Without a
    wrapper the file has the bytes it always had.
    **given: the slots, by the names of SLOT_KEYS (any other keyword: TypeError)."""
    if wrapper is not None and wrapper.get("class_name") not in WRAPPER_CLASSES:
        raise ValueError(f"save_model: optimizer wrapper class {wrapper.get('class_name')!r} is not implemented")
    if wrapper is not None and optimizer is None:
        raise ValueError("save_model: a wrapper needs the optimizer it wraps")
    for k in given:
        if k not in SLOT_KEYS:
            raise TypeError(f"save_model() got an unexpected keyword argument {k!r}")
    layers, _ = keras_layers(nx, ny, nz, maxPoints)
    with hdf5_lite.File(path, "w") as f:
        f.attrs["keras_version"] = KERAS_VERSION.encode()
        f.attrs["backend"] = b"tensorflow"
        f.attrs["model_config"] = json.dumps(model_config(nx, ny, nz, maxPoints, regularizers)).encode("utf8")
        if optimizer is not None:
            f.attrs["training_config"] = json.dumps(_training_config(optimizer, loss, loss_weights, metrics,
                                                                     wrapper, weighted_metrics)).encode("utf8")
        g = f.create_group("model_weights")
        g.attrs["layer_names"] = [L["name"].encode("utf8") for L in layers]
        g.attrs["backend"] = b"tensorflow"
        g.attrs["keras_version"] = KERAS_VERSION.encode()
        slots = []
        for L in layers:
            lg = g.create_group(L["name"])
            names = [f"{L['name']}/{w}:0" for w, _ in L["weights"]]
            lg.attrs["weight_names"] = [n.encode("utf8") for n in names]
            for n, (w, pname) in zip(names, L["weights"]):
                lg.create_dataset(n, data=np.asarray(params[pname], dtype=np.float32))
                if w in ("kernel", "bias", "gamma", "beta"):
                    slots.append((f"{L['name']}/{w}", pname))
        if optimizer is None:
            return
        rec = optimizer_table.record_of(optimizer)
        cls, kept = written_class(optimizer), rec.active_slots(rec.values(optimizer))
        if any(given.get(s.name) is None for s in kept):
            return
        # Keras' order: iter, the optimizer's own scalar, then one slot kind for every variable before the next kind
        entries = [(f"{cls}/{var}/{s.kind}:0", given[s.name][pname]) for s in kept for var, pname in slots]
        if wrapper is not None and average is not None:
            entries += [(f"{wrapper['class_name']}/{var}/{AVERAGE_KIND}:0", average[pname]) for var, pname in slots]
        head = [f"{cls}/iter:0"] + ([f"{cls}/{rec.scalar}:0"] if rec.scalar else [])
        og = f.create_group("optimizer_weights")
        og.attrs["weight_names"] = [n.encode() for n in head] + [n.encode("utf8") for n, _ in entries]
        og.create_dataset(f"{cls}/iter:0", data=np.array(int(iterations), dtype=np.int64))
        if rec.scalar:
            og.create_dataset(f"{cls}/{rec.scalar}:0", data=np.array(momentum_cache, dtype=np.float32))
        for n, a in entries:
            og.create_dataset(n, data=np.asarray(a, dtype=np.float32))


def _text(v):
    if isinstance(v, (bytes, np.bytes_)):
        return bytes(v).decode("utf8")
    return str(v)


def _attr_list(group, name):
    """load_attributes_from_hdf5_group: an attribute too large for one object header message is split into
    name0, name1, ... by Keras."""
    if name in group.attrs:
        return [_text(x) for x in np.asarray(group.attrs[name]).ravel()]
    out, i = [], 0
    while f"{name}{i}" in group.attrs:
        out.extend(_text(x) for x in np.asarray(group.attrs[f"{name}{i}"]).ravel())
        i += 1
    return out


_BASES = ("batch_normalization", "conv2d_transpose", "conv3d", "conv2d", "dense", "ClassificationLayer",
          "RegressionLayer")


def _base_of(name):
    return next((b for b in _BASES if name == b or re.fullmatch(re.escape(b) + r"_\d+", name)), None)


def _suffix_number(name, base):
    rest = name[len(base):]
    return int(rest[1:]) if rest else 0


def _layer_regularizers(layer_cfg, weights):
    """{ParamStore name: (l1, l2)} of one layer of a model_config (weights: the layer's [(keras weight, ParamStore
    name)]).  null or an absent key: none.  NotImplementedError, naming the layer: an activity_regularizer, or a
    regularizer class other than L1, L2 and L1L2."""
    c, out = layer_cfg.get("config", {}), {}
    lname = layer_cfg.get("name", c.get("name"))
    if c.get("activity_regularizer") is not None:
        raise NotImplementedError(f"layer {lname}: activity_regularizer is not implemented")
    for w, pname in weights:
        ser = c.get(f"{w}_regularizer")
        if ser is None:
            continue
        try:
            pair = regularizers_mod.deserialize(ser).pair()
        except (ValueError, TypeError, NotImplementedError) as e:
            raise NotImplementedError(f"layer {lname}: {w}_regularizer {ser!r} is not implemented ({e})") from None
        if pair != (0.0, 0.0):
            out[pname] = pair
    return out


def load_model(path, grid=None):
    """Reads a Keras `.h5` written by the reference (or by save_model).  Returns dict(params, nx, ny, nz, maxPoints,
    iterations, optimizer (dict or None, as save_model takes it), loss, loss_weights, metrics (training_config's, as
    serialized there; None without one), the slots of SLOT_KEYS (each a dict of trainable ParamStore name -> array, or
    None; mapped per optimizer class, so "momentum" is SGD's velocity in an SGD file) and momentum_cache (Nadam's, or
    None)) and regularizers ({ParamStore name: (l1, l2)}, read from each layer's config; {} without any).  Slots are
    matched by name, not by position.  A file of an averaging wrapper: wrapper ({"class_name", "config" without
    "optimizer"}; else None), `optimizer` the wrapped one's, and average (like a slot, or None).  An optimizer_config that
    nests an "optimizer" under a class that is not one of WRAPPER_CLASSES is refused by name (ValueError).

    Layers are matched by class and creation order (the numeric suffix of Keras' automatic names), not by the exact
    suffix: a model built as the second one of a Python session carries shifted suffixes."""
    with hdf5_lite.File(path, "r") as f:
        g = f["model_weights"] if "model_weights" in f else f
        if "layer_names" not in g.attrs and "layer_names0" not in g.attrs:
            raise hdf5_lite.H5Error(f"{path}: no Keras layer_names attribute")
        cfg = json.loads(_text(f.attrs["model_config"])) if "model_config" in f.attrs else None
        if cfg is not None:
            inp = next(L for L in cfg["config"]["layers"] if L["class_name"] == "InputLayer")
            _, nz, nx, ny, T, _ = inp["config"]["batch_input_shape"]
        elif grid is not None:
            nx, ny, nz, T = grid
        else:
            from . import Constants
            nx, ny, nz, T = Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints
        found = {}                                    # class base -> [(order, layer name, {weight kind: array})]
        for lname in _attr_list(g, "layer_names"):
            wnames = _attr_list(g[lname], "weight_names")
            if not wnames:
                continue
            base = _base_of(lname)
            if base is None:
                raise hdf5_lite.H5Error(f"{path}: layer {lname!r} with weights is not part of the Lisec network")
            vals = {w.split("/")[-1].split(":")[0]: np.asarray(g[lname][w][()], dtype=np.float32) for w in wnames}
            found.setdefault(base, []).append((_suffix_number(lname, base), lname, vals))
        for v in found.values():
            v.sort(key=lambda t: t[0])
        layers, _ = keras_layers(nx, ny, nz, T)
        want = {}
        for L in layers:
            if L["weights"]:
                base = _base_of(L["name"])
                want.setdefault(base, []).append((_suffix_number(L["name"], base), L))
        params, keras_to_param, regs = {}, {}, {}
        file_cfg = {L.get("name", L.get("config", {}).get("name")): L for L in cfg["config"]["layers"]} if cfg else {}
        for L in file_cfg.values():                   # any layer, with weights or without, may carry one
            _layer_regularizers(L, ())
        for base, lst in want.items():
            lst.sort(key=lambda t: t[0])
            have = found.get(base, [])
            if len(have) != len(lst):
                raise hdf5_lite.H5Error(f"{path}: {len(have)} {base} layers with weights, the network has {len(lst)}")
            for (_, L), (_, lname, vals) in zip(lst, have):
                if lname in file_cfg:
                    regs.update(_layer_regularizers(file_cfg[lname], L["weights"]))
                for w, pname in L["weights"]:
                    if w not in vals:
                        raise hdf5_lite.H5Error(f"{path}: layer {lname} lacks {w}")
                    params[pname] = vals[w]
                    keras_to_param[f"{lname}/{w}"] = pname
        out = dict(params=params, nx=int(nx), ny=int(ny), nz=int(nz), maxPoints=int(T), iterations=0, optimizer=None,
                   loss=None, loss_weights=None, metrics=None, weighted_metrics=None, momentum_cache=None,
                   regularizers=regs, wrapper=None, average=None,
                   **{k: None for k in SLOT_KEYS})
        if "training_config" in f.attrs:
            tc = json.loads(_text(f.attrs["training_config"]))
            out.update(loss=tc.get("loss"), loss_weights=tc.get("loss_weights"), metrics=tc.get("metrics"),
                       weighted_metrics=tc.get("weighted_metrics"))
            oc = tc.get("optimizer_config", {})
            c = oc.get("config", {})
            if isinstance(c.get("optimizer"), dict):              # a wrapper: the optimizer is the one it nests
                if oc.get("class_name") not in WRAPPER_CLASSES:
                    raise ValueError(f"{path}: optimizer wrapper class {oc.get('class_name')!r} is not implemented")
                out["wrapper"] = {"class_name": oc["class_name"], "config": {k: v for k, v in c.items() if k != "optimizer"}}
                oc = c["optimizer"]
                c = oc.get("config", {})
            base = optimizer_table.base_class(oc.get("class_name"))
            rec = optimizer_table.BY_CLASS.get(base)
            if rec is not None:               # another optimizer class: no optimizer, the model comes back uncompiled
                out["optimizer"] = rec.as_dict(c.get("learning_rate", c.get("lr", rec.lr)), c.get("decay", rec.decay),
                                               {h.name: c.get(h.name, h.default) for h in rec.hyper})
                for k in rec.lists:
                    out["optimizer"][k] = None if c.get(k) is None else list(c[k])
                if base != oc["class_name"]:  # <Base>W: the record is <Base>'s, the dict carries the class and the decay
                    out["optimizer"].update(class_name=oc["class_name"], weight_decay=c.get("weight_decay", 0.0))
                    if c.get("decay_var_list") is not None:
                        out["optimizer"]["decay_var_list"] = list(c["decay_var_list"])
                for k in CLIP_KEYS:
                    if c.get(k) is not None:
                        out["optimizer"][k] = float(c[k])
        if "optimizer_weights" in f:
            og = f["optimizer_weights"]
            slot_dataset = re.compile(r"([^/]+)/(.+)/(%s):0" % "|".join(optimizer_table.SLOT_KINDS + (AVERAGE_KIND,)))
            found_slots = {}
            for w in _attr_list(og, "weight_names"):
                a = og[w][()]
                if w.endswith("iter:0"):
                    out["iterations"] = int(a)
                    continue
                if w.endswith("/momentum_cache:0"):
                    out["momentum_cache"] = float(np.float32(a))
                    continue
                m = slot_dataset.fullmatch(w)
                if m and m.group(2) in keras_to_param:
                    kind = optimizer_table.slot_name(m.group(1), m.group(3))
                    found_slots.setdefault(kind, {})[keras_to_param[m.group(2)]] = np.asarray(a, dtype=np.float32)
            out.update(found_slots)
        return out
