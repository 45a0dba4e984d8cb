"""tf.keras.regularizers of 2.4 for the Lisec network: L1L2, L1, L2, the shorthands l1 / l2 / l1_l2, get, serialize and
deserialize.

A regularizer here is a pair of coefficients, nothing more: the penalty  l1*sum|w| + l2*sum w^2  and its gradient
2*l2*w + l1*sign(w)  are computed for every regularised variable by one pass over the flat parameter buffer
(csrc/regularize.hip) in front of the optimizer update, so a regularizer of one's own -- a callable, or a subclass with
its own __call__ -- cannot run and is refused (NotImplementedError), as losses.py refuses a loss of one's own.
Coefficients are kept as Keras keeps them: the Python float of the float32-rounded value (backend.cast_to_floatx), and
get_config() returns them under Keras' keys.  A negative, NaN or infinite coefficient raises ValueError.

createModel / Model take kernel_regularizer, bias_regularizer, gamma_regularizer and beta_regularizer; each applies to
every variable of that kind (params.param_specs()).  Keras' semantics: the penalty is added to `loss` alone (not to the
per-output losses, not scaled by loss_weights), in fit, evaluate and val_loss.

PARITY UNPINNED against Keras itself (TensorFlow is not installed here): the class names and config keys
({"class_name": "L2", "config": {"l2": ...}}) are restated from Keras' public behaviour.

A leaf module, like optimizer_table: it imports neither torch nor the HIP library."""
import math
import struct

KINDS = ("kernel", "bias", "gamma", "beta")          # the <kind>_regularizer keywords, params.TRAINABLE_KINDS


def _floatx(value, what):
    """Keras' cast_to_floatx of a coefficient, as a Python float.  ValueError: not a finite number >= 0."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {value!r} is not a number") from None
    if math.isnan(v) or math.isinf(v) or v < 0.0:
        raise ValueError(f"{what} must be a finite number >= 0, not {value!r}")
    try:
        v = struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:
        v = math.inf
    if math.isinf(v):
        raise ValueError(f"{what} = {value!r} is not finite in float32")
    return v


class Regularizer:
    """Base class, as in Keras.  Only the built-in classes of this module run in the kernels."""

    def __call__(self, x):
        raise NotImplementedError("the regularizers are evaluated by the kernels of Model.fit / Model.evaluate")

    def pair(self):
        """(l1, l2) of a built-in regularizer.  NotImplementedError for any other."""
        raise NotImplementedError(f"regularizer {type(self).__name__}: a regularizer of one's own cannot run in the "
                                  f"kernels; use a built-in Keras regularizer ({', '.join(_BUILTIN)})")

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def get_config(self):
        raise NotImplementedError(f"{type(self).__name__} has no get_config()")


class L1L2(Regularizer):
    """regularizers.L1L2(l1=0., l2=0.): l1*sum|w| + l2*sum w^2."""

    def __init__(self, l1=0., l2=0.):
        self.l1 = _floatx(l1, "l1")
        self.l2 = _floatx(l2, "l2")

    def pair(self):
        _check_builtin(self)
        return (self.l1, self.l2)

    def get_config(self):
        return {"l1": float(self.l1), "l2": float(self.l2)}


class L1(Regularizer):
    """regularizers.L1(l1=0.01): l1*sum|w|."""

    def __init__(self, l1=0.01, **kwargs):
        l1 = kwargs.pop("l", l1)                     # Keras 2.4 accepts the old spelling l=
        if kwargs:
            raise TypeError(f"Argument(s) not recognized: {kwargs}")
        self.l1 = _floatx(l1, "l1")

    def pair(self):
        _check_builtin(self)
        return (self.l1, 0.0)

    def get_config(self):
        return {"l1": float(self.l1)}


class L2(Regularizer):
    """regularizers.L2(l2=0.01): l2*sum w^2."""

    def __init__(self, l2=0.01, **kwargs):
        l2 = kwargs.pop("l", l2)
        if kwargs:
            raise TypeError(f"Argument(s) not recognized: {kwargs}")
        self.l2 = _floatx(l2, "l2")

    def pair(self):
        _check_builtin(self)
        return (0.0, self.l2)

    def get_config(self):
        return {"l2": float(self.l2)}


_BUILTIN = {"L1L2": L1L2, "L1": L1, "L2": L2}


def _check_builtin(reg):
    """A subclass that brings its own __call__ computes something the kernels do not."""
    if type(reg) not in _BUILTIN.values() and type(reg).__call__ is not Regularizer.__call__:
        Regularizer.pair(reg)


def l1_l2(l1=0.01, l2=0.01):
    return L1L2(l1=l1, l2=l2)


l1 = L1
l2 = L2

_NAMES = {"l1": L1, "l2": L2, "l1_l2": l1_l2, "L1": L1, "L2": L2, "L1L2": L1L2}


def serialize(regularizer):
    """{"class_name", "config"} as Keras writes it, or None for None."""
    if regularizer is None:
        return None
    regularizer = get(regularizer)
    # a subclass that get() accepts (no arithmetic of its own) is written under its built-in base, the name that
    # deserialize() knows (none of the three derives from another)
    name = next(n for n, c in _BUILTIN.items() if isinstance(regularizer, c))
    return {"class_name": name, "config": regularizer.get_config()}


def deserialize(config, custom_objects=None):
    """The regularizer of a {"class_name", "config"} dict or of a name.  ValueError: an unknown class or name;
    NotImplementedError: custom_objects (a regularizer of one's own cannot run in the kernels)."""
    if custom_objects:
        raise NotImplementedError("regularizers.deserialize(custom_objects=...): a regularizer of one's own cannot run in "
                                  "the kernels; use a built-in Keras regularizer")
    if isinstance(config, str):
        if config not in _NAMES:
            raise ValueError(f"Unknown regularizer: {config}")
        return _NAMES[config]()
    if not isinstance(config, dict) or "class_name" not in config:
        raise ValueError(f"Could not interpret regularizer config: {config!r}")
    cls = _BUILTIN.get(config["class_name"])
    if cls is None:
        raise ValueError(f"Unknown regularizer: {config['class_name']}")
    return cls.from_config(dict(config.get("config") or {}))


def get(identifier):
    """None, a regularizer object, one of the names 'l1' / 'l2' / 'l1_l2', or a {"class_name", "config"} dict.
    NotImplementedError: a callable of one's own, or a subclass with its own __call__."""
    if identifier is None:
        return None
    if isinstance(identifier, Regularizer):
        identifier.pair()                            # refuses a regularizer of one's own
        return identifier
    if isinstance(identifier, (dict, str)):
        return deserialize(identifier)
    if callable(identifier):
        raise NotImplementedError(f"regularizer {getattr(identifier, '__name__', identifier)!r}: a regularizer of one's own "
                                  "cannot run in the kernels; use a built-in Keras regularizer")
    raise ValueError(f"Could not interpret regularizer identifier: {identifier!r}")


def from_pair(l1, l2):
    """The built-in regularizer of a coefficient pair, in its shortest spelling; None for (0, 0)."""
    if l1 == 0 and l2 == 0:
        return None
    if l1 == 0:
        return L2(l2)
    if l2 == 0:
        return L1(l1)
    return L1L2(l1, l2)


def coefficients(specs, kernel=None, bias=None, gamma=None, beta=None):
    """{variable name: (l1, l2)} over `specs` (params.param_specs(): [(name, shape, kind)]) for the variables whose pair is
    not (0, 0): each <kind> regularizer (anything get() accepts) applies to every variable of that kind."""
    by_kind = {}
    for kind, ident in zip(KINDS, (kernel, bias, gamma, beta)):
        reg = get(ident)
        if reg is not None and reg.pair() != (0.0, 0.0):
            by_kind[kind] = reg.pair()
    return {name: by_kind[kind] for name, _, kind in specs if kind in by_kind}
