"""tf.keras.mixed_precision for this model: a dtype policy chosen before a Model is built.

    from lisec_amd import mixed_precision
    mixed_precision.set_global_policy('mixed_bfloat16')
    model = load_model(path)            # predict() / evaluate() multiply in bfloat16, variables stay float32

Two policies exist.  'float32' (the default) is the model as it always was.  'mixed_bfloat16' keeps float32 variables
and float32 activations in memory and runs the 3x3 contractions of inference -- the Conv3D blocks behind the first and
the Conv2Ds of the RPN -- with bfloat16 operands on the bf16 matrix cores (csrc/igemm_bf16.hip).  Deviations from Keras,
all stated in INTEGRATION.md: the VFE, the first Conv3D, the Dense(64) layers and the heads stay float32; training under
the policy is refused; save() does not persist the policy."""

_IMPLEMENTED = ("float32", "mixed_bfloat16")
_KERAS_ONLY = ("mixed_float16", "bfloat16", "float16", "float64")


class Policy:
    """tf.keras.mixed_precision.Policy: `name`, `compute_dtype`, `variable_dtype`."""

    def __init__(self, name):
        if isinstance(name, Policy):
            name = name.name
        if not isinstance(name, str):
            raise TypeError(f"'name' must be a string, but got: {name!r}")
        if name in _KERAS_ONLY:
            raise NotImplementedError(
                f"dtype policy '{name}' is not implemented; the policies that exist are 'float32' and 'mixed_bfloat16'")
        if name not in _IMPLEMENTED:
            raise ValueError(
                f"Cannot convert value {name} to a mixed precision Policy. Valid policies include 'float32' and "
                f"'mixed_bfloat16'.")
        self._name = name

    @property
    def name(self):
        return self._name

    @property
    def compute_dtype(self):
        return "bfloat16" if self._name == "mixed_bfloat16" else "float32"

    @property
    def variable_dtype(self):
        return "float32"

    def get_config(self):
        return {"name": self._name}

    @classmethod
    def from_config(cls, config, custom_objects=None):
        del custom_objects
        return cls(**config)

    def __eq__(self, other):
        return isinstance(other, Policy) and other.name == self._name

    def __hash__(self):
        return hash(self._name)

    def __repr__(self):
        return f'<Policy "{self._name}">'


_global_policy = Policy("float32")


def global_policy():
    """The policy a Model built now takes."""
    return _global_policy


def set_global_policy(policy):
    """policy: a Policy, the name of one, or None (= 'float32').  Models that exist keep the policy they were built under."""
    global _global_policy
    _global_policy = Policy("float32") if policy is None else (policy if isinstance(policy, Policy) else Policy(policy))
