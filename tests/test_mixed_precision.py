"""lisec_amd.mixed_precision: the tf.keras.mixed_precision surface (no GPU; the model-level checks are in
test_gpu_bf16_inference.py)."""
import pytest


@pytest.fixture(autouse=True)
def _restore_policy():
    from lisec_amd import mixed_precision as mp
    before = mp.global_policy()
    yield
    mp.set_global_policy(before)


def test_default_policy_is_float32():
    from lisec_amd import mixed_precision as mp
    p = mp.global_policy()
    assert (p.name, p.compute_dtype, p.variable_dtype) == ("float32", "float32", "float32")


def test_mixed_bfloat16_keeps_float32_variables():
    from lisec_amd import mixed_precision as mp
    p = mp.Policy("mixed_bfloat16")
    assert (p.name, p.compute_dtype, p.variable_dtype) == ("mixed_bfloat16", "bfloat16", "float32")


def test_set_global_policy_round_trip():
    from lisec_amd import mixed_precision as mp
    mp.set_global_policy("mixed_bfloat16")
    assert mp.global_policy().name == "mixed_bfloat16" and mp.global_policy() == mp.Policy("mixed_bfloat16")
    mp.set_global_policy(mp.Policy("float32"))
    assert mp.global_policy().name == "float32"
    mp.set_global_policy("mixed_bfloat16")
    mp.set_global_policy(None)
    assert mp.global_policy().name == "float32"


def test_config_round_trip():
    from lisec_amd import mixed_precision as mp
    p = mp.Policy("mixed_bfloat16")
    assert p.get_config() == {"name": "mixed_bfloat16"}
    q = mp.Policy.from_config(p.get_config())
    assert q == p and q is not p and hash(q) == hash(p) and q != mp.Policy("float32")


@pytest.mark.parametrize("name", ["mixed_float16", "bfloat16", "float16", "float64"])
def test_keras_policies_that_do_not_exist_here_are_named_as_such(name):
    from lisec_amd import mixed_precision as mp
    with pytest.raises(NotImplementedError) as e:
        mp.Policy(name)
    assert "'float32'" in str(e.value) and "'mixed_bfloat16'" in str(e.value)
    with pytest.raises(NotImplementedError):
        mp.set_global_policy(name)
    assert mp.global_policy().name == "float32"             # a refused policy changes nothing


@pytest.mark.parametrize("name", ["mixed_bfloat", "int8", "", "Float32"])
def test_unknown_policy_names_are_value_errors(name):
    from lisec_amd import mixed_precision as mp
    with pytest.raises(ValueError):
        mp.Policy(name)
    with pytest.raises(ValueError):
        mp.set_global_policy(name)


def test_policy_name_must_be_a_string():
    from lisec_amd import mixed_precision as mp
    with pytest.raises(TypeError):
        mp.Policy(16)


def test_training_entry_points_refuse_the_policy_before_any_work(monkeypatch):
    """train() / train_with_model() under 'mixed_bfloat16' raise before a sweep is voxelised (nothing here touches a GPU)."""
    from lisec_amd import mixed_precision as mp
    from lisec_amd import model_training as mt
    monkeypatch.setattr(mt, "_preprocess", lambda *a, **k: pytest.fail("preprocessing ran"))
    mp.set_global_policy("mixed_bfloat16")
    with pytest.raises(NotImplementedError):
        mt.train([], None, "unused.h5")
    with pytest.raises(NotImplementedError):
        mt.train_with_model([], None, "unused_in.h5", "unused.h5")
