"""The full-grid gradient check of tests/test_gpu_network.py (gradient_rows + _check_gradients) must fail on a wrong
gradient, not only pass on a right one.  CPU only: synthetic gradients whose fp32 noise follows what was measured at the
Lyft grid (profiles/r02_grad_conditioning_u20k_mse.txt): ~0.75 % relative L2 for every tensor behind an RPN block's last
BatchNormalization, 1e-6 or less for the up-sampling branches and the heads."""
import numpy as np
import pytest

import test_gpu_network as N

# name, shape, relative L2 noise of an fp32 evaluation (the measured floor of that kind of tensor)
TENSORS = [(f"mid{i}.conv.kernel", (3, 3, 3, 64, 64), 7.5e-3) for i in (1, 2, 3)] + \
          [(f"mid{i}.bn.gamma", (64,), 7.5e-3) for i in (1, 2, 3)] + \
          [(f"rpn{b}.conv{j}.kernel", (3, 3, 64, 64), 6e-3) for b in (1, 2, 3) for j in range(4)] + \
          [(f"rpn{b}.bn{j}.beta", (64,), 6e-3) for b in (1, 2, 3) for j in range(4)] + \
          [("rpn1.bn3.gamma", (128,), 3e-4), ("up1.kernel", (3, 3, 128, 256), 4e-7), ("up2.kernel", (3, 3, 128, 256), 8e-7),
           ("up3.kernel", (3, 3, 256, 256), 1.5e-6), ("cls.kernel", (768, 2), 2e-6), ("reg.kernel", (768, 14), 4e-7),
           ("mid1.conv.bias", (64,), 0.0)]


def _noisy(rng, ref, rel):
    """ref plus Gaussian noise of relative L2 size `rel`."""
    noise = rng.normal(0, 1, ref.shape)
    return ref + noise * (rel * np.linalg.norm(ref) / max(np.linalg.norm(noise), 1e-300))


def _case(gpu_factor=1.0, off=None, off_by=0.0, seed=0):
    """fp64 'truth', an fp32-oracle stand-in and a 'gpu' result whose noise is gpu_factor x the oracle's; tensor `off`
    is, in addition, scaled by (1 + off_by).  Returns (out, rows) as full_grid_gradient_report hands them over."""
    rng = np.random.default_rng(seed)
    ref, o32, got = {}, {}, {}
    for name, shape, rel in TENSORS:
        if name.endswith(".bias") and ".conv" in name:
            ref[name] = np.zeros(shape)                # a conv bias ahead of a training-mode BN: exact gradient 0
            o32[name] = rng.normal(0, 1e-9, shape)
            got[name] = rng.normal(0, 1e-8, shape)
            continue
        ref[name] = rng.normal(0, 1e-2, shape)
        o32[name] = _noisy(rng, ref[name], rel)
        got[name] = _noisy(rng, ref[name], gpu_factor * rel)
        if name == off:
            got[name] = got[name] * (1.0 + off_by)
    rows, l2, _ = N.gradient_rows(got, ref, o32)
    return dict(l2=l2), rows


def test_check_passes_gradients_at_the_fp32_noise_floor():
    out, rows = _case()
    assert "mid1.conv.bias" not in [r[0] for r in rows]
    med = N._check_gradients(out, rows, median_bound=1.3)
    assert 0.8 < med < 1.25


@pytest.mark.parametrize("name", ["up2.kernel", "cls.kernel", "rpn1.bn3.gamma"])
def test_check_fails_one_tensor_one_percent_off(name):
    """One tensor scaled by 1.01 where the fp32 floor is far below 1 % (branches, heads, an RPN block's last BN):
    the per-tensor rule names it.  (Behind a BN of a nearly constant map the floor is ~0.75 %, and a 1 % error there is
    within 3x of it: that is what the rule, by design, cannot tell from noise.)"""
    out, rows = _case(off=name, off_by=0.01)
    with pytest.raises(AssertionError, match=r"beyond max\(3e-3") as e:
        N._check_gradients(out, rows, median_bound=2.0)
    assert {n for n, *_ in TENSORS if f"{n}: L2 gpu" in str(e.value)} == {name}       # that tensor alone


def test_check_fails_a_global_loss_of_accuracy_by_its_median():
    """Every gradient with 2x the fp32 oracle's error: within SPREAD = 3 on each tensor, so only the median catches it,
    at the bound of the U20k test (1.3) and at the loosest in use (2.0, which 2.2x exceeds)."""
    out, rows = _case(gpu_factor=2.2)
    bad = [n for n, *_ in rows if out["l2"][n][0] > max(N.FLAT, N.SPREAD * out["l2"][n][1])]
    assert not bad                                     # the per-tensor rule alone lets it through
    for bound in (1.3, 2.0):
        with pytest.raises(AssertionError, match="median gpu/fp32-oracle error ratio"):
            N._check_gradients(out, rows, median_bound=bound)


def test_check_fails_a_mis_scaled_noisy_tensor():
    """A tensor behind a BN with a 5 % scale error (a wrong count or normaliser) is caught although its fp32 floor
    is 0.75 %."""
    out, rows = _case(off="mid2.conv.kernel", off_by=0.05)
    with pytest.raises(AssertionError, match="mid2.conv.kernel"):
        N._check_gradients(out, rows, median_bound=2.0)


def test_exact_zero_tensors_are_reported_apart():
    rng = np.random.default_rng(3)
    ref = {"a": np.zeros(8), "b": rng.normal(0, 1, 8)}
    got = {"a": np.full(8, 1e-9), "b": ref["b"] * (1 + 1e-7)}
    rows, l2, zero = N.gradient_rows(got, ref, {k: v.copy() for k, v in ref.items()}, exact_zero=("a",))
    assert [r[0] for r in rows] == ["b"] and set(l2) == {"b"}
    assert zero == {"a": (1e-9, 0.0, 0.0)}
