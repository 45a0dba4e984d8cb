"""The VoxelNet detection loss without a GPU: the fp64 definition (tests/detection_loss_ref.py) against finite differences
of itself and against plain sigmoid cross-entropy, and what compile() makes of losses.VoxelNetLoss: config and
serialization round trips, the DetectionLossSpec and every refusal."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import detection_loss_ref as R  # noqa: E402
from lisec_amd import keras_h5, losses as K  # noqa: E402


def _point(seed, M=7, b=1.0):
    """Codes of all three kinds on both anchors; every SmoothL1 residual at least 0.05 away from the kink |d| = b (S is
    smooth at d = 0)."""
    rng = np.random.default_rng(seed)
    head = rng.normal(0, 1.5, (M, 16))
    y_cls = rng.integers(0, 3, (M, 2)).astype(np.float64)
    y_cls[0], y_cls[1] = (2, 1), (0, 2)
    y_reg = rng.normal(0, 1.0, (M, 14)) + 1.0
    d = head[:, 2:] - (y_reg - 1.0)
    near = np.abs(np.abs(d) - b) < 0.05
    head[:, 2:] += np.where(near, 0.2 * np.sign(d), 0.0)
    return head, y_cls, y_reg


@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("b", [1.0, 1.0 / 9.0])
def test_gradient_is_the_finite_difference_of_the_loss(gamma, b):
    head, y_cls, y_reg = _point(3, b=b)
    kw = dict(alpha=1.5, beta=0.7, gamma=gamma, smooth_l1_beta=b, weights=(2.0, 0.5))
    _, counts, g = R.detection_loss(head, y_cls, y_reg, grad_scale=0.75, **kw)
    assert counts[0] > 0 and counts[1] > 0 and counts.sum() < 14
    h = 1e-6
    fd = np.zeros_like(head)
    for i in range(head.shape[0]):
        for j in range(16):
            up, dn = head.copy(), head.copy()
            up[i, j] += h
            dn[i, j] -= h
            fd[i, j] = 0.75 * (R.loss_only(up, y_cls, y_reg, **kw)[0] - R.loss_only(dn, y_cls, y_reg, **kw)[0]) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-9)
    pos, neg = R.masks(y_cls)
    assert not g[:, :2][~(pos | neg)].any() and not g[:, 2:].reshape(-1, 2, 7)[~pos].any()


def test_paper_form_reduces_to_mean_sigmoid_cross_entropy():
    """gamma=0, alpha=beta=1, no ignored anchor, N_pos == N_neg == M: L_cls = 2 * mean over the 2M anchors of the sigmoid
    cross-entropy with labels pos -> 1, neg -> 0 (each half is a mean over M)."""
    rng = np.random.default_rng(5)
    M = 12
    head = rng.normal(0, 2, (M, 16))
    y_cls = np.tile([2.0, 1.0], (M, 1))
    y_cls[::2] = (1.0, 2.0)
    loss, counts, _ = R.detection_loss(head, y_cls, np.zeros((M, 14)), alpha=1.0, beta=1.0)
    assert counts.tolist() == [M, M]
    z, t = head[:, :2], (y_cls > 1.5).astype(np.float64)
    ce = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
    np.testing.assert_allclose(loss[1], 2.0 * ce.mean(), rtol=1e-13)


def test_extreme_logits_and_empty_classes_stay_finite():
    head = np.zeros((4, 16))
    head[:, 0], head[:, 1] = (1e4, -1e4, 80.0, -80.0), (0.0, 1e4, -1e4, 80.0)
    for y in (np.zeros((4, 2)), np.ones((4, 2)), np.full((4, 2), 2.0)):
        for gamma in (0.0, 2.0):
            loss, counts, g = R.detection_loss(head, y, np.ones((4, 14)), gamma=gamma)
            assert np.isfinite(loss).all() and np.isfinite(g).all()
            if not y.any():
                assert not loss.any() and not g.any() and counts.tolist() == [0, 0]
    head[2, 0] = np.nan
    loss, _, g = R.detection_loss(head, np.ones((4, 2)), np.ones((4, 14)))
    assert np.isnan(loss[0]) and np.isnan(g[2, 0]) and np.isfinite(g[3]).all()


# ---- losses.VoxelNetLoss and compile() ----------------------------------------------------------------------------------
def test_config_and_serialization_round_trip():
    loss = K.VoxelNetLoss(alpha=0.5, beta=1.5, gamma=2.0, smooth_l1_beta=1.0 / 9.0, target_offset=0.0, name="focal")
    cfg = loss.get_config()
    assert cfg == dict(reduction="auto", name="focal", alpha=0.5, beta=1.5, gamma=2.0, smooth_l1_beta=1.0 / 9.0,
                       target_offset=0.0)
    assert K.VoxelNetLoss.from_config(cfg).get_config() == cfg
    ser = K.serialize(loss)
    assert ser == {"class_name": "VoxelNetLoss", "config": cfg}
    back = K.deserialize(ser)
    assert isinstance(back, K.VoxelNetLoss) and back.get_config() == cfg
    assert isinstance(K.get(ser), K.VoxelNetLoss) and K.get(loss) is loss
    assert K.get("voxelnet") == "voxelnet" and K.serialize("voxelnet") == "voxelnet" and K.deserialize("voxelnet") == "voxelnet"
    assert K.VoxelNetLoss().get_config() == dict(reduction="auto", name="voxelnet_loss", alpha=1.5, beta=1.0, gamma=0.0,
                                                 smooth_l1_beta=1.0, target_offset=1.0)
    # what save() writes into training_config comes back as an equal spec
    tc = keras_h5._training_config(None, loss=loss, loss_weights=[2.0, 0.5])
    again, _ = K.compile_loss(K.deserialize(tc["loss"]), loss_weights=tc["loss_weights"])
    assert again == K.compile_loss(loss, loss_weights=[2.0, 0.5])[0]


def test_compile_loss_returns_a_hashable_detection_spec():
    spec, names = K.compile_loss("voxelnet")
    assert isinstance(spec, K.DetectionLossSpec) and names == [] and spec.n_metrics == 0
    assert spec.params == (1.5, 1.0, 0.0, 1.0, 1.0) and spec.weights == (1.0, 1.0)
    assert spec == K.compile_loss(K.VoxelNetLoss())[0] == K.compile_loss("VoxelNet", metrics=[])[0]
    assert hash(spec) == hash(K.compile_loss(K.VoxelNetLoss())[0])
    weighted, _ = K.compile_loss("voxelnet", loss_weights=[2, .5])
    assert weighted != spec and weighted.weights == (2.0, 0.5) and len({spec, weighted}) == 2
    assert weighted == K.compile_loss("voxelnet", loss_weights={"ClassificationLayer": 2, "RegressionLayer": .5})[0]
    focal, _ = K.compile_loss(K.VoxelNetLoss(gamma=2.0))
    assert focal != spec and len({spec, weighted, focal}) == 3
    assert spec != K.compile_loss("mae")[0] and spec != "mse"
    from lisec_amd.network import loss_acc_len
    assert loss_acc_len(spec) == 4
    # the other step losses are what they were
    assert K.compile_loss(["mse", "mse"]) == ("mse", []) and K.compile_loss("smoothl1_ce") == ("smoothl1_ce", [])


def test_descriptor_layout():
    import ctypes
    from lisec_amd import _lib
    d = K.compile_loss(K.VoxelNetLoss(alpha=0.25, beta=0.75, gamma=2.0, smooth_l1_beta=1 / 9, target_offset=0.0),
                       loss_weights=[2, .5])[0].descriptor()
    assert ctypes.sizeof(_lib.DetectionLossCfg) == 8 + 7 * 8 == d.struct_bytes and d.reserved == 0
    assert (d.alpha, d.beta, d.gamma, d.smooth_l1_beta, d.target_offset) == (0.25, 0.75, 2.0, 1 / 9, 0.0)
    assert list(d.weight) == [2.0, 0.5]


@pytest.mark.parametrize("kw", [dict(alpha=-1.0), dict(beta=-0.5), dict(gamma=-2.0), dict(smooth_l1_beta=0.0),
                                dict(smooth_l1_beta=-1.0), dict(alpha=float("nan")), dict(target_offset=float("inf"))])
def test_constructor_refuses_bad_parameters(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        K.VoxelNetLoss(**kw)


def test_constructor_refuses_another_reduction():
    with pytest.raises(NotImplementedError):
        K.VoxelNetLoss(reduction="sum")


@pytest.mark.parametrize("loss", [
    lambda: [K.VoxelNetLoss(), "mse"], lambda: ["mse", K.VoxelNetLoss()], lambda: [K.VoxelNetLoss(), K.VoxelNetLoss()],
    lambda: ["voxelnet", "mse"], lambda: {"ClassificationLayer": K.VoxelNetLoss(), "RegressionLayer": "mse"},
    lambda: {"ClassificationLayer": "mse", "RegressionLayer": "voxelnet"},
    lambda: [K.serialize(K.VoxelNetLoss()), "mse"]])
def test_per_output_use_is_refused_with_the_reason(loss):
    with pytest.raises(ValueError, match="joint loss of both outputs"):
        K.compile_loss(loss())


@pytest.mark.parametrize("metrics", [["mae"], [["accuracy"], []], {"RegressionLayer": ["mse"]}])
def test_metrics_are_refused(metrics):
    with pytest.raises(NotImplementedError, match="metrics"):
        K.compile_loss("voxelnet", metrics=metrics)
    with pytest.raises(NotImplementedError, match="metrics"):
        K.compile_loss(K.VoxelNetLoss(gamma=2.0), metrics=metrics)


def test_weighted_metrics_and_bad_weights_are_refused_as_for_the_other_losses():
    with pytest.raises(NotImplementedError):
        K.compile_loss("voxelnet", weighted_metrics=["mae"])
    with pytest.raises(ValueError):
        K.compile_loss("voxelnet", loss_weights=[1.0])
    with pytest.raises(ValueError):
        K.compile_loss("voxelnet", loss_weights={"NoSuchLayer": 1.0})
