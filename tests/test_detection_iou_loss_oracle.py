"""The detection loss with the IoU term without a GPU: known answers of the fp64 definition
(tests/detection_iou_loss_ref.py), the condition the GPU tolerance rests on, checked on the reference alone for every
positive of the GPU cases (tests/detection_iou_cases.py), and what compile() makes of losses.VoxelNetIoULoss: config and
serialization round trips, the DetectionIoULossSpec, its descriptor and every refusal."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import detection_iou_cases as C  # noqa: E402
import detection_iou_loss_ref as R  # noqa: E402
import detection_loss_ref as R0  # noqa: E402
from lisec_amd import keras_h5, losses as K, metrics as KM  # noqa: E402


def _box(x=0.0, y=0.0, z=0.0, l=4.0, w=2.0, h=1.5, yaw=0.0):
    return np.array([[x, y, z, l, w, h, yaw]])


# ---- the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw", [0.0, 0.3, -1.2, math.pi / 2])
def test_known_ious(yaw):
    b = _box(x=0.7, y=-0.4, yaw=yaw)
    for mode in ("bev", "3d"):
        assert abs(R.iou(b, b, mode)[0] - 1.0) < 1e-12
    # shifted by half a width along u = (cos yaw, -sin yaw): the footprints share half of each, 1/2 / (2 - 1/2)
    half = _box(x=0.7 + math.cos(yaw) * 1.0, y=-0.4 - math.sin(yaw) * 1.0, yaw=yaw)
    assert abs(R.iou(b, half, "bev")[0] - 1.0 / 3.0) < 1e-12
    # turned by 90 degrees, l = 2 w: a w x w square out of two areas of 2 w^2
    assert abs(R.iou(b, _box(x=0.7, y=-0.4, yaw=yaw + math.pi / 2), "bev")[0] - 1.0 / 3.0) < 1e-12
    # disjoint, inside and outside the sum of the circumradii
    for far in (3.0, 30.0):
        assert R.iou(b, _box(x=0.7 + math.cos(yaw) * far, y=-0.4 - math.sin(yaw) * far, yaw=yaw), "bev")[0] == 0.0
    # half the height in common: (A h/2) / (2 A h - A h/2) = 1/3; disjoint heights: 0, whatever the footprints
    assert abs(R.iou(b, _box(x=0.7, y=-0.4, z=0.75, yaw=yaw), "3d")[0] - 1.0 / 3.0) < 1e-12
    assert R.iou(b, _box(x=0.7, y=-0.4, z=1.5, yaw=yaw), "3d")[0] == 0.0
    assert abs(R.iou(b, _box(x=0.7, y=-0.4, z=1.5, yaw=yaw), "bev")[0] - 1.0) < 1e-12


def test_zero_extents_and_non_finite_boxes_have_iou_zero():
    b = _box()
    assert R.iou(b, _box(l=0.0), "bev")[0] == 0.0 and R.iou(_box(w=0.0), b, "bev")[0] == 0.0
    assert R.iou(b, _box(h=0.0), "3d")[0] == 0.0 and R.iou(b, _box(h=0.0), "bev")[0] == 1.0
    an = np.array([R.ANCHORS[0]])
    r = np.zeros((1, 7))
    for k, v in ((3, 800.0), (0, np.inf), (6, np.nan)):
        bad = r.copy()
        bad[0, k] = v
        for mode in ("bev", "3d"):
            assert R.decoded_iou(bad, r, an, mode)[0] == 0.0 and R.decoded_iou(r, bad, an, mode)[0] == 0.0
            assert not R.iou_term_grad(bad, r, an, mode).any()


def test_decode_is_the_metrics_decode():
    import detection_metrics_ref as RM
    rng = np.random.default_rng(1)
    r, t = rng.normal(0, 0.4, (40, 7)), rng.normal(0, 0.3, (40, 7))
    for a in range(2):
        an = np.tile(R.ANCHORS[a], (40, 1))
        assert np.array_equal(R.decode(r, an), np.stack([RM.decode(v, R.ANCHORS[a]) for v in r]))
        for mode in ("bev", "3d"):
            want = [RM.decoded_iou(r[i], t[i], R.ANCHORS[a], mode) for i in range(40)]
            np.testing.assert_allclose(R.decoded_iou(r, t, an, mode), want, rtol=0, atol=1e-13)


def test_the_loss_extends_the_detection_loss():
    head, y_cls, y_reg = C.build("mix", 300, 1, seed=5)
    y_cls[:20] = 2.0
    base, counts0, grad0 = R0.detection_loss(head, y_cls, y_reg, weights=C.WEIGHTS, grad_scale=0.75, gamma=2.0)
    zero, counts, grad = R.detection_iou_loss(head, y_cls, y_reg, weights=C.WEIGHTS, grad_scale=0.75, gamma=2.0,
                                              iou_weight=0.0)
    assert np.array_equal(zero, base) and np.array_equal(counts, counts0) and np.array_equal(grad, grad0)
    for mode in ("bev", "3d"):
        loss, _, grad = R.detection_iou_loss(head, y_cls, y_reg, weights=C.WEIGHTS, grad_scale=0.75, gamma=2.0,
                                             iou_weight=2.0, iou_mode=mode)
        ious = R.decoded_iou(*R.positives(head, y_cls, y_reg)[2:], mode)
        assert 0 < ious.max() < 1 and ious.min() == 0
        assert abs(loss[2] - (base[2] + 2.0 * (1.0 - ious).mean())) < 1e-12 and loss[1] == base[1]
        assert abs(loss[0] - (2.0 * loss[1] + 0.5 * loss[2])) < 1e-12
        # the class channels and every anchor that is not positive are the detection loss's
        pos, _ = R0.masks(y_cls)
        assert np.array_equal(grad[:, :2], grad0[:, :2])
        assert np.array_equal(grad[:, 2:].reshape(-1, 2, 7)[~pos], grad0[:, 2:].reshape(-1, 2, 7)[~pos])
        changed = (grad != grad0)[:, 2:].reshape(-1, 2, 7)[pos]
        assert changed.any() and (mode == "3d" or not changed[:, [2, 5]].any())


@pytest.mark.parametrize("case", C.all_cases(), ids=lambda c: "%s-%d-%d" % c)
def test_difference_steps_agree_on_every_positive_of_the_gpu_cases(case):
    """What the GPU test's 1e-6 rests on: the reference gradient is a derivative, not a kink, at every positive --
    fd(1e-6) and fd(3e-6) agree to 1e-6 of the anchor's largest component, no anchor left out."""
    pattern, M, combo = case
    head, y_cls, y_reg = C.case(*case)
    dev, g1 = C.fd_disagreement(head, y_cls, y_reg, C.COMBOS[combo][0])
    assert len(dev) == (R0.masks(y_cls)[0]).sum() > 0
    assert dev.max() <= C.FD_AGREE, (int(dev.argmax()), float(dev.max()))


def test_all_three_overlap_regimes_are_exercised():
    share = {}
    for combo in range(3):
        head, y_cls, y_reg = C.case("positives", 257, combo)
        share[C.COMBOS[combo][1]] = (R.decoded_iou(*R.positives(head, y_cls, y_reg)[2:], "bev") > 0).mean()
    assert share[0.15] > 0.97 and 0.6 < share[0.5] < 0.95 and 0.1 < share[1.5] < 0.5


# ---- losses.VoxelNetIoULoss and compile() --------------------------------------------------------------------------------
def test_config_and_serialization_round_trip():
    loss = K.VoxelNetIoULoss(alpha=0.5, beta=1.5, gamma=2.0, smooth_l1_beta=1.0 / 9.0, target_offset=0.0, iou_weight=2.5,
                             iou_mode="3d", name="focal_iou")
    cfg = loss.get_config()
    assert cfg == dict(reduction="auto", name="focal_iou", alpha=0.5, beta=1.5, gamma=2.0, smooth_l1_beta=1.0 / 9.0,
                       target_offset=0.0, iou_weight=2.5, iou_mode="3d")
    assert set(cfg) == set(K.VoxelNetLoss().get_config()) | {"iou_weight", "iou_mode"}
    assert K.VoxelNetIoULoss.from_config(cfg).get_config() == cfg
    ser = K.serialize(loss)
    assert ser == {"class_name": "VoxelNetIoULoss", "config": cfg}
    back = K.deserialize(ser)
    assert type(back) is K.VoxelNetIoULoss and back.get_config() == cfg
    assert type(K.get(ser)) is K.VoxelNetIoULoss and K.get(loss) is loss
    for name in ("voxelnet_iou", "voxelnet_iou_loss"):
        assert K.get(name) == name and K.serialize(name) == name and K.deserialize(name) == name
        assert K.compile_loss(name)[0] == K.compile_loss(K.VoxelNetIoULoss())[0]
    assert K.VoxelNetIoULoss().get_config() == dict(
        reduction="auto", name="voxelnet_iou_loss", alpha=1.5, beta=1.0, gamma=0.0, smooth_l1_beta=1.0, target_offset=1.0,
        iou_weight=1.0, iou_mode="bev")
    # what save() writes into training_config comes back as an equal spec
    tc = keras_h5._training_config(None, loss=loss, loss_weights=[2.0, 0.5])
    assert tc["loss"]["class_name"] == "VoxelNetIoULoss"
    again, _ = K.compile_loss(K.deserialize(tc["loss"]), loss_weights=tc["loss_weights"])
    assert again == K.compile_loss(loss, loss_weights=[2.0, 0.5])[0]
    assert again == K.compile_loss(tc["loss"], loss_weights=[2.0, 0.5])[0]


def test_compile_loss_returns_a_hashable_spec_of_its_own():
    from lisec_amd import Constants
    from lisec_amd.network import loss_acc_len
    spec, names = K.compile_loss("voxelnet_iou")
    assert isinstance(spec, K.DetectionIoULossSpec) and isinstance(spec, K.DetectionLossSpec)
    assert names == [] and spec.n_metrics == 0 and loss_acc_len(spec) == 4
    assert spec.params == (1.5, 1.0, 0.0, 1.0, 1.0) and spec.weights == (1.0, 1.0)
    assert (spec.iou_weight, spec.iou_mode) == (1.0, "bev")
    assert spec.anchors == tuple(tuple(float(v) for v in a) for a in Constants.anchors)
    assert spec == K.compile_loss(K.VoxelNetIoULoss())[0] and hash(spec) == hash(K.compile_loss(K.VoxelNetIoULoss())[0])
    plain = K.compile_loss("voxelnet")[0]
    assert spec != plain and plain != spec and len({spec, plain}) == 2
    others = [K.compile_loss(K.VoxelNetIoULoss(iou_mode="3d"))[0], K.compile_loss(K.VoxelNetIoULoss(iou_weight=2.0))[0],
              K.compile_loss(K.VoxelNetIoULoss(iou_weight=0.0))[0], K.compile_loss(K.VoxelNetIoULoss(gamma=2.0))[0],
              K.compile_loss("voxelnet_iou", loss_weights=[2, .5])[0],
              K.DetectionIoULossSpec(spec.params, anchors=((1.0, 2.0, 1.5, 0.0), (1.0, 2.0, 1.5, 1.0)))]
    assert len({spec, plain, *others}) == 8 and all(o != plain for o in others)
    # with the detection metrics: the accumulator grows by a pair each, and the spec still differs from 'voxelnet' with them
    with_m, names = K.compile_loss("voxelnet_iou", metrics=[KM.PositiveIoU("3d"), "anchor_recall"])
    assert sorted(names) == ["ClassificationLayer_anchor_recall", "RegressionLayer_positive_iou"]
    assert with_m.n_metrics == 2 and loss_acc_len(with_m) == 8 and with_m != spec
    assert with_m != K.compile_loss("voxelnet", metrics=[KM.PositiveIoU("3d"), "anchor_recall"])[0]
    assert with_m.metrics_descriptor().n_metrics == 2
    # the other step losses are what they were
    assert type(plain) is K.DetectionLossSpec and plain.config == ((1.5, 1.0, 0.0, 1.0, 1.0), (1.0, 1.0))
    assert K.compile_loss(["mse", "mse"]) == ("mse", [])


def test_descriptor_layout():
    from lisec_amd import _lib
    anchors = ((1.0, 2.0, 1.5, 0.25), (3.0, 4.0, 2.5, 1.0))
    spec = K.DetectionIoULossSpec((0.25, 0.75, 2.0, 1 / 9, 0.0), (2, .5), anchors=anchors, iou_weight=2.5, iou_mode="3d")
    d = spec.descriptor()
    assert ctypes.sizeof(_lib.DetectionIoULossCfg) == 8 + (8 + 7 * 8) + 8 + 8 + 8 * 8 == d.struct_bytes
    assert d.reserved == 0 and d.reserved2 == 0
    assert d.det.struct_bytes == ctypes.sizeof(_lib.DetectionLossCfg) and d.det.reserved == 0
    assert (d.det.alpha, d.det.beta, d.det.gamma, d.det.smooth_l1_beta, d.det.target_offset) == (0.25, 0.75, 2.0, 1 / 9, 0.0)
    assert list(d.det.weight) == [2.0, 0.5]
    assert (d.iou_weight, d.iou_mode) == (2.5, 0) and K.compile_loss("voxelnet_iou")[0].descriptor().iou_mode == 1
    assert [list(a) for a in d.anchors] == [list(a) for a in anchors]


@pytest.mark.parametrize("kw", [dict(iou_weight=-1.0), dict(iou_weight=float("nan")), dict(iou_weight=float("inf")),
                                dict(iou_mode="2d"), dict(iou_mode=None), dict(alpha=-1.0), dict(smooth_l1_beta=0.0)])
def test_constructor_refuses_bad_parameters(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        K.VoxelNetIoULoss(**kw)
    with pytest.raises(NotImplementedError):
        K.VoxelNetIoULoss(reduction="sum")


@pytest.mark.parametrize("loss", [
    lambda: [K.VoxelNetIoULoss(), "mse"], lambda: ["mse", K.VoxelNetIoULoss()], lambda: ["voxelnet_iou", "mse"],
    lambda: {"ClassificationLayer": K.VoxelNetIoULoss(), "RegressionLayer": "mse"},
    lambda: {"ClassificationLayer": "mse", "RegressionLayer": "voxelnet_iou_loss"},
    lambda: [K.serialize(K.VoxelNetIoULoss()), "mse"]])
def test_per_output_use_is_refused_with_the_reason(loss):
    with pytest.raises(ValueError, match="joint loss of both outputs"):
        K.compile_loss(loss())


@pytest.mark.parametrize("metrics", [["mae"], [["accuracy"], []], {"RegressionLayer": ["mse"]}])
def test_keras_metrics_are_refused_and_detection_metrics_accepted(metrics):
    with pytest.raises(NotImplementedError, match="metrics"):
        K.compile_loss("voxelnet_iou", metrics=metrics)
    with pytest.raises(NotImplementedError):
        K.compile_loss("voxelnet_iou", weighted_metrics=["mae"])
    spec, names = K.compile_loss(K.VoxelNetIoULoss(iou_mode="3d"), metrics=["positive_iou", "positive_mae"])
    assert spec.n_metrics == 2 and len(names) == 2
