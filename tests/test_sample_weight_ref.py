"""The fp64 definition of the sample-weighted losses (tests/sample_weight_ref.py) without a GPU: at unit weights it is
the unweighted references the loss tests already use, and on two cells it gives what the formulas give by hand."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import detection_iou_cases as C  # noqa: E402
import detection_iou_loss_ref as IOU  # noqa: E402
import detection_loss_ref as DET  # noqa: E402
import sample_weight_ref as SW  # noqa: E402
from lisec_amd import losses as K  # noqa: E402
from test_gpu_detection_loss import _case as det_case  # noqa: E402
from test_gpu_losses import LEGACY_CE, TERMS, _spec, ref_head_loss  # noqa: E402


def _head_inputs(M, seed, positive):
    rng = np.random.default_rng(seed)
    head = rng.normal(0, 1.2, (M, 16)).astype(np.float32)
    if positive:
        head = np.abs(head) + np.float32(0.01)
    return head, rng.choice(np.float32([0, 1, 2, -1]), (M, 2)), rng.normal(0, 1, (M, 14)).astype(np.float32)


@pytest.mark.parametrize("name", sorted(TERMS) + ["legacy_ce"])
def test_unit_weights_are_the_unweighted_head_reference(name):
    terms = LEGACY_CE if name == "legacy_ce" else (TERMS[name], TERMS[name])
    spec = _spec(*terms)
    M = 37
    head, yc, yr = _head_inputs(M, 5, name == "poisson")
    rl, rm, rg = ref_head_loss(spec, head, yc, yr, grad_scale=0.75)
    for w in ((None, None), (1.0, 1.0), (np.ones(M), None), (np.ones(M), np.ones(M))):
        for weighted in (((), ()), ((0, 1, 2, 3), (0, 1, 2, 3))):
            loss, pairs, grad = SW.head_loss(spec, head, yc, yr, w=w, weighted=weighted, grad_scale=0.75)
            np.testing.assert_allclose(loss, rl, rtol=1e-14)
            np.testing.assert_allclose(pairs[:, 0] / pairs[:, 1], rm, rtol=1e-14)
            np.testing.assert_allclose(grad, rg, rtol=1e-14, atol=0)
    # the denominators of unweighted pairs are the counts: elements, or cells for the categorical accuracy ('accuracy'
    # of the class output, 'acc' of the regression output)
    assert pairs[:, 1].tolist() == [2 * M, M, 2 * M, 2 * M, 14 * M, 14 * M, 14 * M, M]


@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("pattern", ["mix", "positives", "ignored"])
def test_unit_weights_are_the_unweighted_detection_reference(pattern, gamma):
    M = 257
    head, y_cls, y_reg = det_case(pattern, M, 1.0 / 9.0, seed=3)
    params = dict(alpha=0.5, beta=1.5, gamma=gamma, smooth_l1_beta=1.0 / 9.0)
    rl, rc, rg = DET.detection_loss(head, y_cls, y_reg, weights=(2.0, 0.5), grad_scale=0.75, **params)
    for w in ((None, None), (1.0, np.ones(M))):
        loss, counts, grad = SW.detection_loss(head, y_cls, y_reg, w=w, weights=(2.0, 0.5), grad_scale=0.75, **params)
        assert np.array_equal(counts, rc)
        np.testing.assert_allclose(loss, rl, rtol=1e-13)
        np.testing.assert_allclose(grad, rg, rtol=1e-13, atol=0)


@pytest.mark.parametrize("combo", [1, 3])
def test_unit_weights_are_the_unweighted_iou_reference(combo):
    M = 17
    head, y_cls, y_reg = C.case("positives", M, combo)
    det, iou = C.params(combo)
    rl, rc, rg = IOU.detection_iou_loss(head, y_cls, y_reg, weights=C.WEIGHTS, grad_scale=C.GRAD_SCALE, **det, **iou)
    loss, counts, grad = SW.detection_loss(head, y_cls, y_reg, w=(np.ones(M), 1.0), weights=C.WEIGHTS,
                                           grad_scale=C.GRAD_SCALE, iou=iou, **det)
    assert np.array_equal(counts, rc)
    np.testing.assert_allclose(loss, rl, rtol=1e-13)
    np.testing.assert_allclose(grad, rg, rtol=1e-12, atol=1e-15)


def test_two_cells_of_keras_losses_by_hand():
    """MSE on both outputs, two cells, weights (3, 0.5) on the class output and a sweep weight 2 on the regression
    output.  Class errors: cell 0 (1, -1), cell 1 (2, 0); regression errors: 1 on every element of cell 0, 0 on cell 1."""
    spec = K.LossSpec((TERMS["mse"], TERMS["mse"]), (1.5, 0.25),
                      (((K.MAE, 0, 0.0, 0.0), (K.CATEGORICAL_ACCURACY, 0, 0.0, 0.0)), ((K.MAE, 0, 0.0, 0.0),)))
    head = np.zeros((2, 16))
    yc = np.array([[-1.0, 1.0], [-2.0, 0.0]])          # e = p - t
    yr = np.zeros((2, 14))
    yr[0] = -1.0
    loss, pairs, grad = SW.head_loss(spec, head, yc, yr, w=(np.array([3.0, 0.5]), 2.0), weighted=((0, 1), ()))
    l_cls = (3.0 * (1 + 1) + 0.5 * (4 + 0)) / 4         # divisor M*C = 4, not the sum of the weights
    l_reg = (2.0 * 14 + 2.0 * 0) / 28
    assert loss.tolist() == [1.5 * l_cls + 0.25 * l_reg, l_cls, l_reg]
    # weighted MAE of the class output: sum w|e| / sum w over elements; its accuracy over cells: argmax p = 0 on both
    # cells, argmax t = 1 on cell 0 (a miss) and 1 -> index 1 on cell 1 too (t = (-2, 0)): both miss
    assert pairs[0].tolist() == [3.0 * 2 + 0.5 * 2, 2 * 3.5] and pairs[1].tolist() == [0.0, 3.5]
    assert pairs[2].tolist() == [14.0, 28.0]            # under metrics=: unweighted although the output has a weight
    assert grad[0, :2].tolist() == [1.5 * 3.0 * 2 * 1 / 4, 1.5 * 3.0 * 2 * -1 / 4]
    assert grad[1, :2].tolist() == [1.5 * 0.5 * 2 * 2 / 4, 0.0]
    assert np.array_equal(grad[0, 2:], np.full(14, 0.25 * 2.0 * 2 * 1 / 28)) and not grad[1, 2:].any()
    # weights that sum to zero: the pair divides to 0.0
    _, pairs, _ = SW.head_loss(spec, head, yc, yr, w=(np.array([1.0, -1.0]), None), weighted=((0, 1), ()))
    assert pairs[0, 1] == 0.0 and SW.div_no_nan(*pairs[0]) == 0.0 and SW.div_no_nan(*pairs[1]) == 0.0


def test_two_cells_of_the_detection_loss_by_hand():
    """Cell 0: anchor 0 positive with logit 0 and residual 0.5 on one channel, anchor 1 negative with logit 0.  Cell 1:
    both ignored, but weighted -- an ignored anchor stays out whatever its weight.  gamma = 0, b = 1."""
    head = np.zeros((2, 16))
    y_cls = np.array([[2.0, 1.0], [0.0, 0.0]])
    y_reg = np.ones((2, 14))                            # t = 0 after the offset
    head[0, 2] = 0.5
    w = (np.array([4.0, 100.0]), np.array([0.5, 100.0]))
    loss, counts, grad = SW.detection_loss(head, y_cls, y_reg, w=w, weights=(2.0, 3.0), alpha=1.5, beta=1.0)
    assert counts.tolist() == [1, 1]                    # unweighted counts
    ln2 = np.log(2.0)
    np.testing.assert_allclose(loss[1], 1.5 * 4.0 * ln2 + 1.0 * 4.0 * ln2, rtol=1e-15)
    np.testing.assert_allclose(loss[2], 0.5 * (0.5 * 0.5 / 2), rtol=1e-15)
    np.testing.assert_allclose(loss[0], 2.0 * loss[1] + 3.0 * loss[2], rtol=1e-15)
    np.testing.assert_allclose(grad[0, :3], [2.0 * 1.5 * 4.0 * -0.5, 2.0 * 1.0 * 4.0 * 0.5, 3.0 * 0.5 * 0.5], rtol=1e-15)
    assert not grad[0, 3:].any() and not grad[1].any()
    # a zero weight removes the anchor's loss, not its count
    loss0, counts0, grad0 = SW.detection_loss(head, y_cls, y_reg, w=(0.0, 0.0), weights=(2.0, 3.0))
    assert counts0.tolist() == [1, 1] and not loss0.any() and not grad0.any()


def test_weighted_metrics_compile_behind_an_outputs_metrics_and_share_its_cap():
    from lisec_amd import model_training as mt
    spec, names = K.compile_weighted_loss("mae", metrics={"ClassificationLayer": ["binary_accuracy"]},
                                          weighted_metrics=["mae", "accuracy"])
    assert names == ["ClassificationLayer_binary_accuracy", "ClassificationLayer_weighted_mae",
                     "ClassificationLayer_weighted_accuracy", "RegressionLayer_weighted_mae", "RegressionLayer_weighted_accuracy"]
    assert spec.weighted == (0b110, 0b11) and [len(m) for m in spec.metrics] == [3, 2]
    plain, _ = K.compile_weighted_loss("mae", metrics={"ClassificationLayer": ["binary_accuracy", "mae", "accuracy"],
                                                       "RegressionLayer": ["mae", "accuracy"]})
    assert plain.metrics == spec.metrics and plain != spec and plain.weighted == (0, 0)
    assert K.compile_weighted_loss("mse") == ("mse", []) and K.compile_loss("mse", metrics=["mae"])[0].weighted == (0, 0)
    with pytest.raises(ValueError):                     # metrics and weighted_metrics share the cap of 4 per output
        K.compile_weighted_loss("mse", metrics=["mae", "mse", "mape"], weighted_metrics=["mae", "mse"])
    with pytest.raises(ValueError):
        K.compile_weighted_loss("mse", weighted_metrics=["mae", "mae"])
    for loss in ("voxelnet", "voxelnet_iou"):
        with pytest.raises(NotImplementedError):
            K.compile_weighted_loss(loss, weighted_metrics=["mae"])
    with pytest.raises(NotImplementedError):            # a step compiled without sample weights keeps refusing them
        K.compile_loss("mse", weighted_metrics=["mae"])
    # an array without rows weighs nothing
    for w in (np.ones(0), [None, np.ones((0, 8, 16))], {"RegressionLayer": []}):
        with pytest.raises(NotImplementedError, match="sample_weight"):
            mt._refuse_empty_sample_weight(w)
    for w in (None, [None, None], np.ones(2), {"RegressionLayer": np.ones((1, 8, 16))}):
        mt._refuse_empty_sample_weight(w)
    assert mt._sample_weight_arrays([None, None], 3, (8, 16)) is None
    assert mt._weight_form(mt._sample_weight_arrays([np.ones((3, 8, 16)), np.ones(4)], 3, (8, 16))) == ("cell", "sweep")
    for bad in (np.ones((3, 4)), np.ones((3, 16, 8)), np.ones(2), [np.ones(3)], {"Other": np.ones(3)}, np.float32([1, np.nan, 1])):
        with pytest.raises(ValueError):
            mt._sample_weight_arrays(bad, 3, (8, 16))
