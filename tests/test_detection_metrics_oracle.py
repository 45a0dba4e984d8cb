"""The detection metrics without a GPU: the fp64 definitions of tests/detection_metrics_ref.py on hand-worked cases (counts
by inspection), and what compile() makes of metrics= next to the VoxelNet detection loss (lisec_amd/metrics.py,
lisec_amd/losses.py): acceptance, routing, names, refusals, the spec as a plan key, serialization."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import detection_metrics_ref as R  # noqa: E402
from lisec_amd import losses as K  # noqa: E402
from lisec_amd import metrics as Mx  # noqa: E402

NAN = float("nan")
CLS, REG = "ClassificationLayer_", "RegressionLayer_"
FIVE = ["anchor_precision", "anchor_recall", "anchor_accuracy", "positive_mae", "positive_iou"]


def _maps(M):
    """An all-ignored sweep whose regression output equals its target (y_reg carries the +1)."""
    return np.zeros((M, 16)), np.zeros((M, 2)), np.ones((M, 14))


# ---- the definitions, by hand ------------------------------------------------------------------------------------------
def test_counts_by_inspection():
    head, y_cls, y_reg = _maps(4)
    #            anchor 0                  anchor 1
    y_cls[:] = [[2, 1],                  # pos, p = .88 (hit)        neg, p = .12 (rejected)
                [2, 1],                  # pos, p = .12 (missed)     neg, p = .88 (false alarm)
                [0, 2],                  # ignored, p = .88          pos, p = .5: NOT > 0.5 (missed)
                [1, 0]]                  # neg, p = .27              ignored
    head[:, :2] = [[2, -2], [-2, 2], [2, 0], [-1, 5]]
    assert R.anchor_precision(head, y_cls) == (1.0, 2.0)
    assert R.anchor_recall(head, y_cls) == (1.0, 3.0)
    assert R.anchor_accuracy(head, y_cls) == (3.0, 6.0)            # hit + two rejected negatives of 3 pos + 3 neg
    # threshold 0.3: the p = .5 positive is now hit, nothing else moves (.27 and .12 stay below)
    assert R.anchor_precision(head, y_cls, 0.3) == (2.0, 3.0)
    assert R.anchor_recall(head, y_cls, 0.3) == (2.0, 3.0)
    assert R.anchor_accuracy(head, y_cls, 0.3) == (4.0, 6.0)
    # threshold 0.9: nothing is predicted; precision's denominator is 0 and its value 0.0
    assert R.anchor_precision(head, y_cls, 0.9) == (0.0, 0.0) and R.value([R.anchor_precision(head, y_cls, 0.9)]) == 0.0
    assert R.anchor_accuracy(head, y_cls, 0.9) == (3.0, 6.0)


def test_nan_code_is_ignored_and_nan_logit_is_predicted_negative():
    head, y_cls, y_reg = _maps(2)
    y_cls[:] = [[NAN, 2], [1, 2]]
    head[:, :2] = [[9, NAN], [NAN, 9]]
    assert R.anchor_precision(head, y_cls) == (1.0, 1.0)           # the NaN-coded anchor at p = 1 counts nowhere
    assert R.anchor_recall(head, y_cls) == (1.0, 2.0)              # the NaN-logit positive is missed
    assert R.anchor_accuracy(head, y_cls) == (2.0, 3.0)            # the NaN-logit negative is rejected: correct
    assert R.positive_mae(head, y_cls, y_reg) == (0.0, 14.0)
    assert R.positive_iou(head, y_cls, y_reg) == (2.0, 2.0)


def test_no_positives_and_no_anchors_give_zero():
    head, y_cls, y_reg = _maps(3)
    for name in FIVE:
        assert R.pair(name, head, y_cls, y_reg) == (0.0, 0.0) and R.value([R.pair(name, head, y_cls, y_reg)]) == 0.0
    y_cls[:] = 1                                                   # negatives only, every p = 0.5: none predicted
    assert R.anchor_recall(head, y_cls) == (0.0, 0.0) and R.anchor_accuracy(head, y_cls) == (6.0, 6.0)
    assert R.positive_mae(head, y_cls, y_reg) == (0.0, 0.0) and R.positive_iou(head, y_cls, y_reg) == (0.0, 0.0)
    # pooling: a sweep without positives adds nothing and does not poison the epoch
    assert R.value([(0.0, 0.0), (3.0, 4.0), (0.0, 0.0)]) == 0.75


def test_positive_mae_by_hand():
    head, y_cls, y_reg = _maps(2)
    y_cls[0, 1] = y_cls[1, 0] = 2
    head[0, 9:16] = [1, -1, 0.5, 0, 0, 0, 2]                      # anchor 1 of cell 0: |d| sums to 4.5
    head[1, 2:9] = 0.25                                           # anchor 0 of cell 1: 7 * 0.25
    head[0, 2:9] = 100                                            # not a positive: not looked at
    assert R.positive_mae(head, y_cls, y_reg) == (4.5 + 1.75, 14.0)
    # target_offset is the compiled loss's: with 0 the targets are 1 everywhere
    assert R.positive_mae(head, y_cls, y_reg, target_offset=0.0)[0] == pytest.approx(2 + 0 + .5 + 1 + 1 + 1 + 1 + 7 * .75)


def test_positive_iou_by_hand():
    head, y_cls, y_reg = _maps(3)
    y_cls[:, 1] = 2                                               # anchor 1 (yaw pi/2: its length lies along x)
    head[0, 9:16] = 0                                             # r == t: IoU 1
    head[1, 9] = 0.5                                              # centre moved by half a length along the length: 1/3
    head[2, 11] = 0.5                                             # centre raised by half a height
    bev, i3d = (R.positive_ious(head, y_cls, y_reg, mode) for mode in ("bev", "3d"))
    np.testing.assert_allclose(bev, [1.0, 1.0 / 3.0, 1.0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(i3d, [1.0, 1.0 / 3.0, 1.0 / 3.0], rtol=0, atol=1e-12)
    assert R.positive_iou(head, y_cls, y_reg)[1] == 3.0
    # both boxes grown alike keep IoU 1; a box twice as long inside... holds the other: 1/2
    head[0, 12:15] = y_reg[0, 10:13] - 1 + 0.7
    y_reg[0, 10:13] += 0.7
    head[1, 9] = 0
    head[1, 12] = np.log(2.0)
    np.testing.assert_allclose(R.positive_ious(head, y_cls, y_reg, "bev")[:2], [1.0, 0.5], rtol=0, atol=1e-12)


def test_overflowing_extent_is_iou_zero_but_counted():
    head, y_cls, y_reg = _maps(2)
    y_cls[:, 0] = 2
    head[1, 5] = 1000.0                                           # r3: exp overflows
    for mode in ("bev", "3d"):
        assert R.positive_iou(head, y_cls, y_reg, mode) == (1.0, 2.0)
    head[1, 5], head[1, 2] = 0.0, NAN                             # a NaN offset likewise
    assert R.positive_iou(head, y_cls, y_reg) == (1.0, 2.0)
    head[1, 2], head[1, 8] = 0.0, np.inf                          # an infinite yaw: the IoU itself is not finite
    assert R.positive_iou(head, y_cls, y_reg) == (1.0, 2.0)
    head[1, 8], head[1, 6] = 0.0, -1000.0                         # exp underflows to a zero extent: IoU 0 by definition
    assert R.positive_iou(head, y_cls, y_reg) == (1.0, 2.0)


# ---- compile(): acceptance ---------------------------------------------------------------------------------------------
def test_flat_list_routes_each_metric_to_its_output_class_output_first():
    spec, names = K.compile_loss("voxelnet", metrics=["positive_iou", "anchor_recall", "positive_mae", "anchor_precision",
                                                      "anchor_accuracy"])
    assert names == [CLS + "anchor_recall", CLS + "anchor_precision", CLS + "anchor_accuracy", REG + "positive_iou",
                     REG + "positive_mae"]
    assert isinstance(spec, K.DetectionLossSpec) and spec.n_metrics == 5 and list(spec.metric_names) == names
    assert spec.metrics == ((Mx.ANCHOR_RECALL, 0, 0.5), (Mx.ANCHOR_PRECISION, 0, 0.5), (Mx.ANCHOR_ACCURACY, 0, 0.5),
                            (Mx.POSITIVE_IOU, Mx.IOU_MODES["bev"], 0.0), (Mx.POSITIVE_MAE, 0, 0.0))
    assert spec.anchors == R.ANCHORS


def test_strings_equal_default_objects_in_any_case():
    objects = [Mx.AnchorPrecision(), Mx.AnchorRecall(), Mx.AnchorAccuracy(), Mx.PositiveMeanAbsoluteError(), Mx.PositiveIoU()]
    assert [o.name for o in objects] == FIVE
    by_name, names = K.compile_loss("voxelnet", metrics=FIVE)
    by_object, names_o = K.compile_loss(K.VoxelNetLoss(), metrics=objects)
    assert by_name == by_object and hash(by_name) == hash(by_object) and names == names_o
    assert K.compile_loss("voxelnet", metrics=[s.upper() for s in FIVE])[0] == by_name
    assert Mx.AnchorRecall(0.5).det_term() == (Mx.ANCHOR_RECALL, 0, 0.5)
    assert Mx.PositiveIoU("3d").det_term() == (Mx.POSITIVE_IOU, Mx.IOU_MODES["3d"], 0.0)


def test_dict_and_nested_forms():
    want = [CLS + "anchor_recall", CLS + "p30", REG + "positive_iou"]
    cls, reg = ["anchor_recall", Mx.AnchorPrecision(0.3, name="p30")], [Mx.PositiveIoU("3d")]
    flat, n0 = K.compile_loss("voxelnet", metrics=[reg[0]] + cls)
    nested, n1 = K.compile_loss("voxelnet", metrics=[cls, reg])
    keyed, n2 = K.compile_loss("voxelnet", metrics={"RegressionLayer": reg[0], "ClassificationLayer": cls})
    assert n0 == n1 == n2 == want and flat == nested == keyed
    assert flat.metrics[1] == (Mx.ANCHOR_PRECISION, 0, 0.3) and flat.metrics[2][1] == Mx.IOU_MODES["3d"]
    only, n3 = K.compile_loss("voxelnet", metrics={"RegressionLayer": ["positive_mae"]})
    assert n3 == [REG + "positive_mae"] and only.n_metrics == 1
    # the same class twice under two names is two metrics
    two, n4 = K.compile_loss("voxelnet", metrics=[Mx.AnchorRecall(0.3, name="r30"), Mx.AnchorRecall(0.7, name="r70")])
    assert n4 == [CLS + "r30", CLS + "r70"] and two.n_metrics == 2
    eight = [Mx.AnchorRecall(0.1 * k, name=f"r{k}") for k in range(1, 9)]
    assert K.compile_loss("voxelnet", metrics=eight)[0].n_metrics == 8 == Mx.DET_MAX_METRICS


def test_the_metrics_are_part_of_the_plan_key_and_a_spec_without_them_is_the_old_one():
    plain = K.compile_loss("voxelnet", loss_weights=[2, .5])[0]
    old_way = K.DetectionLossSpec((1.5, 1.0, 0.0, 1.0, 1.0), (2.0, 0.5))
    assert plain == old_way and hash(plain) == hash(old_way) and plain.n_metrics == 0 and plain.metrics == ()
    assert hash(plain) == hash(("detection", (1.5, 1.0, 0.0, 1.0, 1.0), (2.0, 0.5)))
    assert plain == K.compile_loss("voxelnet", loss_weights=[2, .5], metrics=[])[0]
    assert plain.metrics_descriptor() is None
    a = K.compile_loss("voxelnet", loss_weights=[2, .5], metrics=["anchor_recall"])[0]
    b = K.compile_loss("voxelnet", loss_weights=[2, .5], metrics=[Mx.AnchorRecall(0.7)])[0]
    c = K.compile_loss("voxelnet", loss_weights=[2, .5], metrics=[Mx.AnchorRecall(name="another_name")])[0]
    assert len({plain, a, b}) == 3 and a != plain and a != b
    assert a == c and hash(a) == hash(c)                          # names are not part of the key
    assert K.compile_loss("voxelnet", metrics=["positive_iou"])[0] != K.compile_loss("voxelnet", metrics=[Mx.PositiveIoU("3d")])[0]


def test_descriptor():
    import ctypes
    from lisec_amd import _lib
    spec, _ = K.compile_loss(K.VoxelNetLoss(target_offset=0.25), metrics=[Mx.PositiveIoU("3d"), Mx.AnchorAccuracy(0.7)])
    d = spec.metrics_descriptor()
    assert d.struct_bytes == ctypes.sizeof(_lib.DetectionMetricsCfg) == 8 + 8 + 64 + 16 * _lib.DET_MAX_METRICS
    assert d.n_metrics == 2 and d.target_offset == 0.25
    assert [list(a) for a in d.anchors] == [list(a) for a in R.ANCHORS]
    assert (d.metric[0].kind, d.metric[0].mode, d.metric[0].threshold) == (Mx.ANCHOR_ACCURACY, 0, 0.7)
    assert (d.metric[1].kind, d.metric[1].mode) == (Mx.POSITIVE_IOU, 0)                   # LISEC_IOU_3D
    assert spec.descriptor().struct_bytes == ctypes.sizeof(_lib.DetectionLossCfg)         # the loss's own: untouched


# ---- compile(): refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metrics", [{"RegressionLayer": ["anchor_recall"]}, {"ClassificationLayer": "positive_iou"},
                                     [["positive_mae"], []], [[], [Mx.AnchorAccuracy()]]])
def test_a_metric_on_the_wrong_output_is_refused(metrics):
    with pytest.raises(ValueError, match="belongs to output"):
        K.compile_loss("voxelnet", metrics=metrics)


def test_duplicate_names_too_many_and_bad_shapes_are_refused():
    with pytest.raises(ValueError, match="appears twice"):
        K.compile_loss("voxelnet", metrics=["anchor_recall", Mx.AnchorRecall(0.3)])
    with pytest.raises(ValueError, match="appears twice"):
        K.compile_loss("voxelnet", metrics=[[], ["positive_iou", Mx.PositiveIoU("3d")]])
    nine = [Mx.AnchorRecall(0.1 * k, name=f"r{k}") for k in range(1, 9)] + ["positive_mae"]
    with pytest.raises(ValueError, match="at most 8"):
        K.compile_loss("voxelnet", metrics=nine)
    with pytest.raises(ValueError, match="one list per model output"):
        K.compile_loss("voxelnet", metrics=[["anchor_recall"], "positive_mae"])
    with pytest.raises(ValueError):
        K.compile_loss("voxelnet", metrics={"NoSuchLayer": ["anchor_recall"]})
    with pytest.raises(ValueError, match="Unknown metric"):
        K.compile_loss("voxelnet", metrics=["anchor_f1"])
    with pytest.raises(NotImplementedError):
        K.compile_loss("voxelnet", weighted_metrics=["anchor_recall"])


@pytest.mark.parametrize("cls", [Mx.AnchorPrecision, Mx.AnchorRecall, Mx.AnchorAccuracy])
@pytest.mark.parametrize("threshold", [0.0, 1.0, -0.1, 1.5, NAN])
def test_thresholds_outside_the_open_interval_are_refused(cls, threshold):
    with pytest.raises(ValueError, match="threshold"):
        cls(threshold)
    with pytest.raises(ValueError, match="threshold"):
        cls(threshold=threshold)


def test_unknown_iou_mode_is_refused():
    with pytest.raises(ValueError, match="mode"):
        Mx.PositiveIoU("2d")


@pytest.mark.parametrize("loss", ["mse", ["binary_crossentropy", "huber"], "smoothl1_ce"])
@pytest.mark.parametrize("metric", FIVE + [Mx.AnchorRecall(0.3), Mx.PositiveIoU()])
def test_a_detection_metric_with_another_loss_is_refused(loss, metric):
    with pytest.raises(NotImplementedError, match="loss='voxelnet'"):
        K.compile_loss(loss, metrics=[metric])


@pytest.mark.parametrize("metrics", [["mae"], ["accuracy"], [Mx.BinaryAccuracy()], ["anchor_recall", "mse"],
                                     {"ClassificationLayer": ["anchor_recall", "binary_accuracy"]}, [["precision"], []],
                                     [Mx.MeanAbsoluteError()], ["recall"], ["mean_iou"]])
def test_keras_metrics_with_the_detection_loss_stay_refused(metrics):
    with pytest.raises(NotImplementedError, match="metrics"):
        K.compile_loss("voxelnet", metrics=metrics)
    with pytest.raises(NotImplementedError, match="metrics"):
        K.compile_loss(K.VoxelNetLoss(gamma=2.0), metrics=metrics)


def test_a_subclass_of_ones_own_is_refused():
    class Mine(Mx.AnchorRecall):
        pass
    with pytest.raises(NotImplementedError):
        K.compile_loss("voxelnet", metrics=[Mine()])


# ---- serialization -----------------------------------------------------------------------------------------------------
def test_serialize_deserialize_round_trip():
    objects = [Mx.AnchorPrecision(0.3), Mx.AnchorRecall(0.7, name="r70"), Mx.AnchorAccuracy(), Mx.PositiveMeanAbsoluteError(),
               Mx.PositiveIoU("3d", name="iou3d")]
    for o in objects:
        cfg = Mx.serialize(o)
        assert cfg["class_name"] == type(o).__name__ and cfg["config"]["name"] == o.name
        back = Mx.deserialize(cfg)
        assert type(back) is type(o) and back.get_config() == o.get_config() and back.det_term() == o.det_term()
        assert type(o).from_config(o.get_config()).get_config() == o.get_config()
        assert isinstance(Mx.get(cfg), type(o))
    assert Mx.serialize(objects[0])["config"]["threshold"] == 0.3 and Mx.serialize(objects[4])["config"]["mode"] == "3d"
    assert Mx.serialize("anchor_recall") == "anchor_recall" == Mx.deserialize("anchor_recall")
    # what save() writes and load_model compiles again: the same spec and names
    from lisec_amd.keras_h5 import _serialize_nested
    from lisec_amd.model_training import _deserialize_nested
    given = {"ClassificationLayer": [objects[0], "anchor_recall"], "RegressionLayer": objects[4]}
    again = _deserialize_nested(_serialize_nested(given), Mx.deserialize)
    assert K.compile_loss("voxelnet", metrics=again) == K.compile_loss("voxelnet", metrics=given)


def test_accumulator_layout_keeps_the_sweep_count_where_the_loss_kernel_writes_it():
    from lisec_amd.network import loss_acc_len, loss_acc_logs, loss_acc_split
    plain = K.compile_loss("voxelnet")[0]
    spec = K.compile_loss("voxelnet", metrics=["anchor_recall", "positive_mae"])[0]
    assert loss_acc_len(plain) == 4 and loss_acc_len(spec) == 8 and loss_acc_len("mse") == 4
    #            total class reg sweeps | recall num den | mae num den
    acc = np.array([6.0, 3.0, 9.0, 3.0, 5.0, 20.0, 0.0, 0.0])
    sums, count = loss_acc_split(spec, acc)
    assert count == 3.0 and loss_acc_logs(spec, sums, count) == [2.0, 1.0, 3.0, 0.25, 0.0]
    sums, count = loss_acc_split(plain, acc[:4])
    assert count == 3.0 and loss_acc_logs(plain, sums, count) == [2.0, 1.0, 3.0]
    # a Keras-metric accumulator keeps its layout: [total, class, regression, metrics..., sweeps], every word a mean
    keras = K.compile_loss("mse", metrics=["mae"])[0]
    sums, count = loss_acc_split(keras, np.array([6.0, 3.0, 9.0, 1.0, 2.0, 2.0]))
    assert loss_acc_len(keras) == 6 and count == 2.0 and loss_acc_logs(keras, sums, count) == [3.0, 1.5, 4.5, 0.5, 1.0]
    # no sweeps: the losses are NaN as before, a pooled ratio is 0.0
    logs = loss_acc_logs(spec, np.zeros(7), 0.0)
    assert np.isnan(logs[:3]).all() and logs[3:] == [0.0, 0.0]
