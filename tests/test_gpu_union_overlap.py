"""lisec_boxes_union_overlap / boxes.union_overlap / rpnToRegion.calcIoUAll / Predict.scoreMain against the test-local
oracle (tests/union_overlap_ref.py).  Areas are held to rtol 1e-10 of the scene's summed box areas + atol 1e-12: the
bound tests/test_gpu_boxes.py holds the device polygon area to, scaled by the magnitude the boundary sums cancel over."""
import math
import os

import numpy as np
import pytest

import union_overlap_ref as R

pytestmark = pytest.mark.gpu


def _box(x, y, l, w, yaw=0.0, z=1.0, h=1.5):
    """x, y, z, l, w, h, yaw; at yaw 0 the WIDTH lies along x and the length along y (serialize_data.py:151-163)."""
    return [x, y, z, l, w, h, yaw]


def _rows(b):
    return np.asarray(b, dtype=np.float64).reshape(-1, 7)


def _tol(P, L):
    P, L = _rows(P), _rows(L)
    return 1e-10 * float(np.abs(P[:, 3] * P[:, 4]).sum() + np.abs(L[:, 3] * L[:, 4]).sum()) + 1e-12


def _check(P, L, slots=(0, 1, 2)):
    """One sample through the GPU and the oracle; returns the GPU row."""
    from lisec_amd import boxes
    got = boxes.union_overlap([_rows(P)], [_rows(L)])
    assert got.shape == (1, 5) and got.dtype == np.float64
    want, tol = R.union_overlap(P, L), _tol(P, L)
    for k in slots:
        print(f"slot {k}: gpu {got[0, k]!r} oracle {want[k]!r} diff {abs(got[0, k] - want[k]):.3e} bound {tol:.3e}")
    for k in slots:
        assert abs(got[0, k] - want[k]) <= tol, (k, got[0, k], want[k])
    assert got[0, 3] == pytest.approx(want[3], rel=1e-13) and got[0, 4] == pytest.approx(want[4], rel=1e-13)
    return got[0]


@pytest.fixture(scope="module")
def lyft_scene():
    """20 predictions x 40 labels in 10 well-separated clusters, the oracle's answer, and the GPU's (computed once)."""
    from lisec_amd import boxes
    P, L = R.clustered_scene(np.random.default_rng(8), 20, 40, 10)
    return P, L, R.union_overlap(P, L), boxes.union_overlap([P], [L])[0]


def test_one_pair_in_general_position_matches_the_pairwise_area():
    import torch
    from lisec_amd import _lib
    P, L = _box(0.3, -0.2, 4.5, 1.9, 0.4), _box(1.0, 0.5, 4.1, 2.0, -0.7)
    got = _check([P], [L])
    lib, dev = _lib.load(), torch.device("cuda")
    bx = torch.from_numpy(_rows([P, L])).to(dev)
    corners = torch.zeros((2, 4, 2), dtype=torch.float64, device=dev)
    pair = torch.zeros((1, 4), dtype=torch.float64, device=dev)
    _lib.check(lib.lisec_box_geometry(_lib.ptr(bx), 2, None, _lib.ptr(corners), _lib.ptr(pair), _lib.current_stream()))
    pairwise = float(pair.cpu()[0, 3])
    assert pairwise > 1.0 and abs(got[0] - pairwise) <= _tol([P], [L])
    assert got[1] == pytest.approx(4.5 * 1.9, rel=1e-12) and got[2] == pytest.approx(4.1 * 2.0, rel=1e-12)


def test_containment_without_crossings():
    small, big = _box(0.2, 0.1, 1.0, 0.8, 0.3), _box(0, 0, 6, 5, -0.2)
    assert _check([small], [big])[0] == pytest.approx(0.8, rel=1e-12)
    assert _check([big], [small])[0] == pytest.approx(0.8, rel=1e-12)


def test_overlapping_predictions_are_not_counted_twice():
    P = [_box(-0.5, 0, 2.0, 3.0, 0.2), _box(0.5, 0.2, 2.0, 3.0, -0.3)]
    L = [_box(0, 0, 8, 8, 0.1)]
    got = _check(P, L)
    pairwise = sum(R.area(R.clip(R.footprint(p), R.footprint(L[0]))) for p in P)
    assert pairwise == pytest.approx(12.0, rel=1e-12) and got[0] < pairwise - 1.0
    assert got[0] == pytest.approx(got[1], rel=1e-12)          # everything lies under L


_sq = _box(0, 0, 2, 2)
DEGENERATE = {
    # name: (P, L, slot 0 by hand or None)
    "duplicate_prediction": ([_box(0.5, 0, 2, 2, 0.3)] * 2, [_sq], None),
    "abutting_predictions_under_one_label": ([_box(-1, 0, 2, 2), _box(1, 0, 2, 2)], [_box(0, 0, 3, 5)], 4 * 2 + 0.0),
    "collinear_edges_same_orientation": ([_box(0, 0, 2, 3), _box(1, 0, 2, 3)], [_box(0.5, 0, 4, 6)], 4.0 * 2),
    "label_vertex_on_prediction_edge": ([_sq], [_box(1 + math.sqrt(0.5), 0, 1, 1, math.pi / 4),
                                               _box(0, 1, 1, 1)], 0.5),
    "corner_touch": ([_sq], [_box(2, 2, 2, 2)], 0.0),
    "edge_touch": ([_sq], [_box(2, 0.5, 2, 2)], 0.0),
    "quarter_turns_equal_coordinates": ([_box(0, 0, 2, 4, 0.0), _box(0, 0, 4, 2, math.pi / 2)],
                                        [_box(0, 0, 2, 4, math.pi), _box(1, 0, 2, 4, math.pi / 2)], None),
    "zero_width_box": ([_box(0, 0, 2, 0), _box(0.5, 0.5, 0, 3), _sq], [_box(1, 1, 2, 2)], 1.0),
    "negative_length": ([_box(0, 0, -2, 2, 0.3)], [_box(0.5, 0, 2, -2, 0.3), _box(0.2, 0.1, -1, -1, 1.0)], None),
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_configurations(name):
    P, L, by_hand = DEGENERATE[name]
    got = _check(P, L)
    if by_hand is not None:
        assert abs(got[0] - by_hand) <= _tol(P, L)
    got = _check(L, P)                                         # the same with the sides swapped
    if by_hand is not None:
        assert abs(got[0] - by_hand) <= _tol(P, L)


def test_empty_sides():
    from lisec_amd import boxes
    some = _rows([_box(0, 0, 2, 3, 0.2), _box(0.5, 0, 2, 3, -0.2)])
    none = np.zeros((0, 7))
    vol = float((some[:, 3] * some[:, 4] * some[:, 5]).sum())
    got = boxes.union_overlap([none, some, none], [some, none, none])
    union = R.union_overlap(some, none)[1]
    assert np.allclose(got[0], [0, 0, union, 0, vol], rtol=1e-13, atol=0) and got[0, 0] == 0.0 and got[0, 1] == 0.0
    assert np.allclose(got[1], [0, union, 0, vol, 0], rtol=1e-13, atol=0) and got[1, 0] == 0.0 and got[1, 2] == 0.0
    assert np.array_equal(got[2], np.zeros(5))
    assert boxes.calcIoUAll_boxes(none, some) == 0.0 and boxes.calcIoUAll_boxes(some, none) == 0.0
    with pytest.raises(ZeroDivisionError):
        boxes.calcIoUAll_boxes(none, none)
    assert boxes.bev_iou(none, none) == 0.0 and boxes.bev_iou(some, none) == 0.0
    assert boxes.bev_iou(some, some) == pytest.approx(1.0, rel=1e-12)


def test_permutation_invariance_and_determinism():
    from lisec_amd import boxes
    rng = np.random.default_rng(4)
    P, L = R.clustered_scene(rng, 6, 6, 1, spread=1.5)
    L = L[:4]                                                  # 6 x 4 = 24 candidate pieces, of which <= 12 may be non-empty
    P = np.concatenate([P, P[:2] + [9.0, 0, 0, 0, 0, 0, 0]])[2:]
    L = np.concatenate([L, L[:2] + [9.0, 0.3, 0, 0, 0, 0, 0.1]])
    base = boxes.union_overlap([P], [L])
    again = boxes.union_overlap([P], [L])
    assert np.array_equal(base, again)                         # bit for bit
    assert base[0, 0] > 1.0
    for _ in range(4):
        got = boxes.union_overlap([P[rng.permutation(len(P))]], [L[rng.permutation(len(L))]])
        assert np.allclose(got[0, :3], base[0, :3], rtol=1e-12, atol=0)


def test_batched_launch_equals_single_launches():
    """Segment indexing: seven samples with uneven counts in one launch == seven launches, bit for bit; and one sample
    of 64 + 64 boxes (32 clusters of 2 + 2), more edges than one pass of the workgroup, against the oracle."""
    from lisec_amd import boxes
    rng = np.random.default_rng(5)
    counts = [(0, 0), (1, 1), (3, 3), (20, 20), (0, 5), (20, 40), (2, 2)]
    scenes = [R.clustered_scene(rng, p, l, 10) for p, l in counts]
    whole = boxes.union_overlap([s[0] for s in scenes], [s[1] for s in scenes])
    for i, (P, L) in enumerate(scenes):
        assert np.array_equal(boxes.union_overlap([P], [L])[0], whole[i]), i
    assert (whole[[1, 2, 3, 5, 6], 1] > 0).all() and whole[0, 1] == 0.0
    P, L = R.clustered_scene(rng, 64, 64, 32)
    _check(P, L)
    P, L = R.clustered_scene(rng, 72, 72, 36)                  # 144 rectangles: beyond the kernel's LDS cache of 128
    _check(P, L)


def test_lyft_sized_scene(lyft_scene):
    P, L, want, got = lyft_scene
    tol = _tol(P, L)
    print("gpu", got.tolist(), "oracle", want.tolist(), "bound", tol)
    assert want[0] > 10.0
    assert np.all(np.abs(got[:3] - want[:3]) <= tol)
    assert np.allclose(got[3:], want[3:], rtol=1e-13, atol=0)


def test_reference_quirk_area_over_volumes(lyft_scene):
    from lisec_amd import boxes
    P, L, _, got = lyft_scene
    inter = boxes.calcIntersectAll(P, L)
    assert inter == got[0]
    vols = float((P[:, 3] * P[:, 4] * P[:, 5]).sum() + (L[:, 3] * L[:, 4] * L[:, 5]).sum())
    union = boxes.calcUnionAll(P, L, inter)
    assert union == pytest.approx(vols - inter, rel=1e-15)
    assert boxes.calcIoUAll_boxes(P, L) == pytest.approx(inter / union, rel=1e-15)
    assert boxes.bev_iou(P, L) == pytest.approx(got[0] / (got[1] + got[2] - got[0]), rel=1e-15)


class _FakeLyft:
    """Duck-typed LyftDataset: the tables calcIoUAll reads (rpnToRegion.py:224-251)."""

    def __init__(self, anns, ego_t, ego_q):
        self.t = {"sample_data": {"sd": {"ego_pose_token": "ego"}}, "ego_pose": {"ego": {"translation": ego_t, "rotation": ego_q}},
                  "sample_annotation": {f"a{i}": a for i, a in enumerate(anns)},
                  "instance": {f"i{i}": {"category_token": a["_cat"]} for i, a in enumerate(anns)},
                  "category": {"car": {"name": "car"}, "bus": {"name": "bus"}}}

    def get(self, table, token):
        return self.t[table][token]


@pytest.mark.parametrize("ego_yaw", [0.0, 0.3])
def test_calc_iou_all_and_annotation_boxes(ego_yaw):
    from lisec_amd import boxes, rpnToRegion
    from lisec_amd.model_training import rotate_points
    ego_t = [100.0, -40.0, 2.0] if ego_yaw else [0.0, 0.0, 0.0]
    ego_q = [math.cos(ego_yaw / 2), 0.0, 0.0, math.sin(ego_yaw / 2)]
    local = _rows([[3.0, 4.0, 1.0, 4.5, 1.9, 1.6, 0.2], [-20.0, 10.0, 0.9, 4.2, 2.0, 1.5, -1.1], [5.0, 5.0, 1.0, 10.0, 3.0, 3.0, 0.0],
                   [50.0, -10.0, 1.1, 4.4, 1.8, 1.5, 0.5], [50.01, 10.0, 1.0, 4.4, 1.8, 1.5, 0.5]])
    cats = ["car", "car", "bus", "car", "car"]
    if ego_yaw:                                                # a rotated pose does not land on 50 exactly: 49.99 instead
        local[3, 0] = 49.99
    anns = []
    for i, b in enumerate(local):
        g = rotate_points(b[None, :3], np.array(ego_q), False)[0] + np.array(ego_t)           # ego -> global
        anns.append({"translation": list(g), "size": list(b[3:6]), "rotation": [math.cos(b[6] / 2), 0, 0, math.sin(b[6] / 2)],
                     "instance_token": f"i{i}", "_cat": cats[i]})
    ds = _FakeLyft(anns, ego_t, ego_q)
    sample = {"anns": [f"a{i}" for i in range(len(local))], "data": {"LIDAR_TOP": "sd"}}
    rows = boxes.annotationBoxes(sample, ds)
    assert rows.shape == (3, 7) and np.allclose(rows, local[[0, 1, 3]], rtol=0, atol=1e-9)    # bus and x = 50.01 dropped
    if not ego_yaw:
        assert rows[2, 0] == 50.0                              # the window is closed
    pred = _rows([[3.4, 4.2, 1.0, 4.4, 1.8, 1.5, 0.3], [-19.0, 10.5, 1.0, 4.0, 1.9, 1.5, -1.0], [30.0, 30.0, 1.0, 4.0, 1.9, 1.5, 0.0]])
    want = R.union_overlap(pred, rows)
    ref_iou = want[0] / (want[3] + want[4] - want[0])
    assert want[0] > 5.0
    got = rpnToRegion.calcIoUAll(pred, sample, ds)
    assert abs(got - ref_iou) <= _tol(pred, rows) / (want[3] + want[4] - want[0]) * 2
    rpnToRegion.level5Data = ds                                # the reference's module-global form
    try:
        assert rpnToRegion.calcIoUAll(pred, sample) == got
    finally:
        rpnToRegion.level5Data = None
    with pytest.raises(RuntimeError):
        rpnToRegion.calcIoUAll(pred, sample)
    assert rpnToRegion.calcIntersectAll(pred, rows) == pytest.approx(want[0], abs=_tol(pred, rows))
    assert rpnToRegion.calcUnionAll(pred, rows, 1.5) == pytest.approx(want[3] + want[4] - 1.5, rel=1e-15)


def test_rpn_to_region_as_device():
    import torch
    from lisec_amd import boxes
    rng = np.random.default_rng(3)
    cls = rng.uniform(0, 1, (100, 200, 2)).astype(np.float32)
    reg = rng.normal(0, 0.1, (100, 200, 14)).astype(np.float32)
    b, p = boxes.rpnToRegion(cls, reg)
    db, dp, dk = boxes.rpnToRegion(cls, reg, as_device=True)
    assert db.is_cuda and dp.is_cuda and dk.is_cuda and dk.dtype == torch.int32
    k = int(dk.item())
    assert k == len(p) and np.array_equal(db[:k].cpu().numpy(), b) and np.array_equal(dp[:k].cpu().numpy(), p)


class _Level5(_FakeLyft):
    """Lidar files (model_training.combine_lidar_data) and annotation tables in one duck-typed dataset."""

    def __init__(self, root, rng, n_samples):
        anns = [{"translation": [float(rng.uniform(-40, 40)), float(rng.uniform(-40, 40)), 1.0], "size": [4.5, 1.9, 1.6],
                 "rotation": [math.cos(a / 2), 0, 0, math.sin(a / 2)], "instance_token": f"i{i}", "_cat": "car"}
                for i, a in enumerate(rng.uniform(-3, 3, 30))]
        super().__init__(anns, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0])
        self.t["calibrated_sensor"] = {"cs": {"rotation": [1.0, 0, 0, 0], "translation": [0.0, 0.0, 1.0]}}
        self.samples = []
        for i in range(n_samples):
            raw = np.zeros((4000, 5), np.float32)
            raw[:, :2] = rng.uniform(-45, 45, (4000, 2))
            raw[:, 2] = rng.uniform(-1.0, 1.2, 4000)
            raw.tofile(os.path.join(root, f"s{i}.bin"))
            self.t["sample_data"][f"sd{i}"] = {"filename": f"s{i}.bin", "calibrated_sensor_token": "cs", "ego_pose_token": "ego"}
            self.samples.append({"data": {"LIDAR_TOP": f"sd{i}"}, "anns": [f"a{j}" for j in range(30)]})


def test_score_main_equals_the_host_chain(tmp_path):
    from lisec_amd import Constants, Predict, boxes, model_training
    rng = np.random.default_rng(2)
    l5 = _Level5(str(tmp_path), rng, 2)
    np.random.seed(0)
    model = model_training.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    scores = Predict.scoreMain(l5.samples, l5, model, dataDir=str(tmp_path))
    assert len(scores) == 2
    for sample, (ref_iou, bev) in zip(l5.samples, scores):
        pts = model_training.combine_lidar_data(sample, str(tmp_path), l5)
        vfe = model_training.VFE_preprocessing(pts, Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints,
                                               Constants.nx // 2, Constants.ny // 2, Constants.nz)
        prob, regress = model.predict(vfe)
        found, _ = boxes.rpnToRegion(prob[0], regress[0])
        found[:, 0] -= 50
        found[:, 1] -= 50
        labels = boxes.annotationBoxes(sample, l5)
        assert len(found) == 21 and len(labels) >= 20
        assert ref_iou == pytest.approx(boxes.calcIoUAll_boxes(found, labels), rel=1e-12, abs=1e-15)
        assert bev == pytest.approx(boxes.bev_iou(found, labels), rel=1e-12, abs=1e-15)
        assert 0.0 <= bev <= 1.0


def test_invalid_arguments():
    import torch
    from lisec_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda")
    bx = torch.zeros((1, 7), dtype=torch.float64, device=dev)
    start = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    out = torch.zeros(5, dtype=torch.float64, device=dev)
    st = _lib.current_stream()
    EINVAL = -1
    args = [_lib.ptr(bx), _lib.ptr(start), _lib.ptr(bx), _lib.ptr(start), 1, None, 0, _lib.ptr(out), st]
    assert lib.lisec_boxes_union_overlap(*args) == 0
    for slot in (0, 1, 2, 3, 7):                               # NULL boxes, offsets, out
        bad = list(args)
        bad[slot] = None
        assert lib.lisec_boxes_union_overlap(*bad) == EINVAL and lib.lisec_last_error()
    bad = list(args)
    bad[4] = -1
    assert lib.lisec_boxes_union_overlap(*bad) == EINVAL
    need = lib.lisec_boxes_union_overlap_workspace_bytes(1, 1, 1)
    if need:                                                   # a short workspace, once an algorithm needs one
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        bad = list(args)
        bad[5], bad[6] = _lib.ptr(ws), need - 1
        assert lib.lisec_boxes_union_overlap(*bad) == EINVAL
    assert lib.lisec_boxes_union_overlap(*(args[:4] + [0] + args[5:])) == 0          # no samples: nothing to do
    torch.cuda.synchronize()
