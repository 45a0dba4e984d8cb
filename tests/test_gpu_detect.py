"""lisec_detect / boxes.detect / Predict.detectMain / Predict.detectionAP(detector=...) against the test-local oracle
(tests/detect_ref.py) on the cases of tests/detect_cases.py.

The kept flat indices and both counts equal the oracle's exactly: every quantity that decides them is an integer or sits at
least 1e-9 from its threshold (tests/test_detect_oracle.py holds every case to that on the CPU, where the seeds were chosen).
out_boxes[k] is row out_index[k] of lisec_rpn_decode at rtol 1e-15 (the same expression; the tolerance only allows for a
different fused-multiply-add contraction), raw scores are exact, sigmoid scores agree to rtol 1e-14 (exp and one division in
float64 on both sides).  Each case goes through boxes.detect and once through the C entry with its own buffers."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import detect_cases as C

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -1, -2


@functools.lru_cache(maxsize=None)
def _device_maps(name):
    import torch
    c = C.case(name)
    return torch.from_numpy(c["cls"].copy()).cuda(), torch.from_numpy(c["reg"].copy()).cuda()


@functools.lru_cache(maxsize=None)
def _decoded(name):
    """Every candidate of the case as lisec_rpn_decode writes it: (2 M, 7) float64 on the host."""
    import torch
    from lisec_amd import _lib, boxes
    cls, reg = _device_maps(name)
    cfg, n = boxes._cfg(), 2 * C.M
    dec = torch.empty((n, 7), dtype=torch.float64, device="cuda")
    prob = torch.empty(n, dtype=torch.float64, device="cuda")
    legal = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().lisec_rpn_decode(ctypes.byref(cfg), _lib.ptr(cls), 2, _lib.ptr(reg), 14, _lib.ptr(dec), _lib.ptr(prob),
                                            _lib.ptr(legal), _lib.current_stream()))
    return dec.cpu().numpy()


def _check(name, got_boxes, got_scores, got_index, got_count):
    """Four host arrays against the oracle's result and the device's own decode."""
    c = C.case(name)
    ref = c["ref"]
    k = ref["count"][0]
    print(f"{name}: kept {got_count[0]} (oracle {k}), passing {got_count[1]} (oracle {ref['count'][1]})")
    assert tuple(int(v) for v in got_count) == ref["count"]
    assert got_index[:k].tolist() == ref["index"].tolist()
    assert np.allclose(got_boxes[:k], _decoded(name)[ref["index"]], rtol=1e-15, atol=0.0)
    assert np.allclose(got_boxes[:k], ref["boxes"], rtol=1e-12, atol=1e-12)            # and the oracle's own decode (numpy's exp)
    if C.oracle_arguments(c["kw"])["sigmoid_scores"]:
        assert np.allclose(got_scores[:k], ref["scores"], rtol=1e-14, atol=0.0)
    else:
        assert np.array_equal(got_scores[:k], ref["raw"].astype(np.float64))
    assert np.all(np.diff(got_scores[:k]) <= 0)


def _raw_call(name, sentinel=7.0, **override):
    """lisec_detect itself on the case, into buffers one row longer than max_boxes and filled with a sentinel."""
    import torch
    from lisec_amd import _lib, boxes, ops
    lib = _lib.load()
    cls, reg = _device_maps(name)
    o = dict(C.oracle_arguments(C.case(name)["kw"]), **override)
    det = ops.detect_params(o["score_threshold"], o["sigmoid_scores"], o["pre_nms_top_n"], o["max_boxes"], o["iou_threshold"],
                            o.get("iou_mode_code", {"3d": 0, "bev": 1}[o["iou_mode"]]), o["inside_only"])
    cfg = boxes._cfg()
    need = lib.lisec_detect_workspace_bytes(ctypes.byref(cfg), ctypes.byref(det))
    rows = max(o["max_boxes"], 1) + 1
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    out = (torch.full((rows, 7), sentinel, dtype=torch.float64, device="cuda"),
           torch.full((rows,), sentinel, dtype=torch.float64, device="cuda"),
           torch.full((rows,), -7, dtype=torch.int32, device="cuda"), torch.full((3,), -7, dtype=torch.int32, device="cuda"))
    rc = lib.lisec_detect(ctypes.byref(cfg), ctypes.byref(det), _lib.ptr(cls), 2, _lib.ptr(reg), 14, _lib.ptr(ws),
                          override.get("workspace_bytes", need), *[_lib.ptr(t) for t in out], _lib.current_stream())
    return rc, need, [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_case_through_the_python_surface_and_the_c_entry(name):
    import torch
    from lisec_amd import boxes
    c = C.case(name)
    cls, reg = _device_maps(name)
    k = c["ref"]["count"][0]
    d_boxes, d_scores, d_index, d_count = boxes.detect(cls, reg, as_device=True, **c["kw"])
    cap = C.oracle_arguments(c["kw"])["max_boxes"]
    assert d_boxes.shape == (cap, 7) and d_scores.shape == (cap,) and d_index.shape == (cap,) and d_count.shape == (2,)
    assert d_boxes.dtype == d_scores.dtype == torch.float64 and d_index.dtype == d_count.dtype == torch.int32
    got = [t.cpu().numpy() for t in (d_boxes, d_scores, d_index, d_count)]
    _check(name, *got)
    assert not got[0][k:].any() and not got[1][k:].any() and not got[2][k:].any()         # zero past the kept rows
    h_boxes, h_scores = boxes.detect(c["cls"].copy(), c["reg"].copy(), **c["kw"])      # numpy in, numpy out
    assert h_boxes.shape == (k, 7) and h_scores.shape == (k,) and h_boxes.dtype == h_scores.dtype == np.float64
    assert np.array_equal(h_boxes, got[0][:k]) and np.array_equal(h_scores, got[1][:k])
    rc, _, raw = _raw_call(name)
    assert rc == 0
    _check(name, raw[0], raw[1], raw[2], raw[3][:2])
    for a, b in zip(raw[:3], got[:3]):
        assert np.array_equal(a[:k], b[:k])                                            # bit for bit what the surface returned
    assert np.all(raw[0][k:] == 7.0) and np.all(raw[1][k:] == 7.0) and np.all(raw[2][k:] == -7) and raw[3][2] == -7


def test_nothing_passes_leaves_the_outputs_alone():
    rc, _, raw = _raw_call("nothing_passes")
    assert rc == 0 and raw[3].tolist() == [0, 0, -7]
    assert np.all(raw[0] == 7.0) and np.all(raw[1] == 7.0) and np.all(raw[2] == -7)


def test_output_cap_reports_the_passing_total():
    from lisec_amd import boxes
    c = C.case("cap")
    cls, reg = _device_maps("cap")
    _, _, index, count = boxes.detect(cls, reg, as_device=True, **c["kw"])
    _, _, more, count_more = boxes.detect(cls, reg, as_device=True, **dict(c["kw"], max_boxes=600))
    assert count.tolist() == [50, 600] and count_more[1].item() == 600 and count_more[0].item() > 100
    assert more[:50].tolist() == index.tolist()


def test_as_device_returns_at_once_and_calls_do_not_disturb_each_other():
    import torch
    from lisec_amd import boxes
    names = ("clustered_scene", "top65", "filters_logits")
    maps = [_device_maps(n) for n in names]
    for n in names:
        _decoded(n)
    busy = torch.ones(2 ** 28, device="cuda")
    torch.cuda.synchronize()
    for _ in range(60):
        busy.mul_(1.0001)                                      # tens of milliseconds of queued work ahead of the calls
    outs = [boxes.detect(cls, reg, as_device=True, **C.case(n)["kw"]) for n, (cls, reg) in zip(names, maps)]
    again = boxes.detect(*maps[0], as_device=True, **C.case(names[0])["kw"])
    done = torch.cuda.Event()
    done.record()
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "boxes.detect(as_device=True) waited for the GPU"
    for n, out in zip(names, outs):
        _check(n, *[t.cpu().numpy() for t in out])
    for a, b in zip(outs[0], again):
        assert torch.equal(a, b)                                # run to run: bit-identical


# ---- Predict ---------------------------------------------------------------------------------------------------------------
class _Level5:
    """Duck-typed LyftDataset: lidar files (model_training.combine_lidar_data) and the tables annotationBoxes reads."""

    def __init__(self, root, rng, n_samples):
        anns = [{"translation": [float(rng.uniform(-40, 40)), float(rng.uniform(-40, 40)), 1.0], "size": [4.5, 1.9, 1.6],
                 "rotation": [math.cos(a / 2), 0, 0, math.sin(a / 2)], "instance_token": f"i{i}"}
                for i, a in enumerate(rng.uniform(-3, 3, 20))]
        self.t = {"sample_data": {}, "ego_pose": {"ego": {"translation": [0.0, 0.0, 0.0], "rotation": [1.0, 0.0, 0.0, 0.0]}},
                  "sample_annotation": {f"a{i}": a for i, a in enumerate(anns)},
                  "instance": {f"i{i}": {"category_token": "car"} for i in range(len(anns))},
                  "category": {"car": {"name": "car"}},
                  "calibrated_sensor": {"cs": {"rotation": [1.0, 0, 0, 0], "translation": [0.0, 0.0, 1.0]}}}
        self.samples = []
        for i in range(n_samples):
            raw = np.zeros((4000, 5), np.float32)
            raw[:, :2] = rng.uniform(-45, 45, (4000, 2))
            raw[:, 2] = rng.uniform(-1.0, 1.2, 4000)
            raw.tofile(os.path.join(root, f"s{i}.bin"))
            self.t["sample_data"][f"sd{i}"] = {"filename": f"s{i}.bin", "calibrated_sensor_token": "cs", "ego_pose_token": "ego"}
            self.samples.append({"data": {"LIDAR_TOP": f"sd{i}"}, "anns": [f"a{j}" for j in range(len(anns))]})

    def get(self, table, token):
        return self.t[table][token]


def test_detect_main_and_detection_ap_equal_the_calls_by_hand(tmp_path):
    from lisec_amd import Constants, Predict, boxes, model_training
    rng = np.random.default_rng(3)
    l5 = _Level5(str(tmp_path), rng, 2)
    np.random.seed(0)
    model = model_training.createModel(Constants.nx, Constants.ny, Constants.nz, Constants.maxPoints)
    detector = dict(pre_nms_top_n=500, max_boxes=60, iou_threshold=0.2, iou_mode="3d")
    got = Predict.detectMain(l5.samples, l5, model, dataDir=str(tmp_path), **detector)
    ap = Predict.detectionAP(l5.samples, l5, model, dataDir=str(tmp_path), detector=detector)
    ap_reference_path = Predict.detectionAP(l5.samples, l5, model, dataDir=str(tmp_path), detector=None)
    ap_as_before = Predict.detectionAP(l5.samples, l5, model, dataDir=str(tmp_path))
    found, scores, old_found, old_probs, labels = [], [], [], [], []
    for sample in l5.samples:
        pts = model_training.combine_lidar_data(sample, str(tmp_path), l5)
        vfe = model_training.VFE_preprocessing(pts, Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints,
                                               Constants.nx // 2, Constants.ny // 2, Constants.nz)
        prob, regress = model.predict(vfe)
        b, s = boxes.detect(prob[0], regress[0], **detector)
        b[:, 0] -= 50
        b[:, 1] -= 50
        found.append(b); scores.append(s)
        b, p = boxes.rpnToRegion(prob[0], regress[0])
        b[:, 0] -= 50
        b[:, 1] -= 50
        old_found.append(b); old_probs.append(p); labels.append(boxes.annotationBoxes(sample, l5))
    assert len(got) == 2 and all(0 < len(b) <= 60 for b, _ in got)
    for (b, s), hb, hs in zip(got, found, scores):
        assert b.dtype == s.dtype == np.float64 and np.array_equal(b, hb) and np.array_equal(s, hs)
    by_hand = boxes.average_precision(found, scores, labels)
    old_by_hand = boxes.average_precision(old_found, old_probs, labels)
    for name in ("ap", "tp", "tp_count", "best_iou", "best_label", "thresholds"):
        assert np.array_equal(getattr(ap, name), getattr(by_hand, name)), name
        assert np.array_equal(getattr(ap_reference_path, name), getattr(old_by_hand, name)), name        # None: today's path,
        assert np.array_equal(getattr(ap_as_before, name), getattr(old_by_hand, name)), name             # bit for bit
    assert ap.n_predictions == sum(len(b) for b in found) and ap_reference_path.n_predictions == sum(len(b) for b in old_found)
    assert Predict.detectMain([], l5, model) == []
    with pytest.raises(ValueError):
        Predict.detectMain(l5.samples, l5, model, dataDir=str(tmp_path), as_device=True)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_the_c_entry_refuses_what_it_cannot_serve():
    from lisec_amd import _lib
    lib = _lib.load()
    rc, need, _ = _raw_call("top64")
    assert rc == 0 and need > 2 * C.M * 8
    for bad, word in ((dict(pre_nms_top_n=4097, max_boxes=10), b"pre_nms_top_n"), (dict(pre_nms_top_n=0, max_boxes=1), b"pre_nms_top_n"),
                      (dict(pre_nms_top_n=64, max_boxes=65), b"max_boxes"), (dict(max_boxes=0), b"max_boxes"),
                      (dict(iou_threshold=1.0), b"iou_threshold"), (dict(iou_threshold=-0.01), b"iou_threshold"),
                      (dict(iou_threshold=math.nan), b"iou_threshold"), (dict(score_threshold=math.nan), b"score_threshold"),
                      (dict(iou_mode_code=2), b"iou_mode")):
        rc, need_bad, raw = _raw_call("top64", **bad)
        assert rc == EINVAL and need_bad == 0 and word in lib.lisec_last_error(), bad
        assert raw[3].tolist() == [-7, -7, -7] and np.all(raw[0] == 7.0)               # nothing was enqueued
    rc, _, raw = _raw_call("top64", workspace_bytes=need - 1)
    assert rc == ENOSPC and b"workspace" in lib.lisec_last_error() and raw[3].tolist() == [-7, -7, -7]
    rc, _, _ = _raw_call("top64", score_threshold=-math.inf)                            # no threshold is a value, not an error
    assert rc == 0


def test_python_refusals():
    from lisec_amd import boxes
    c = {k: v.copy() for k, v in C.case("top64").items() if k in ("cls", "reg")}
    for bad in (dict(pre_nms_top_n=4097), dict(pre_nms_top_n=0), dict(pre_nms_top_n=10.5), dict(pre_nms_top_n=True),
                dict(pre_nms_top_n=64, max_boxes=65), dict(max_boxes=0), dict(max_boxes="3"), dict(iou_threshold=1.0),
                dict(iou_threshold=-0.1), dict(iou_threshold=math.nan), dict(iou_threshold="high"), dict(iou_mode="2d"),
                dict(score_threshold=math.nan), dict(score_threshold=0.0, from_logits=True),
                dict(score_threshold=1.0, from_logits=True), dict(score_threshold=-0.2, from_logits=True)):
        with pytest.raises(ValueError):
            boxes.detect(c["cls"], c["reg"], **bad)
    b, s = boxes.detect(c["cls"], c["reg"], score_threshold=None, from_logits=True, pre_nms_top_n=8, max_boxes=8)
    assert len(b) == len(s) == 8 and np.all((s > 0) & (s <= 1))                         # None: no threshold in either mode
