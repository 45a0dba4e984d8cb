"""Host side of the box-geometry kernels (include/lisec_hip.h section 5): the reference's label generation
(serialize_data.preprocessLabels) and RPN post-processing (rpnToRegion.rpnToRegion) with the same names."""
import ctypes
import math
import random

import numpy as np
import torch

from . import Constants, _lib
from ._lib import RpnCfg


def _cfg():
    c = RpnCfg()
    c.outX, c.outY = Constants.nx // 2, Constants.ny // 2
    c.vx, c.vy = Constants.voxelx * 2, Constants.voxely * 2
    for i, a in enumerate(Constants.anchors):
        for j in range(4):
            c.anchors[i][j] = float(a[j])
    return c


def rpnToRegion(labelsClass, labelsRegress, maxBoxes=20, overlapThresh=0., as_device=False):
    """rpnToRegion(labelsClass (100,200,2), labelsRegress (100,200,14)) -> (boxes (k,7), probs (k,))
    (rpnToRegion.py:113-164; the reference hard-codes maxBoxes=20, overlapThresh=0.).  Inputs may be numpy
    arrays or device tensors (e.g. views of LisecNet's head buffer).  Probability ties pick the larger flat
    index (the reference's np.argsort order among equal keys is unspecified).
    Deviation from the reference, on purpose: nonMaxSuppressionFast deletes the suppressed candidates with
    np.delete(idxs, toDelete) where toDelete holds box INDICES (rpnToRegion.py:66-67) -- a positional delete that
    removes unrelated entries and raises IndexError on numpy >= 1.19 for any realistic map.  Here the boxes found to
    overlap (IoU > overlapThresh) or to lie out of range are the ones suppressed (by value).
    as_device=True returns (boxes (maxBoxes+1,7), probs (maxBoxes+1,), count (1,) int32) as device tensors, the first `count`
    rows valid, without waiting for the GPU: what a caller that keeps scoring on the device (Predict.scoreMain) wants."""
    dev = _lib.require_gpu()
    lib = _lib.load()
    cfg = _cfg()
    cls = torch.as_tensor(labelsClass, dtype=torch.float32).to(dev)
    reg = torch.as_tensor(labelsRegress, dtype=torch.float32).to(dev)
    cls = cls.reshape(cfg.outX, cfg.outY, -1)
    reg = reg.reshape(cfg.outX, cfg.outY, -1)
    if cls.stride(-1) != 1 or reg.stride(-1) != 1:
        cls, reg = cls.contiguous(), reg.contiguous()
    ws = torch.empty(lib.lisec_rpn_to_region_workspace_bytes(ctypes.byref(cfg), maxBoxes), dtype=torch.uint8, device=dev)
    boxes = torch.zeros((maxBoxes + 1, 7), dtype=torch.float64, device=dev)
    probs = torch.zeros(maxBoxes + 1, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.lisec_rpn_to_region(ctypes.byref(cfg), _lib.ptr(cls), cls.stride(1), _lib.ptr(reg), reg.stride(1),
                                       float(overlapThresh), int(maxBoxes), _lib.ptr(ws), ws.numel(), _lib.ptr(boxes),
                                       _lib.ptr(probs), _lib.ptr(count), _lib.current_stream()))
    if as_device:
        return boxes, probs, count
    k = int(count.item())
    return boxes[:k].cpu().numpy(), probs[:k].cpu().numpy()


def _count(value, name, lo, hi):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, not {value!r}")
    return int(value)


def detect(labelsClass, labelsRegress, score_threshold=None, pre_nms_top_n=1000, max_boxes=100, iou_threshold=0.1,
           iou_mode='bev', from_logits=False, inside_only=True, as_device=False):
    """detect(labelsClass (100,200,2), labelsRegress (100,200,14)) -> (boxes (k,7) float64, scores (k,)) in descending score:
    the many-box path from the head to detections (lisec_detect; ours, rpnToRegion is the reference's).  The candidates
    above score_threshold whose decoded box is finite with positive extents (and, with inside_only, centred inside the
    grid) are cut to the pre_nms_top_n best, equal scores by the larger flat index as in rpnToRegion; greedy rotated NMS
    over those keeps a candidate unless a KEPT better one overlaps it with box_iou(mode=iou_mode) > iou_threshold, and stops
    at max_boxes.  Inputs are numpy arrays or device tensors, as for rpnToRegion.
    from_logits=False: the head is the reference's linear one; score_threshold is compared with the raw values, which are
    the scores returned.  from_logits=True: a head trained with VoxelNetLoss; score_threshold is a probability in (0, 1)
    (compared as the logit log(t / (1 - t)) with the raw values) and the scores returned are sigmoids.  None: no threshold.
    as_device=True returns (boxes (max_boxes,7), scores (max_boxes,), index (max_boxes,) int32 flat candidate index a*M+m,
    count (2,) int32 = kept, candidates that passed the filters) as device tensors, zero past the first `kept` rows,
    without waiting for the GPU.  pre_nms_top_n is at most 4096, max_boxes at most pre_nms_top_n."""
    from . import ops
    top_n = _count(pre_nms_top_n, "pre_nms_top_n", 1, _lib.DETECT_MAX_TOP_N)
    cap = _count(max_boxes, "max_boxes", 1, top_n)
    try:
        iou_t = float(iou_threshold)
        score_t = -math.inf if score_threshold is None else float(score_threshold)
    except (TypeError, ValueError):
        raise ValueError("score_threshold and iou_threshold must be numbers") from None
    if not 0.0 <= iou_t < 1.0:
        raise ValueError(f"iou_threshold must lie in [0, 1), not {iou_threshold!r}")
    if from_logits and score_threshold is not None:
        if not 0.0 < score_t < 1.0:
            raise ValueError(f"with from_logits the score_threshold is a probability in (0, 1), not {score_threshold!r}")
        score_t = math.log(score_t / (1.0 - score_t))
    if math.isnan(score_t):
        raise ValueError("score_threshold must not be NaN")
    det = ops.detect_params(score_t, bool(from_logits), top_n, cap, iou_t, _iou_mode(iou_mode), bool(inside_only))
    dev = _lib.require_gpu()
    cfg = _cfg()
    cls = torch.as_tensor(labelsClass, dtype=torch.float32).to(dev)
    reg = torch.as_tensor(labelsRegress, dtype=torch.float32).to(dev)
    cls = cls.reshape(cfg.outX, cfg.outY, -1)
    reg = reg.reshape(cfg.outX, cfg.outY, -1)
    if cls.stride(-1) != 1 or reg.stride(-1) != 1:
        cls, reg = cls.contiguous(), reg.contiguous()
    boxes, scores, index, count = ops.detect(cfg, det, cls, reg)
    if as_device:
        return boxes, scores, index, count
    k = int(count[0].item())
    return boxes[:k].cpu().numpy(), scores[:k].cpu().numpy()


def preprocessLabels(data, seed=0, balance=True):
    """preprocessLabels(data (B,7) rows x,y,z,l,w,h,yaw) -> [outClass (100,200,2), outRegress (100,200,14)]
    float64 (serialize_data.py:194-338).  The anchors x boxes IoU sweep runs on the GPU; the region balancing of
    :310-325 uses random.Random(seed) where the reference draws from the unseeded module-level `random`."""
    dev = _lib.require_gpu()
    lib = _lib.load()
    cfg = _cfg()
    data = np.asarray(data, dtype=np.float64).reshape(-1, 7)
    fixed = data.copy()                                    # fixBoxScaling (:181-191)
    fixed[:, [0, 3]] *= cfg.outX / Constants.nx
    fixed[:, [1, 4]] *= cfg.outY / Constants.ny
    B = len(fixed)
    d_fixed = torch.from_numpy(np.ascontiguousarray(fixed)).to(dev) if B else None
    cells = cfg.outX * cfg.outY
    valid = torch.empty(cells * 2, dtype=torch.float64, device=dev)
    overlap = torch.empty(cells * 2, dtype=torch.float64, device=dev)
    outreg = torch.empty(cells * 14, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.lisec_rpn_labels_workspace_bytes(B), dtype=torch.uint8, device=dev)
    _lib.check(lib.lisec_rpn_labels(ctypes.byref(cfg), _lib.ptr(d_fixed), B, float(Constants.iouLowerBound),
                                    float(Constants.iouUpperBound), _lib.ptr(ws), ws.numel(), _lib.ptr(valid),
                                    _lib.ptr(overlap), _lib.ptr(outreg), _lib.current_stream()))
    valid = valid.cpu().numpy().reshape(cfg.outX, cfg.outY, 2)
    overlap = overlap.cpu().numpy().reshape(cfg.outX, cfg.outY, 2)
    outreg = outreg.cpu().numpy().reshape(cfg.outX, cfg.outY, 14)
    if balance:
        _balance(valid, overlap, Constants.maxRegions, seed)
    return [valid + overlap, outreg + np.repeat(overlap, 7, axis=2)]


_TARGET_WS = {}


def rpnTargets(boxes, seed=0, item=0, epoch=0, balance=True, out=None, n_boxes=None):
    """The label maps of one sweep made on the device (lisec_rpn_targets; ours, not the reference's): boxes (B, 7) rows
    x, y, z, l, w, h, yaw in ego metres, numpy or a device tensor -> [y_cls (outX, outY, 2), y_reg (outX, outY, 14)] device
    float32, written into `out` = [y_cls, y_reg] when given (the target buffers of a recorded step).  No copy to the host
    and no wait.  balance=False equals float32(preprocessLabels(boxes, balance=False)) bit for bit; balance=True keeps at
    most maxRegions/2 positives and, when there are too many, as many negatives as positives (serialize_data.py:310-325)
    by the smallest Philox keys of (seed, item, epoch, anchor) -- reproducible, unlike the reference's random.sample.
    n_boxes: a device int32 (1,) holding the number of rows of `boxes` that count (lisec_rpn_targets_n: the count
    augment.sample_objects leaves on the device); the rows past it are ignored."""
    dev = _lib.require_gpu()
    lib = _lib.load()
    cfg = _cfg()
    if torch.is_tensor(boxes):
        d_boxes = boxes.to(device=dev, dtype=torch.float64).reshape(-1, 7).contiguous()
    else:
        d_boxes = torch.from_numpy(np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 7))).to(dev)
    B = int(d_boxes.shape[0])
    if out is None:
        out = [torch.empty((cfg.outX, cfg.outY, 2), dtype=torch.float32, device=dev),
               torch.empty((cfg.outX, cfg.outY, 14), dtype=torch.float32, device=dev)]
    y_cls, y_reg = out
    for t, c in ((y_cls, 2), (y_reg, 14)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != cfg.outX * cfg.outY * c:
            raise ValueError(f"out must be dense float32 maps of {cfg.outX} x {cfg.outY} x (2, 14)")
    key = (str(dev), cfg.outX, cfg.outY)
    need = lib.lisec_rpn_targets_workspace_bytes(ctypes.byref(cfg), max(B, 64))
    if key not in _TARGET_WS or _TARGET_WS[key].numel() < need:
        _TARGET_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    ws = _TARGET_WS[key]
    tail = (cfg.outX / Constants.nx, cfg.outY / Constants.ny, float(Constants.iouLowerBound), float(Constants.iouUpperBound),
            1 if balance else 0, int(Constants.maxRegions), int(seed) & (2 ** 64 - 1), int(item) & 0xffffffff,
            int(epoch) & 0xffffffff, _lib.ptr(ws), ws.numel(), _lib.ptr(y_cls), _lib.ptr(y_reg), _lib.current_stream())
    if n_boxes is None:
        _lib.check(lib.lisec_rpn_targets(ctypes.byref(cfg), _lib.ptr(d_boxes) if B else None, B, *tail))
    else:
        if n_boxes.dtype != torch.int32 or n_boxes.numel() != 1 or n_boxes.device != d_boxes.device:
            raise ValueError("n_boxes must be one int32 on the device")
        _lib.check(lib.lisec_rpn_targets_n(ctypes.byref(cfg), _lib.ptr(d_boxes) if B else None, _lib.ptr(n_boxes), B, *tail))
    return [y_cls, y_reg]


def _balance(valid, overlap, max_regions, seed):
    """serialize_data.py:310-325: keep <= maxRegions/2 positives and as many negatives as positives."""
    rng = random.Random(seed)
    pos = np.where(np.logical_and(valid == 1, overlap == 1))
    neg = np.where(np.logical_and(valid == 1, overlap == 0))
    pos_count = len(pos[0])
    if pos_count > max_regions / 2:
        locs = rng.sample(range(pos_count), int(pos_count - max_regions / 2))
        valid[pos[0][locs], pos[1][locs], pos[2][locs]] = 0
        pos_count = max_regions / 2
    if len(neg[0]) + pos_count > max_regions:
        locs = rng.sample(range(len(neg[0])), len(neg[0]) - int(pos_count))
        valid[neg[0][locs], neg[1][locs], neg[2][locs]] = 0


def quaternion_yaw(q):
    """pyquaternion's yaw_pitch_roll[0] for a (w,x,y,z) quaternion (serialize_data.py:360-361)."""
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return math.atan2(2 * (w * z - x * y), 1 - 2 * (y * y + z * z))


# ---- scoring detections against annotations (rpnToRegion.py:202-255) ---------------------------------------------------
def _pack_counted(box_list, dev):
    """[(k_s, 7) arrays or device tensors] -> (device (max(rows, 1), 7) float64, host int32 (S+1,) row offsets)."""
    rows = [b.to(device=dev, dtype=torch.float64).reshape(-1, 7) if torch.is_tensor(b)
            else torch.from_numpy(np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1, 7))) for b in box_list]
    start = np.zeros(len(rows) + 1, dtype=np.int32)
    start[1:] = np.cumsum([len(r) for r in rows])
    if all(not r.is_cuda for r in rows):                       # host lists: one upload
        flat = torch.cat(rows + [torch.zeros((1, 7), dtype=torch.float64)]).to(dev)
    else:
        flat = torch.cat([r.to(dev) for r in rows] + [torch.zeros((1, 7), dtype=torch.float64, device=dev)])
    return flat, start


def _pack(box_list, dev):
    """_pack_counted with the row offsets on the device."""
    flat, start = _pack_counted(box_list, dev)
    return flat, torch.from_numpy(start).to(dev)


def union_overlap(pred_list, label_list):
    """For S samples at once -- pred_list[s], label_list[s]: (k, 7) rows x,y,z,l,w,h,yaw, numpy or device tensors --
    returns (S, 5) float64: area((U pred) n (U label)), area(U pred), area(U label), sum of pred l*w*h, sum of label l*w*h
    (lisec_boxes_union_overlap).  One launch and one device-to-host copy for the whole list."""
    if len(pred_list) != len(label_list):
        raise ValueError("union_overlap needs one label set per prediction set")
    dev = _lib.require_gpu()
    lib = _lib.load()
    S = len(pred_list)
    pred, pred_start = _pack(pred_list, dev)
    label, label_start = _pack(label_list, dev)
    out = torch.empty((S, 5), dtype=torch.float64, device=dev)
    nbytes = lib.lisec_boxes_union_overlap_workspace_bytes(S, int(pred.shape[0]), int(label.shape[0]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    _lib.check(lib.lisec_boxes_union_overlap(_lib.ptr(pred), _lib.ptr(pred_start), _lib.ptr(label), _lib.ptr(label_start),
                                             S, _lib.ptr(ws), nbytes, _lib.ptr(out), _lib.current_stream()))
    return out.cpu().numpy()


def calcIntersectAll(boxBoxes, annsBoxes):
    """calcIntersectAll (rpnToRegion.py:202-213): the AREA of (union of the predicted footprints) n (union of the annotated
    ones) -- cascaded_union(...).intersection(cascaded_union(...)).area there, a GPU boundary integral here."""
    return float(union_overlap([boxBoxes], [annsBoxes])[0, 0])


def calcUnionAll(boxesBoxes, annsBoxes, intersect):
    """calcUnionAll (rpnToRegion.py:215-222), literally: the sum of the box VOLUMES of both sides minus `intersect` (which
    calcIoUAll passes as an area -- the reference's quirk, kept)."""
    annsSum = 0
    for box in annsBoxes:
        annsSum += box[3] * box[4] * box[5]
    predictSum = 0
    for box in boxesBoxes:
        predictSum += box[3] * box[4] * box[5]
    return annsSum + predictSum - intersect


def _host_rows(b):
    return b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64).reshape(-1, 7)


def calcIoUAll_boxes(predictBoxes, labelBoxes):
    """The last three lines of calcIoUAll (rpnToRegion.py:253-255) on two box tables: intersect / union with the
    reference's mixed units (area over volumes).  Both sides empty: ZeroDivisionError, as the reference's 0.0 / 0."""
    predictBoxes, labelBoxes = _host_rows(predictBoxes), _host_rows(labelBoxes)
    intersect = calcIntersectAll(predictBoxes, labelBoxes)
    union = calcUnionAll(predictBoxes, labelBoxes, intersect)
    return intersect / union                                   # both empty: 0.0 / 0.0 of Python floats raises


def _bev(row):
    union = row[1] + row[2] - row[0]
    return float(row[0] / union) if union > 0 else 0.0


def bev_iou(predictBoxes, labelBoxes):
    """Bird's-eye IoU of the two box sets: area((U pred) n (U label)) / area((U pred) u (U label)); 0.0 when both sides are
    empty.  This one is OURS, not the reference's: calcIoUAll divides the same area by a sum of volumes."""
    return _bev(union_overlap([predictBoxes], [labelBoxes])[0])


def annotationBoxes(sample, dataset):
    """The label rows of calcIoUAll (rpnToRegion.py:225-251): the sample's annotations moved from global to ego
    coordinates (translate, then the inverse ego rotation), rows [x, y, z, *size, yaw], cars inside the closed +-50 m
    window only.  Returns (k, 7) float64.  `dataset` is anything with LyftDataset's get(table, token)."""
    from .model_training import rotate_points
    sd = dataset.get('sample_data', sample['data']['LIDAR_TOP'])
    ego = dataset.get('ego_pose', sd['ego_pose_token'])
    labels = []
    for token in sample['anns']:
        ann = dataset.get('sample_annotation', token)
        t = np.array(ann['translation'], dtype=np.float64).reshape(1, -1) - np.array(ego['translation'])
        t = rotate_points(t, np.array(ego['rotation']), True)
        row = [t[0, 0], t[0, 1], t[0, 2]] + list(ann['size']) + [quaternion_yaw(ann['rotation'])]
        instance = dataset.get('instance', ann['instance_token'])
        category = dataset.get('category', instance['category_token'])['name']
        if category == 'car' and row[0] >= -50 and row[0] <= 50 and row[1] >= -50 and row[1] <= 50:
            labels.append(row)
    return np.array(labels, dtype=np.float64).reshape(-1, 7)


# ---- detection average precision (ours; the reference has no counterpart) ----------------------------------------------
_IOU_MODES = {'3d': 0, 'bev': 1}                               # LISEC_IOU_3D, LISEC_IOU_BEV
MAX_IOU_THRESHOLDS = 16


class DetectionAP:
    """What average_precision returns: ap (T,), mAP, thresholds (T,), tp (T, N) bool in input order, tp_count (n_samples, T),
    best_iou (N,), best_label (N,) (row within the sample, -1 without labels), n_predictions, n_labels."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        return (f"DetectionAP(mAP={self.mAP:.6f}, n_predictions={self.n_predictions}, n_labels={self.n_labels}, "
                f"ap={np.array2string(self.ap, precision=4)})")


def _iou_mode(mode):
    if mode not in _IOU_MODES:
        raise ValueError(f"mode must be one of {sorted(_IOU_MODES)}, not {mode!r}")
    return _IOU_MODES[mode]


def _iou_thresholds(iou_thresholds):
    thr = np.arange(0.5, 1.0, 0.05) if iou_thresholds is None else np.asarray(iou_thresholds, dtype=np.float64).reshape(-1)
    if not 1 <= len(thr) <= MAX_IOU_THRESHOLDS:
        raise ValueError(f"between 1 and {MAX_IOU_THRESHOLDS} IoU thresholds are accepted, not {len(thr)}")
    if not np.all((thr >= 0) & (thr < 1)):
        raise ValueError(f"IoU thresholds must lie in [0, 1): {thr.tolist()}")
    return thr


def _rows7(b):
    return b.reshape(-1, 7) if torch.is_tensor(b) else np.asarray(b, dtype=np.float64).reshape(-1, 7)


def _pack_samples(pred_list, label_list, dev):
    """Both sides of a list of samples on the device: (pred, pred_start, label, label_start) with the offsets as device
    int32 (S+1,), the host copy of pred_start, and the host counts N, G and total pairs (sum of n_pred * n_label)."""
    if len(pred_list) != len(label_list):
        raise ValueError("one label set per prediction set")
    pred, pred_start = _pack_counted(pred_list, dev)
    label, label_start = _pack_counted(label_list, dev)
    pairs = int((np.diff(pred_start).astype(np.int64) * np.diff(label_start).astype(np.int64)).sum())
    return (pred, torch.from_numpy(pred_start).to(dev), label, torch.from_numpy(label_start).to(dev), pred_start,
            int(pred_start[-1]), int(label_start[-1]), pairs)


def _pack_scores(score_list, pred_start, dev):
    """The scores of all samples as one device float64 row (one pad element); one score per prediction, else ValueError."""
    flat = [c.to(device=dev, dtype=torch.float64).reshape(-1) if torch.is_tensor(c)
            else torch.from_numpy(np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(-1))) for c in score_list]
    if [len(c) for c in flat] != np.diff(pred_start).tolist():
        raise ValueError("every prediction needs exactly one score")
    return torch.cat([c.to(dev) for c in flat] + [torch.zeros(1, dtype=torch.float64, device=dev)])


def _match(pred_list, score_list, label_list, thr, mode):
    """lisec_boxes_match on a list of samples.  Returns device tensors (best_iou, best_label, tp (T, N), tp_count (S, T), flat
    scores) and the host counts N, G."""
    if len(pred_list) != len(score_list):
        raise ValueError("one score set per prediction set")
    dev = _lib.require_gpu()
    lib = _lib.load()
    S, T = len(pred_list), len(thr)
    pred, d_pred_start, label, d_label_start, pred_start, N, G, pairs = _pack_samples(pred_list, label_list, dev)
    scores = _pack_scores(score_list, pred_start, dev)
    ws = torch.empty(max(lib.lisec_boxes_match_workspace_bytes(S, N, pairs, T), 1), dtype=torch.uint8, device=dev)
    best_iou = torch.empty(max(N, 1), dtype=torch.float64, device=dev)
    best_label = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    tp = torch.empty(T * max(N, 1), dtype=torch.uint8, device=dev)
    tp_count = torch.empty((max(S, 1), T), dtype=torch.int32, device=dev)
    _lib.check(lib.lisec_boxes_match(_lib.ptr(pred), _lib.ptr(scores), _lib.ptr(d_pred_start),
                                     _lib.ptr(label), _lib.ptr(d_label_start), S, N, pairs,
                                     (ctypes.c_double * T)(*thr.tolist()), T, mode, _lib.ptr(ws), ws.numel(),
                                     _lib.ptr(best_iou), _lib.ptr(best_label), _lib.ptr(tp), _lib.ptr(tp_count),
                                     _lib.current_stream()))
    return best_iou[:N], best_label[:N], tp[:T * N].reshape(T, N), tp_count[:S], scores[:N], N, G


def box_iou(predictBoxes, labelBoxes, mode='3d'):
    """The (n_pred, n_label) float64 IoU matrix of one sample's predictions and labels (rows x, y, z, l, w, h, yaw; arrays or
    device tensors; lisec_boxes_pair_iou).  mode='3d': inter = footprint overlap area * the CLAMPED z overlap of the two height
    intervals [z - |h|/2, z + |h|/2], union = |l w h|_p + |l w h|_g - inter; mode='bev': the same with areas only.  A box with
    l == 0 or w == 0 (or h == 0 in 3D mode) has IoU 0 with everything; a negative extent mirrors the footprint.  This IoU is
    OURS, as bev_iou is: geometrically consistent, not the reference's calculateIoU (serialize_data.py:170-178), whose z term
    takes the full height as half extent and is not clamped."""
    mode = _iou_mode(mode)
    dev = _lib.require_gpu()
    lib = _lib.load()
    pred, d_pred_start, label, d_label_start, _, N, G, pairs = _pack_samples([predictBoxes], [labelBoxes], dev)
    ws = torch.empty(max(lib.lisec_boxes_match_workspace_bytes(1, N, 0, 1), 1), dtype=torch.uint8, device=dev)
    out = torch.empty(max(pairs, 1), dtype=torch.float64, device=dev)
    _lib.check(lib.lisec_boxes_pair_iou(_lib.ptr(pred), _lib.ptr(d_pred_start), _lib.ptr(label), _lib.ptr(d_label_start), 1, N,
                                        pairs, mode, _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.current_stream()))
    return out[:pairs].cpu().numpy().reshape(N, G)


def average_precision(pred_list, score_list, label_list, iou_thresholds=None, mode='3d'):
    """Detection average precision of score-ranked boxes against annotations, over all samples of the lists (pred_list[s]
    (k, 7), score_list[s] (k,), label_list[s] (m, 7); arrays or device tensors), PASCAL-VOC style:
    rank all predictions by descending score (ties: sample index, then row); a prediction's candidate is the label of its own
    sample with the largest box_iou (ties: lowest row); it is a true positive at threshold t when that IoU > t and no
    earlier-ranked prediction took the label at t; AP(t) = area under the precision envelope over recall; mAP = their mean.
    iou_thresholds: up to 16 values in [0, 1), default 0.5, 0.55, .., 0.95.  Matching and integration run on the device
    (lisec_boxes_match, lisec_boxes_average_precision) with one copy back at the end.  Returns a DetectionAP.  No labels at all:
    ValueError; no predictions: AP 0.  The IoU is ours (see box_iou) and the rule restates what the Lyft devkit is understood
    to do: parity with it is unpinned."""
    thr = _iou_thresholds(iou_thresholds)
    mode = _iou_mode(mode)
    if sum(len(_rows7(b)) for b in label_list) == 0:
        raise ValueError("average precision is undefined without labels")
    best_iou, best_label, tp, tp_count, scores, N, G = _match(pred_list, score_list, label_list, thr, mode)
    lib = _lib.load()
    nan = torch.isnan(scores).any()                                       # read with the results: no copy between the stages
    rank = torch.sort(scores, descending=True, stable=True).indices       # plumbing: ties keep the flat (sample, row) order
    ap = torch.empty(len(thr), dtype=torch.float64, device=scores.device)
    _lib.check(lib.lisec_boxes_average_precision(_lib.ptr(rank) if N else None, _lib.ptr(tp) if N else None, N, G, len(thr),
                                                 _lib.ptr(ap), None, _lib.current_stream()))
    ap = ap.cpu().numpy()
    if bool(nan):
        raise ValueError("scores must not be NaN")
    return DetectionAP(ap=ap, mAP=float(ap.mean()), thresholds=thr, tp=tp.cpu().numpy().astype(bool),
                       tp_count=tp_count.cpu().numpy(), best_iou=best_iou.cpu().numpy(), best_label=best_label.cpu().numpy(),
                       n_predictions=N, n_labels=G)


# ---- detection evaluation: ignored labels, heading score, true-positive errors (ours; the reference has no counterpart) ----
EVAL_WORDS = 7                                                 # LISEC_EVAL_WORDS
_EVAL_FIELDS = ('ap', 'aos', 'ate', 'ase', 'aoe', 'best_f1', 'best_f1_score')      # LISEC_EVAL_AP .. LISEC_EVAL_BEST_F1_SCORE


class DetectionEval:
    """What evaluate_detections returns: ap, aos, ate, ase, aoe, best_f1, best_f1_score (each (T,)), mAP, mAOS, thresholds
    (T,), state (T, N) uint8 in input order (0 false positive, 1 true positive, 2 ignored), tp (T, N) bool = state == 1,
    tp_count (n_samples, T), best_iou (N,), best_label (N,) (row within the sample among ALL its labels, -1 without a
    non-ignored one), ignored_iou (N,), geom (N, 4) = (sim, dist, scale, yaw) against the candidate, n_predictions,
    n_labels (non-ignored), n_ignored_labels, and curve (T, N, 3) = (rec, prec, os) per rank when asked for."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        return (f"DetectionEval(mAP={self.mAP:.6f}, mAOS={self.mAOS:.6f}, n_predictions={self.n_predictions}, "
                f"n_labels={self.n_labels}, n_ignored_labels={self.n_ignored_labels}, "
                f"ap={np.array2string(self.ap, precision=4)})")


def points_in_boxes(points, boxes, as_device=False):
    """The number of points each box owns: points (n, >= 3), boxes (m, 7) rows x, y, z, l, w, h, yaw, arrays or device
    tensors -> (m,) int64 (a device tensor with as_device=True, without waiting for the GPU).  ObjectDatabase's rule
    (lisec_augment_owner): the closed slab test, and a point inside several boxes belongs to the lowest index; counting
    the owners is plumbing."""
    from . import augment, ops
    dev = _lib.require_gpu()
    pts, rows = augment._device_points(points, dev), augment._device_boxes(boxes, dev)
    m = int(rows.shape[0])
    if m == 0:
        per_box = torch.zeros(0, dtype=torch.int64, device=dev)
    else:
        own = ops.augment_owner(pts, rows, augment.PAD_LIMIT).long()
        per_box = torch.bincount(own + 1, minlength=m + 1)[1:]
    return per_box if as_device else per_box.cpu().numpy()


def _flags(flag_list, box_list, what):
    """One host bool array per sample, as long as its boxes; None: nothing flagged."""
    sizes = [len(_rows7(b)) for b in box_list]
    if flag_list is None:
        return [np.zeros(n, dtype=bool) for n in sizes]
    if len(flag_list) != len(sizes):
        raise ValueError(f"{what} needs one flag array per sample")
    out = [(f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)).reshape(-1).astype(bool) for f in flag_list]
    if [len(f) for f in out] != sizes:
        raise ValueError(f"{what} needs exactly one flag per box")
    return out


def _device_flags(flags, dev):
    """The flags of all samples as one device uint8 row (one pad element), or None when none is set (NULL to the kernel)."""
    flat = np.concatenate(flags + [np.zeros(1, dtype=bool)])
    return torch.from_numpy(flat.astype(np.uint8)).to(dev) if flat.any() else None


def evaluate_detections(pred_list, score_list, label_list, label_ignore=None, pred_ignore=None, iou_thresholds=None,
                        mode='3d', curve=False):
    """average_precision with what a lidar benchmark adds to it (lisec_boxes_evaluate, lisec_boxes_evaluate_integrate; the
    definition is include/lisec_hip.h's).  label_ignore[s] (m,) / pred_ignore[s] (k,): truthy = ignored, None: none is.
    An ignored label is neither a hit nor a miss: it is no candidate and does not count in G, and a prediction that is no
    true positive but overlaps one with IoU > t, or carries pred_ignore, is left out of the ranking at t instead of
    counting as a false positive.  Returns a DetectionEval: AP and the heading-weighted AOS per threshold and their means,
    the true-positive errors ATE (centre distance, m), ASE (1 - aligned IoU) and AOE (|yaw difference|, rad) per threshold,
    the best F1 over the ranking and the score that attains it (the score_threshold to hand to detect).  Without flags
    ap, tp, tp_count, best_iou and best_label are average_precision's bit for bit.  Packing, the NaN-score check and the
    rank (a stable descending sort) are average_precision's.  ValueError: flag lists that do not match their boxes, no
    non-ignored label at all, NaN scores."""
    thr = _iou_thresholds(iou_thresholds)
    mode = _iou_mode(mode)
    if len(pred_list) != len(score_list):
        raise ValueError("one score set per prediction set")
    if len(pred_list) != len(label_list):
        raise ValueError("one label set per prediction set")
    l_flags = _flags(label_ignore, label_list, "label_ignore")
    p_flags = _flags(pred_ignore, pred_list, "pred_ignore")
    n_ignored = int(sum(int(f.sum()) for f in l_flags))
    G = int(sum(len(f) for f in l_flags)) - n_ignored
    if G <= 0:
        raise ValueError("the evaluation is undefined without a label that is not ignored")
    dev = _lib.require_gpu()
    lib = _lib.load()
    S, T = len(pred_list), len(thr)
    pred, d_pred_start, label, d_label_start, pred_start, N, _, pairs = _pack_samples(pred_list, label_list, dev)
    scores = _pack_scores(score_list, pred_start, dev)
    d_label_ignore, d_pred_ignore = _device_flags(l_flags, dev), _device_flags(p_flags, dev)
    ws = torch.empty(max(lib.lisec_boxes_evaluate_workspace_bytes(S, N, pairs, T), 1), dtype=torch.uint8, device=dev)
    best_iou = torch.empty(max(N, 1), dtype=torch.float64, device=dev)
    best_label = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    ignored_iou = torch.empty(max(N, 1), dtype=torch.float64, device=dev)
    geom = torch.empty((max(N, 1), 4), dtype=torch.float64, device=dev)
    state = torch.empty(T * max(N, 1), dtype=torch.uint8, device=dev)
    tp_count = torch.empty((max(S, 1), T), dtype=torch.int32, device=dev)
    st = _lib.current_stream()
    _lib.check(lib.lisec_boxes_evaluate(_lib.ptr(pred), _lib.ptr(scores), _lib.ptr(d_pred_start), _lib.ptr(d_pred_ignore),
                                        _lib.ptr(label), _lib.ptr(d_label_start), _lib.ptr(d_label_ignore), S, N, pairs,
                                        (ctypes.c_double * T)(*thr.tolist()), T, mode, _lib.ptr(ws), ws.numel(),
                                        _lib.ptr(best_iou), _lib.ptr(best_label), _lib.ptr(ignored_iou), _lib.ptr(geom),
                                        _lib.ptr(state), _lib.ptr(tp_count), st))
    nan = torch.isnan(scores[:N]).any()                                   # read with the results: no copy between the stages
    rank = torch.sort(scores[:N], descending=True, stable=True).indices   # plumbing: ties keep the flat (sample, row) order
    out = torch.empty((T, EVAL_WORDS), dtype=torch.float64, device=dev)
    d_curve = torch.empty((T, max(N, 1), 3), dtype=torch.float64, device=dev) if curve else None
    _lib.check(lib.lisec_boxes_evaluate_integrate(_lib.ptr(rank) if N else None, _lib.ptr(state) if N else None,
                                                  _lib.ptr(geom) if N else None, _lib.ptr(scores) if N else None, N, G, T,
                                                  _lib.ptr(out), _lib.ptr(d_curve), st))
    out = out.cpu().numpy()
    if bool(nan):
        raise ValueError("scores must not be NaN")
    state = state[:T * N].reshape(T, N).cpu().numpy()
    fields = {name: out[:, i].copy() for i, name in enumerate(_EVAL_FIELDS)}
    if curve:
        fields['curve'] = d_curve[:, :N].cpu().numpy()
    return DetectionEval(mAP=float(fields['ap'].mean()), mAOS=float(fields['aos'].mean()), thresholds=thr, state=state,
                         tp=state == 1, tp_count=tp_count[:S].cpu().numpy(), best_iou=best_iou[:N].cpu().numpy(),
                         best_label=best_label[:N].cpu().numpy(), ignored_iou=ignored_iou[:N].cpu().numpy(),
                         geom=geom[:N].cpu().numpy(), n_predictions=N, n_labels=G, n_ignored_labels=n_ignored, **fields)


def _centre_distance(b):
    """hypot(x, y) of box rows, on the host (flags travel as host arrays)."""
    rows = b.detach().cpu().numpy().reshape(-1, 7) if torch.is_tensor(b) else np.asarray(b, dtype=np.float64).reshape(-1, 7)
    return np.hypot(rows[:, 0], rows[:, 1])


def evaluate_by_range(pred_list, score_list, label_list, ranges=((0, 30), (30, 50), (50, math.inf)), label_ignore=None, **kw):
    """evaluate_detections once per distance bin: {(lo, hi): DetectionEval}.  Within a bin a label whose centre distance
    hypot(x, y) lies outside [lo, hi) is ignored (ORed with label_ignore) and a prediction outside it carries pred_ignore
    (ORed with the one given): what lies in another bin is neither a hit nor a miss here.  A bin without a non-ignored label
    maps to None.  The other keyword arguments are evaluate_detections'."""
    l_flags = _flags(label_ignore, label_list, "label_ignore")
    p_flags = _flags(kw.pop('pred_ignore', None), pred_list, "pred_ignore")
    l_dist = [_centre_distance(b) for b in label_list]
    p_dist = [_centre_distance(b) for b in pred_list]
    out = {}
    for lo, hi in ranges:
        lo, hi = float(lo), float(hi)
        l_bin = [f | ~((d >= lo) & (d < hi)) for f, d in zip(l_flags, l_dist)]
        p_bin = [f | ~((d >= lo) & (d < hi)) for f, d in zip(p_flags, p_dist)]
        if all(f.all() for f in l_bin):
            out[(lo, hi)] = None
            continue
        out[(lo, hi)] = evaluate_detections(pred_list, score_list, label_list, label_ignore=l_bin, pred_ignore=p_bin, **kw)
    return out
