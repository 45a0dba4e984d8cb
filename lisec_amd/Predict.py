"""Drop-in counterpart of the reference's Predict.py: predictMain(samples, outPath, level5Data, model)."""
import os
import time

import numpy as np

from . import Constants
from .model_training import (MaxPoolingVFELayer, RepeatLayer, VFE_preprocessing, combine_lidar_data,  # noqa: F401
                             load_model, sparse)


def predictMain(samples, outPath, level5Data, model, dataDir=None):
    """For every sample: assemble the lidar sweep, voxelise, run the network in inference mode and save
    outPath/sample{i}_label.npy (1,100,200,2) and outPath/sample{i}_regress.npy (1,100,200,14), float32
    (Predict.py:9-40; the reference joins the path with a literal backslash, i.e. Windows only)."""
    dataDir = dataDir if dataDir is not None else Constants.lyft_data_dir
    os.makedirs(outPath, exist_ok=True)
    for i in range(len(samples)):
        sampleLidarPoints = combine_lidar_data(samples[i], dataDir, level5Data)
        startTime = time.time()
        trainVFEPoints = VFE_preprocessing(sampleLidarPoints, Constants.voxelx, Constants.voxely, Constants.voxelz,
                                           Constants.maxPoints, Constants.nx // 2, Constants.ny // 2, Constants.nz)
        trainVFEPoints = sparse.reshape(trainVFEPoints, (1,) + trainVFEPoints.shape)     # Predict.py:29
        print(time.time() - startTime)
        print('finished ' + str(i))
        prob, regress = model.predict(trainVFEPoints)                                     # Predict.py:38
        np.save(os.path.join(outPath, 'sample' + str(i) + '_label.npy'), prob)
        np.save(os.path.join(outPath, 'sample' + str(i) + '_regress.npy'), regress)


def _check_detector(detector):
    if detector is not None and "as_device" in detector:
        raise ValueError("the detector's results stay on the device here: as_device is not one of its arguments")


def _detect_sweep(points, model, detector=None, maxBoxes=20, overlapThresh=0.):
    """From the points of one sweep onward, without leaving the device: voxelise, the inference forward, decode + NMS on the
    head views, the shift to ego-centred metres (rpnToRegion.py:279-280).  detector=None: boxes.rpnToRegion, the reference's
    loop, with maxBoxes and overlapThresh; a dict: boxes.detect with these keyword arguments.  Returns [(boxes, scores, count
    (1,) int32)] as device tensors, the first `count` rows valid -- nothing waits for the GPU.  _detect and
    callbacks.DetectionEvaluation share it."""
    from . import boxes
    vfe = VFE_preprocessing(points, Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints,
                            Constants.nx // 2, Constants.ny // 2, Constants.nz)
    out = []
    for s in model._as_samples(vfe):
        cls, reg = model.net.forward(s, training=False)
        if detector is None:
            b, p, count = boxes.rpnToRegion(cls[0], reg[0], maxBoxes=maxBoxes, overlapThresh=overlapThresh,
                                            as_device=True)          # before the next forward reuses the head
        else:
            b, p, _, count = boxes.detect(cls[0], reg[0], as_device=True, **detector)
            count = count[:1]
        b[:, 0] -= 50
        b[:, 1] -= 50
        out.append((b, p, count))
    return out


def _cut_to_counts(found, probs, counts):
    """The valid rows of every sweep's detections: the counts come back in ONE copy."""
    import torch
    counts = torch.cat(counts).cpu().tolist() if counts else []
    return [b[:k] for b, k in zip(found, counts)], [p[:k] for p, k in zip(probs, counts)]


def _detect(samples, level5Data, model, dataDir=None, maxBoxes=20, overlapThresh=0., detector=None, with_labels=True,
            min_points=0):
    """The per-sample loop scoreMain, detectionAP, detectionEval and detectMain share: the sweep of every sample through
    _detect_sweep.  Returns ([boxes (k, 7)], [scores (k,)]) as device tensors and [annotationBoxes] -- the counts come back in
    ONE copy at the end.  With min_points > 0 a fourth list follows: per sample, the device int64 (m,) number of points of
    its own sweep each annotation owns (boxes.points_in_boxes)."""
    from . import boxes
    _check_detector(detector)
    dataDir = dataDir if dataDir is not None else Constants.lyft_data_dir
    found, probs, counts, labels, owned = [], [], [], [], []
    for sample in samples:
        points = combine_lidar_data(sample, dataDir, level5Data)
        for b, p, count in _detect_sweep(points, model, detector, maxBoxes, overlapThresh):
            found.append(b)
            probs.append(p)
            counts.append(count)
        if with_labels:
            labels.append(boxes.annotationBoxes(sample, level5Data))
            if min_points > 0:
                owned.append(boxes.points_in_boxes(points, labels[-1], as_device=True))
    found, probs = _cut_to_counts(found, probs, counts)
    return (found, probs, labels, owned) if min_points > 0 else (found, probs, labels)


def scoreMain(samples, level5Data, model, dataDir=None):
    """The check at the end of the reference's rpnToRegion.py (:276-295) for a list of samples, without leaving the
    device in between: predict, decode + NMS on the head views (boxes.rpnToRegion), the shift to ego-centred metres
    (:279-280), and ONE launch that scores every sample against its car annotations (boxes.union_overlap).
    Returns [(reference IoU, bird's-eye IoU)] per sample: calcIoUAll's area / (sum of volumes - area), and
    boxes.bev_iou's area / area, which is ours."""
    from . import boxes
    found, _, labels = _detect(samples, level5Data, model, dataDir)
    if not found:
        return []
    out = boxes.union_overlap(found, labels)
    return [(float(r[0]) / (float(r[3]) + float(r[4]) - float(r[0])), boxes._bev(r)) for r in out]


def detectMain(samples, level5Data, model, dataDir=None, **detector):
    """The detections of a list of samples: predict, then boxes.detect on the head views with the keyword arguments given
    (score_threshold, pre_nms_top_n, max_boxes, iou_threshold, iou_mode, from_logits, inside_only), in ego-centred metres
    (the same -50 shift as scoreMain).  Returns [(boxes (k, 7), scores (k,))] per sample, float64 arrays in descending
    score.  Nothing waits for the GPU inside the loop: the counts come back in one copy at the end, then the rows."""
    import torch
    found, scores, _ = _detect(samples, level5Data, model, dataDir, detector=detector, with_labels=False)
    if not found:
        return []
    rows = torch.cat([torch.cat([b, s[:, None]], dim=1) for b, s in zip(found, scores)]).cpu().numpy()
    out, at = [], 0
    for b in found:
        out.append((rows[at:at + len(b), :7].copy(), rows[at:at + len(b), 7].copy()))
        at += len(b)
    return out


def detectionAP(samples, level5Data, model, iou_thresholds=None, mode='3d', maxBoxes=20, overlapThresh=0., dataDir=None,
                detector=None):
    """The data set's detection metric for a list of samples: the same loop as scoreMain with the class probabilities kept
    as scores, then ONE boxes.average_precision call over all samples -- average precision of the score-ranked boxes
    against the car annotations at the 3D IoU thresholds 0.5, 0.55, .., 0.95 and their mean (mAP).  Returns
    boxes.DetectionAP.  Ours: the reference has no such check, and parity with the Lyft devkit is unpinned.
    detector=None ranks the maxBoxes boxes of boxes.rpnToRegion, the reference's loop; a dict of boxes.detect's keyword
    arguments (e.g. dict(score_threshold=0.3, from_logits=True, max_boxes=300)) ranks that path's detections instead, and
    maxBoxes and overlapThresh are not used."""
    from . import boxes
    found, probs, labels = _detect(samples, level5Data, model, dataDir, maxBoxes, overlapThresh, detector)
    return boxes.average_precision(found, probs, labels, iou_thresholds=iou_thresholds, mode=mode)


def detectionEval(samples, level5Data, model, iou_thresholds=None, mode='3d', detector=None, maxBoxes=20, overlapThresh=0.,
                  min_points=0, ranges=None, dataDir=None):
    """detectionAP's loop scored by boxes.evaluate_detections: AP, the heading-weighted AOS, the true-positive errors and
    the best-F1 operating point per IoU threshold (boxes.DetectionEval).  min_points > 0: an annotation that owns fewer
    points of its own sweep (boxes.points_in_boxes on what combine_lidar_data returned) is ignored -- neither a hit nor a
    miss, as KITTI's "don't care" and nuScenes' boxes without points are.  ranges: distance bins ((lo, hi), ...) in metres;
    the result is then boxes.evaluate_by_range's dict, one DetectionEval (or None) per bin.  detector, maxBoxes and
    overlapThresh are detectionAP's."""
    import torch
    from . import boxes
    got = _detect(samples, level5Data, model, dataDir, maxBoxes, overlapThresh, detector, min_points=max(int(min_points), 0))
    found, probs, labels = got[:3]
    ignore = None
    if min_points > 0 and labels:
        few = (torch.cat(got[3]) < int(min_points)).cpu().numpy()            # one copy for all samples
        at = np.cumsum([0] + [len(g) for g in labels])
        ignore = [few[at[i]:at[i + 1]] for i in range(len(labels))]
    if ranges is not None:
        return boxes.evaluate_by_range(found, probs, labels, ranges=ranges, label_ignore=ignore, iou_thresholds=iou_thresholds,
                                       mode=mode)
    return boxes.evaluate_detections(found, probs, labels, label_ignore=ignore, iou_thresholds=iou_thresholds, mode=mode)


if __name__ == '__main__':
    # python -m lisec_amd.Predict [model.h5] [outPath]      (Predict.py:43-59)
    import sys
    from .model_training import MaxPoolingVFELayer, RepeatLayer, _lyft_dataset, load_model
    level5Data = _lyft_dataset()
    model = load_model(sys.argv[1] if len(sys.argv) > 1 else os.path.join('fixedTheta', '15SampleEpoch0_fixed.h5'),
                       custom_objects={'RepeatLayer': RepeatLayer, 'MaxPoolingVFELayer': MaxPoolingVFELayer})
    samples = [level5Data.get('sample', scene['first_sample_token']) for scene in level5Data.scene]
    print('Testing on ' + str(len(samples)))
    predictMain(samples, sys.argv[2] if len(sys.argv) > 2 else 'fixedTheta', level5Data, model)
