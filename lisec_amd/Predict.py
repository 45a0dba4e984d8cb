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


def _detect(samples, level5Data, model, dataDir=None, maxBoxes=20, overlapThresh=0.):
    """The per-sample loop scoreMain and detectionAP share, without leaving the device: predict, decode + NMS on the head
    views (boxes.rpnToRegion), the shift to ego-centred metres (rpnToRegion.py:279-280).  Returns ([boxes (k, 7)],
    [probabilities (k,)]) as device tensors and [annotationBoxes] -- the counts come back in ONE copy at the end."""
    import torch
    from . import boxes
    dataDir = dataDir if dataDir is not None else Constants.lyft_data_dir
    found, probs, counts, labels = [], [], [], []
    for sample in samples:
        points = combine_lidar_data(sample, dataDir, level5Data)
        vfe = VFE_preprocessing(points, Constants.voxelx, Constants.voxely, Constants.voxelz, Constants.maxPoints,
                                Constants.nx // 2, Constants.ny // 2, Constants.nz)
        for s in model._as_samples(vfe):
            cls, reg = model.net.forward(s, training=False)
            b, p, count = boxes.rpnToRegion(cls[0], reg[0], maxBoxes=maxBoxes, overlapThresh=overlapThresh,
                                            as_device=True)              # before the next forward reuses the head
            b[:, 0] -= 50
            b[:, 1] -= 50
            found.append(b)
            probs.append(p)
            counts.append(count)
        labels.append(boxes.annotationBoxes(sample, level5Data))
    counts = torch.cat(counts).cpu().tolist() if counts else []
    return [b[:k] for b, k in zip(found, counts)], [p[:k] for p, k in zip(probs, counts)], labels


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


def detectionAP(samples, level5Data, model, iou_thresholds=None, mode='3d', maxBoxes=20, overlapThresh=0., dataDir=None):
    """The data set's detection metric for a list of samples: the same loop as scoreMain with the class probabilities kept
    as scores, then ONE boxes.average_precision call over all samples -- average precision of the score-ranked boxes
    against the car annotations at the 3D IoU thresholds 0.5, 0.55, .., 0.95 and their mean (mAP).  Returns
    boxes.DetectionAP.  Ours: the reference has no such check, and parity with the Lyft devkit is unpinned."""
    from . import boxes
    found, probs, labels = _detect(samples, level5Data, model, dataDir, maxBoxes, overlapThresh)
    return boxes.average_precision(found, probs, labels, iou_thresholds=iou_thresholds, mode=mode)


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
