"""The reference's post-processing script under its own name: anchor decode + rotated NMS of one sample's RPN maps
(rpnToRegion.py:18-164) and the score of a set of detections against the sample's annotations (:202-255), on the GPU
(lisec_amd.boxes).  The reference reads the Lyft dataset from a module global `level5Data` that its __main__ block fills;
calcIoUAll takes it as an optional last argument and falls back to the module global of the same name."""
import numpy as np

from .boxes import annotationBoxes, average_precision, calcIntersectAll, calcIoUAll_boxes, calcUnionAll   # noqa: F401
from .boxes import evaluate_by_range, evaluate_detections, points_in_boxes                                # noqa: F401
from .boxes import rpnToRegion as _rpn_to_region

level5Data = None            # rpnToRegion.py:265-269 builds a LyftDataset here


def rpnToRegion(labelsClass, labelsRegress):
    """rpnToRegion(labelsClass (100,200,2), labelsRegress (100,200,14)) (rpnToRegion.py:116-164) with the reference's
    fixed maxBoxes=20, overlapThresh=0.; returns what nonMaxSuppressionFast returns there: (boxes (k,7), probs (k,)),
    boxes = x, y, z, l, w, h, yaw.  A leading sample axis of length 1 (predictMain's files) is accepted."""
    cls, reg = np.asarray(labelsClass), np.asarray(labelsRegress)
    if cls.ndim == 4:
        cls, reg = cls[0], reg[0]
    return _rpn_to_region(cls, reg, maxBoxes=20, overlapThresh=0.)


def calcIoUAll(predictBoxes, sample, dataset=None):
    """calcIoUAll(predictBoxes, sample) (rpnToRegion.py:224-255): the sample's car annotations within +-50 m in ego
    coordinates, then calcIntersectAll / calcUnionAll.  predictBoxes are ego-centred (the -50 m shift of :279-280 done)."""
    ds = dataset if dataset is not None else level5Data
    if ds is None:
        raise RuntimeError("set lisec_amd.rpnToRegion.level5Data (or pass the dataset) first")
    return calcIoUAll_boxes(predictBoxes, annotationBoxes(sample, ds))
