"""The detection loss with the IoU term on the GPU: lisec_detection_iou_loss / lisec_detection_iou_loss_eval
(csrc/detection_iou_loss.hip) through the C ABI against the fp64 definition of tests/detection_iou_loss_ref.py, on the
cases of tests/detection_iou_cases.py.

Tolerances.  Values: the fp32 rounding of an fp64 value, rtol 1e-6 (tests/test_gpu_detection_loss.py).  Gradient: the
class channels, every anchor that is not positive and every channel the IoU term does not reach are compared BIT FOR BIT
with lisec_detection_loss on the same inputs.  The regression channels of a positive are compared with the SmoothL1
derivative in closed form plus CENTRAL DIFFERENCES (h = 1e-6) of the reference IoU: |got - ref| <= 1e-6 max_k |ref_k| over
the anchor's seven channels -- the difference quotient is within 5.2e-8 of the derivative wherever the IoU has one, the
fp32 rounding adds 6e-8, and tests/test_detection_iou_loss_oracle.py asserts on the reference alone that every positive of
every case is such a point (two difference steps agree to 1e-6)."""
import ctypes
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
import detection_iou_loss_ref as R  # noqa: E402
from detection_loss_ref import masks  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1


def _specs(combo, iou_weight=None):
    """(the DetectionIoULossSpec of the combo, the DetectionLossSpec of the same VoxelNetLoss parameters)."""
    from lisec_amd import losses as K
    det, iou = C.params(combo)
    if iou_weight is not None:
        iou = dict(iou, iou_weight=iou_weight)
    return (K.compile_loss(K.VoxelNetIoULoss(**det, **iou), loss_weights=list(C.WEIGHTS))[0],
            K.compile_loss(K.VoxelNetLoss(**det), loss_weights=list(C.WEIGHTS))[0])


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in arrays]


def _run(spec, d_head, d_yc, d_yr, M, grad_scale=C.GRAD_SCALE):
    """One training call of the entry the spec belongs to: (dhead, loss_out, counts) on the host; dhead starts as NaN, so
    every element must be written."""
    import torch
    from lisec_amd import losses as K
    from lisec_amd import ops
    dhead = torch.full((M, 16), float("nan"), dtype=torch.float32, device="cuda")
    loss_out = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    run = ops.detection_iou_loss if isinstance(spec, K.DetectionIoULossSpec) else ops.detection_loss
    run(spec.descriptor(), d_head, d_yc, d_yr, M, dhead, loss_out, counts, grad_scale=grad_scale)
    torch.cuda.synchronize()
    return dhead.cpu().numpy(), loss_out.cpu().numpy(), counts.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_case(pattern, M, combo):
    import torch
    from lisec_amd import ops
    head, y_cls, y_reg = C.case(pattern, M, combo)
    det, iou = C.params(combo)
    spec, plain = _specs(combo)
    dev_in = _dev(head, y_cls, y_reg)
    dhead, loss_out, counts = _run(spec, *dev_in, M)
    base, base_loss, base_counts = _run(plain, *dev_in, M)
    r_loss, r_counts, r_grad = R.detection_iou_loss(head, y_cls, y_reg, weights=C.WEIGHTS, grad_scale=C.GRAD_SCALE,
                                                    **det, **iou)
    assert np.array_equal(counts, r_counts) and np.array_equal(counts, base_counts) and counts[0] > 0
    assert np.isfinite(loss_out).all() and np.isfinite(dhead).all()
    print(pattern, M, C.COMBOS[combo], "loss", loss_out, "ref", r_loss)
    np.testing.assert_allclose(loss_out.astype(np.float64), r_loss, rtol=1e-6, atol=0)
    assert _bits(loss_out)[1] == _bits(base_loss)[1]
    # the class channels: lisec_detection_loss's bits
    assert np.array_equal(_bits(dhead[:, :2]), _bits(base[:, :2]))
    pos, _ = masks(y_cls)
    got = dhead[:, 2:].reshape(M, 2, 7)
    # bitwise +0.0 on every regression channel of an anchor that is not positive
    assert not _bits(got)[~pos].any()
    # the positives, anchor by anchor
    g, ref = got[pos].astype(np.float64), r_grad[:, 2:].reshape(M, 2, 7)[pos]
    err = np.abs(g - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print("  positives", len(g), "worst |got - ref| / max_k |ref_k|", err.max())
    assert err.max() <= 1e-6, (int(err.argmax()), float(err.max()))
    plain_reg = base[:, 2:].reshape(M, 2, 7)[pos]
    moved = _bits(got[pos]) != _bits(plain_reg)
    ious = R.decoded_iou(*R.positives(head, y_cls, y_reg)[2:], iou["iou_mode"])
    # no overlap: exactly +0.0 from the term, so the anchor keeps lisec_detection_loss's bits; under 'bev' r2 and r5 always
    assert not moved[ious == 0].any()
    if iou["iou_mode"] == "bev":
        assert not moved[:, [2, 5]].any()
    if (ious > 0).any():
        assert moved[ious > 0].any()
    # the same bits on a second run
    dhead2, loss2, counts2 = _run(spec, *dev_in, M)
    assert np.array_equal(_bits(dhead), _bits(dhead2)) and np.array_equal(_bits(loss_out), _bits(loss2))
    assert np.array_equal(counts, counts2)
    # the evaluation entry adds exactly the training entry's fp32 values and counts the sweep
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.detection_iou_loss_eval(spec.descriptor(), *dev_in, M, acc)
    ops.detection_iou_loss_eval(spec.descriptor(), *dev_in, M, acc)
    torch.cuda.synchronize()
    acc = acc.cpu().numpy()
    vals = loss_out.astype(np.float64)
    assert np.array_equal(acc[:3], vals + vals) and acc[3] == 2.0


@pytest.mark.parametrize("M", C.SIZES)
@pytest.mark.parametrize("pattern", C.PATTERNS)
def test_abi_vs_fp64_reference(pattern, M):
    for combo in C.combos(pattern, M):
        _check_case(pattern, M, combo)


@pytest.mark.parametrize("combo", [1, 3])
def test_second_trip_of_the_anchor_pass(combo):
    """131072 + 37 cells: 1024 workgroups of 256 anchors take a second trip beyond cell 131072; positives on cell 0, on
    both sides of that border and on the last cell."""
    head, y_cls, _ = C.case("stride", C.STRIDE_M, combo)
    assert (y_cls[[0, 131071, 131072, 131073, C.STRIDE_M - 1]] == 2).any(axis=1).all() and (y_cls == 2).sum() == 64
    _check_case("stride", C.STRIDE_M, combo)


@pytest.mark.parametrize("pattern,M", [("positives", 17), ("mix", 257), ("positives", 257), ("mix", 16385),
                                       ("stride", C.STRIDE_M)])
def test_iou_weight_zero_is_the_detection_loss_bit_for_bit(pattern, M):
    for combo in (1, 3):
        spec, plain = _specs(combo, iou_weight=0.0)
        dev_in = _dev(*C.case(pattern, M, combo))
        got, want = _run(spec, *dev_in, M), _run(plain, *dev_in, M)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
        assert np.array_equal(got[2], want[2])


@pytest.mark.parametrize("combo", [0, 3])
def test_disjoint_positives_keep_the_detection_gradient(combo):
    """r0 moved 10 anchor lengths away: no pair overlaps, the gradient is lisec_detection_loss's and L_reg exceeds its by
    iou_weight."""
    M = 257
    head, y_cls, y_reg = (a.copy() for a in C.case("positives", M, combo))
    head[:, [2, 9]] += 10.0
    det, iou = C.params(combo)
    assert not R.decoded_iou(*R.positives(head, y_cls, y_reg)[2:], iou["iou_mode"]).any()
    spec, plain = _specs(combo)
    dev_in = _dev(head, y_cls, y_reg)
    dhead, loss_out, _ = _run(spec, *dev_in, M)
    base, base_loss, _ = _run(plain, *dev_in, M)
    assert np.array_equal(_bits(dhead), _bits(base))
    print("L_reg", loss_out[2], "plain", base_loss[2])
    assert abs(float(loss_out[2]) - float(base_loss[2]) - iou["iou_weight"]) <= 1e-6 * float(loss_out[2])


@pytest.mark.parametrize("mode", ["bev", "3d"])
def test_coincident_boxes(mode):
    """r == t on every positive (residuals on a grid of 1/64, exact in fp32 with and without the +1): IoU 1, so L_reg is
    the SmoothL1 value 0; the gradient is some one-sided derivative, finite."""
    from lisec_amd import losses as K
    M = 257
    rng = np.random.default_rng(3)
    t = rng.integers(-48, 49, (M, 14)) / 64.0
    head = np.concatenate([rng.normal(0, 1.5, (M, 2)), t], axis=1).astype(np.float32)
    y_cls = np.full((M, 2), 2.0, np.float32)
    y_reg = (t + 1.0).astype(np.float32)
    assert np.array_equal(head[:, 2:].astype(np.float64), y_reg.astype(np.float64) - 1.0)
    spec, _ = K.compile_loss(K.VoxelNetIoULoss(iou_weight=2.0, iou_mode=mode))
    dhead, loss_out, counts = _run(spec, *_dev(head, y_cls, y_reg), M, grad_scale=1.0)
    print("L_reg", loss_out[2])
    assert counts[0] == 2 * M and np.isfinite(dhead).all() and np.isfinite(loss_out).all()
    assert abs(float(loss_out[2])) <= 1e-6


@pytest.mark.parametrize("mode", ["bev", "3d"])
def test_an_overflowing_extent_has_no_iou_gradient(mode):
    """r3 = 800: exp overflows, the decoded box is not finite -- IoU 0 as the metric has it; loss and gradient finite, the
    anchor keeps lisec_detection_loss's bits and the others their IoU part."""
    combo = 0 if mode == "bev" else 3
    M = 17
    head, y_cls, y_reg = (a.copy() for a in C.case("positives", M, combo))
    head[3, 2 + 3], head[11, 9 + 3] = 800.0, 800.0
    det, iou = C.params(combo)
    spec, plain = _specs(combo)
    dev_in = _dev(head, y_cls, y_reg)
    dhead, loss_out, _ = _run(spec, *dev_in, M)
    base, _, _ = _run(plain, *dev_in, M)
    assert np.isfinite(dhead).all() and np.isfinite(loss_out).all()
    assert np.array_equal(_bits(dhead[3, 2:9]), _bits(base[3, 2:9]))
    assert np.array_equal(_bits(dhead[11, 9:]), _bits(base[11, 9:]))
    assert (_bits(dhead) != _bits(base)).sum() > 7
    r_loss = R.detection_iou_loss(head, y_cls, y_reg, weights=C.WEIGHTS, **det, **iou)[0]
    np.testing.assert_allclose(loss_out.astype(np.float64), r_loss, rtol=1e-6, atol=0)


def test_refusals_of_the_abi():
    """Every LISEC_EINVAL of the two entries, each with a text in lisec_last_error; nothing is launched."""
    import torch
    from lisec_amd import _lib
    from lisec_amd import losses as K
    lib = _lib.load()
    M = 64
    d_head, d_yc, d_yr = _dev(*C.build("mix", M, 1, seed=1))
    dhead = torch.zeros_like(d_head)
    lo = torch.zeros(3, dtype=torch.float32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    need = lib.lisec_detection_iou_loss_workspace_bytes()
    assert need >= 2 * 8 + 3 * 8 and need % 256 == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    good = K.compile_loss("voxelnet_iou")[0].descriptor()
    st = _lib.current_stream()

    def train(cfg=good, head=d_head, yc=d_yc, yr=d_yr, M=M, dhead=dhead, lo=lo, counts=counts, ws=ws, nbytes=need):
        cfg = ctypes.byref(cfg) if cfg is not None else None
        return lib.lisec_detection_iou_loss(cfg, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M, 1.0, _lib.ptr(dhead),
                                            _lib.ptr(lo), _lib.ptr(counts), _lib.ptr(ws), nbytes, st)

    def evaluate(cfg=good, head=d_head, yc=d_yc, yr=d_yr, M=M, acc=acc, ws=ws, nbytes=need):
        cfg = ctypes.byref(cfg) if cfg is not None else None
        return lib.lisec_detection_iou_loss_eval(cfg, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M, _lib.ptr(acc),
                                                 _lib.ptr(ws), nbytes, st)

    def refused(rc):
        assert rc == EINVAL and lib.lisec_last_error().decode().strip()

    assert train() == 0 and evaluate() == 0
    for name in ("cfg", "head", "yc", "yr", "dhead", "lo", "counts", "ws"):
        refused(train(**{name: None}))
    for name in ("cfg", "head", "yc", "yr", "acc", "ws"):
        refused(evaluate(**{name: None}))
    for m in (0, -5):
        refused(train(M=m))
        refused(evaluate(M=m))

    def bad_descriptors():
        for field, value in (("struct_bytes", 64), ("struct_bytes", 0), ("iou_weight", -1.0), ("iou_weight", float("nan")),
                             ("iou_weight", float("inf")), ("iou_mode", 2), ("iou_mode", -1)):
            bad = K.compile_loss("voxelnet_iou")[0].descriptor()
            setattr(bad, field, value)
            yield bad
        # the refusals of lisec_detection_loss, on the embedded descriptor
        for field, value in (("alpha", -1.0), ("beta", -0.25), ("gamma", -2.0), ("smooth_l1_beta", 0.0),
                             ("struct_bytes", 32)):
            bad = K.compile_loss("voxelnet_iou")[0].descriptor()
            setattr(bad.det, field, value)
            yield bad
        for a, k, value in ((0, 0, 0.0), (1, 1, -3.9), (0, 2, 0.0), (1, 3, float("nan")), (0, 0, float("inf"))):
            bad = K.compile_loss("voxelnet_iou")[0].descriptor()
            bad.anchors[a][k] = value
            yield bad

    for bad in bad_descriptors():
        refused(train(cfg=bad))
        refused(evaluate(cfg=bad))
    refused(train(nbytes=need - 1))
    refused(evaluate(nbytes=need - 1))
    refused(train(nbytes=0))
    torch.cuda.synchronize()
    assert lib.lisec_abi_version() == 14
