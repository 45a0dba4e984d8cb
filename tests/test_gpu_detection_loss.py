"""The VoxelNet detection loss on the GPU: lisec_detection_loss / lisec_detection_loss_eval (csrc/detection_loss.hip)
through the C ABI against the fp64 definition of tests/detection_loss_ref.py.

Tolerances.  The kernels evaluate every element in double from the fp32 inputs and round once, and the sums are fp64 over
at most 320 000 non-negative terms (relative error ~1e-13): what is left is the fp32 rounding of an fp64 value, 2^-24 =
6e-8 relative, so rtol 1e-6 with atol 0 against the oracle.  Where the oracle's fp64 value lies below the fp32 normal range
(|v| < 2^-126: a focal gradient at a logit of 80, say) fp32 cannot hold it to 1e-6; there the kernel's value is compared,
with the same rtol, to the oracle's value rounded to fp32 -- the nearest denormal, or zero."""
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

import detection_loss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# one workgroup holds 16 cells (256 threads / 16 lanes); the grid of 1024 workgroups holds 16384 cells, beyond which the
# grid-stride loop takes a second trip
SIZES = [1, 3, 15, 16, 17, 255, 256, 257, 16383, 16384, 16385, 20000]
PATTERNS = ["ignored", "negatives", "positives", "last_positive", "mix"]
SPECIAL_LOGITS = np.float32([0.0, 80.0, -80.0, 1e4, -1e4])
TINY = float(np.finfo(np.float32).tiny)
EINVAL = -1


def _labels(pattern, M, rng):
    if pattern == "ignored":
        return np.zeros((M, 2), np.float32)
    if pattern == "negatives":
        return np.ones((M, 2), np.float32)
    if pattern == "positives":
        return np.full((M, 2), 2.0, np.float32)
    if pattern == "last_positive":
        y = rng.choice(np.float32([0, 1]), (M, 2))
        y[-1, 1] = 2.0
        return y
    return rng.choice(np.float32([0, 1, 2]), (M, 2), p=[0.49, 0.5, 0.01])       # about 1 % positives


def _case(pattern, M, b, seed):
    """head, y_cls, y_reg (float32).  The special logits land on every kind of anchor (each value on both anchors, every
    13 / 11 cells and in the last cell); the regression residuals d are normal with deviation 1.5 b -- both sides of
    |d| = b -- and the targets carry the +1 of the reference on every cell (only positives are looked at)."""
    rng = np.random.default_rng(seed)
    head = rng.normal(0, 1.5, (M, 16)).astype(np.float32)
    for k, z in enumerate(SPECIAL_LOGITS):
        head[k::13, 0] = z
        head[(k + 2)::11, 1] = z
    head[-1, 1] = SPECIAL_LOGITS[(seed + M) % 5]
    y_cls = _labels(pattern, M, rng)
    d = rng.normal(0, 1.5 * b, (M, 14))
    y_reg = (head[:, 2:].astype(np.float64) - d + 1.0).astype(np.float32)
    return head, y_cls, y_reg


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in arrays]


def _run(spec, d_head, d_yc, d_yr, M, grad_scale):
    """One training call: (dhead, loss_out, counts) on the host; dhead starts as NaN, so every element must be written."""
    import torch
    from lisec_amd import ops
    dev = d_head.device
    dhead = torch.full((M, 16), float("nan"), dtype=torch.float32, device=dev)
    loss_out = torch.full((3,), float("nan"), dtype=torch.float32, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int64, device=dev)
    ops.detection_loss(spec.descriptor(), d_head, d_yc, d_yr, M, dhead, loss_out, counts, grad_scale=grad_scale)
    torch.cuda.synchronize()
    return dhead.cpu().numpy(), loss_out.cpu().numpy(), counts.cpu().numpy()


def _close(got, ref):
    """rtol 1e-6, atol 0 against the fp64 oracle; against its fp32 rounding where fp32 has no normal number for it."""
    ref = np.asarray(ref, np.float64)
    want = np.where(np.abs(ref) >= TINY, ref, ref.astype(np.float32).astype(np.float64))
    np.testing.assert_allclose(np.asarray(got, np.float64), want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_abi_vs_fp64_oracle(pattern, M):
    import torch
    from lisec_amd import losses as K
    from lisec_amd import ops
    for gamma, b in ((0.0, 1.0), (2.0, 1.0 / 9.0), (0.0, 1.0 / 9.0), (2.0, 1.0)):
        params = dict(alpha=1.5 if gamma == 0 else 0.5, beta=1.0 if gamma == 0 else 1.5, gamma=gamma, smooth_l1_beta=b)
        spec, _ = K.compile_loss(K.VoxelNetLoss(**params), loss_weights=[2.0, 0.5])
        head, y_cls, y_reg = _case(pattern, M, b, seed=M + len(pattern))
        dev_in = _dev(head, y_cls, y_reg)
        dhead, loss_out, counts = _run(spec, *dev_in, M, grad_scale=0.75)
        r_loss, r_counts, r_grad = R.detection_loss(head, y_cls, y_reg, weights=(2.0, 0.5), grad_scale=0.75, **params)
        assert np.array_equal(counts, r_counts)
        assert np.isfinite(loss_out).all() and np.isfinite(dhead).all()
        _close(loss_out, r_loss)
        _close(dhead, r_grad)
        # bitwise +0.0 on ignored anchors and on every regression channel of an anchor that is not positive
        pos, neg = R.masks(y_cls)
        bits = dhead.view(np.uint32)
        assert not bits[:, :2][~(pos | neg)].any()
        assert not bits[:, 2:].reshape(M, 2, 7)[~pos].any()
        if pattern == "ignored":
            assert not loss_out.view(np.uint32).any() and not bits.any() and counts.tolist() == [0, 0]
        if pattern == "last_positive":
            assert counts[0] == 1 and np.abs(dhead[-1, 9:]).max() > 0
        # the same bits on a second run
        dhead2, loss2, counts2 = _run(spec, *dev_in, M, grad_scale=0.75)
        assert np.array_equal(dhead.view(np.uint32), dhead2.view(np.uint32))
        assert np.array_equal(loss_out.view(np.uint32), loss2.view(np.uint32)) and np.array_equal(counts, counts2)
        # the evaluation entry adds exactly the training entry's fp32 values and counts the sweep
        acc = torch.zeros(4, dtype=torch.float64, device="cuda")
        ops.detection_loss_eval(spec.descriptor(), *dev_in, M, acc)
        ops.detection_loss_eval(spec.descriptor(), *dev_in, M, acc)
        torch.cuda.synchronize()
        acc = acc.cpu().numpy()
        vals = loss_out.astype(np.float64)
        assert np.array_equal(acc[:3], vals + vals) and acc[3] == 2.0


def test_unit_weights_defaults_and_grad_scale():
    """The defaults of VoxelNetLoss() as 'voxelnet' compiles them; grad_scale scales the gradient and nothing else."""
    from lisec_amd import losses as K
    M = 300
    head, y_cls, y_reg = _case("mix", M, 1.0, seed=11)
    y_cls[:40] = 2.0
    spec, _ = K.compile_loss("voxelnet")
    dev_in = _dev(head, y_cls, y_reg)
    dhead, loss_out, counts = _run(spec, *dev_in, M, grad_scale=1.0)
    r_loss, r_counts, r_grad = R.detection_loss(head, y_cls, y_reg)
    assert np.array_equal(counts, r_counts) and counts[0] >= 80
    _close(loss_out, r_loss)
    _close(dhead, r_grad)
    half, loss_half, _ = _run(spec, *dev_in, M, grad_scale=0.5)
    assert np.array_equal(loss_half, loss_out) and np.array_equal(half, np.float32(0.5) * dhead)


def test_a_nan_logit_is_copied_through():
    """A NaN logit on a looked-at anchor is a NaN loss and a NaN gradient there and nowhere else; on an ignored anchor it
    is not looked at."""
    from lisec_amd import losses as K
    M = 40
    head, y_cls, y_reg = _case("mix", M, 1.0, seed=2)
    y_cls[:] = 1.0
    y_cls[5, 0], y_cls[7, 1], y_cls[9, 0] = 2.0, 1.0, 0.0
    for gamma in (0.0, 2.0):
        spec, _ = K.compile_loss(K.VoxelNetLoss(gamma=gamma))
        h = head.copy()
        h[9, 0] = np.nan                                       # ignored
        dhead, loss_out, _ = _run(spec, *_dev(h, y_cls, y_reg), M, 1.0)
        assert np.isfinite(loss_out).all() and np.isfinite(dhead).all() and dhead[9, 0] == 0
        for cell, col in ((5, 0), (7, 1)):
            h = head.copy()
            h[cell, col] = np.nan
            dhead, loss_out, _ = _run(spec, *_dev(h, y_cls, y_reg), M, 1.0)
            assert np.isnan(loss_out[0]) and np.isnan(loss_out[1]) and np.isfinite(loss_out[2])
            nan = np.isnan(dhead)
            assert nan[cell, col] and nan.sum() == 1


def test_refusals_of_the_abi():
    """Every LISEC_EINVAL of the two entries, each with a text in lisec_last_error; nothing is launched."""
    import torch
    from lisec_amd import _lib
    from lisec_amd import losses as K
    lib = _lib.load()
    M = 64
    head, y_cls, y_reg = _case("mix", M, 1.0, seed=1)
    d_head, d_yc, d_yr = _dev(head, y_cls, y_reg)
    dhead = torch.zeros_like(d_head)
    lo = torch.zeros(3, dtype=torch.float32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    need = lib.lisec_detection_loss_workspace_bytes()
    assert need >= 2 * 8 + 3 * 8 and need % 256 == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    good = K.compile_loss("voxelnet")[0].descriptor()
    st = _lib.current_stream()

    def train(cfg=good, head=d_head, yc=d_yc, yr=d_yr, M=M, dhead=dhead, lo=lo, counts=counts, ws=ws, nbytes=need):
        cfg = ctypes.byref(cfg) if cfg is not None else None
        return lib.lisec_detection_loss(cfg, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M, 1.0, _lib.ptr(dhead),
                                        _lib.ptr(lo), _lib.ptr(counts), _lib.ptr(ws), nbytes, st)

    def evaluate(cfg=good, head=d_head, yc=d_yc, yr=d_yr, M=M, acc=acc, ws=ws, nbytes=need):
        cfg = ctypes.byref(cfg) if cfg is not None else None
        return lib.lisec_detection_loss_eval(cfg, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M, _lib.ptr(acc),
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
    for field, value in (("alpha", -1.0), ("beta", -0.25), ("gamma", -2.0), ("smooth_l1_beta", 0.0),
                         ("smooth_l1_beta", -1.0), ("struct_bytes", 32), ("struct_bytes", 0)):
        bad = K.compile_loss("voxelnet")[0].descriptor()
        setattr(bad, field, value)
        refused(train(cfg=bad))
        refused(evaluate(cfg=bad))
    refused(train(nbytes=need - 1))
    refused(evaluate(nbytes=need - 1))
    refused(train(nbytes=0))
    torch.cuda.synchronize()
    assert lib.lisec_abi_version() == 14
