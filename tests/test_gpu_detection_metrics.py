"""The detection metrics on the GPU: lisec_detection_metrics (csrc/detection_metrics.hip) through lisec_amd.ops against the
fp64 definitions of tests/detection_metrics_ref.py.

Partition.  One thread per anchor, 256 threads per workgroup, 1024 workgroups at most: one workgroup holds 128 cells (256
anchors) and one full grid 131 072 cells, beyond which the grid-stride loop takes a second trip.  SIZES lie either side of
both, plus 20 000 cells, the Lyft grid.

Tolerances.
  counts   (numerators and denominators of precision / recall / accuracy, every denominator) are exact integers held in
           doubles: ==.  That needs every decision p > threshold to be the reference's: the test asserts on the CPU that no
           looked-at anchor has |p - threshold| < 1e-6 -- except the planted logit 0 at threshold 0.5, where p = 1 / (1 + 1) is
           exactly 0.5 in any IEEE arithmetic (exp(-0) = 1), equals the threshold, and is "not predicted" on both sides.
  MAE num  rtol 1e-10: an fp64 sum of at most 2.8e6 non-negative terms in another order, n 2^-53 ~ 3e-10 at the very worst
           and ~sqrt(n) 2^-53 typically.
  IoU num  atol 1e-9 max(N_pos, 1): the per-pair bound tests/test_gpu_detection_ap.py holds pair_iou to against the same
           reference."""
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

import detection_metrics_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 127, 128, 129, 131071, 131072, 131073, 20000]
PATTERNS = ["ignored", "negatives", "positives", "last_positive", "mix"]
CASES = [(p, M) for M in SIZES for p in PATTERNS if p != "positives" or M <= 129]     # all-positive: small M (the IoU work)
SPECIAL_LOGITS = np.float32([0.0, 80.0, -80.0, 1e4, -1e4, np.nan])
EINVAL = -1
# (default name, threshold, mode): all eight slots, every kind, the three thresholds, both modes
EIGHT = [("anchor_precision", 0.3, None), ("anchor_recall", 0.5, None), ("anchor_accuracy", 0.7, None),
         ("positive_mae", None, None), ("positive_iou", None, "bev"), ("positive_iou", None, "3d"),
         ("anchor_precision", 0.5, None), ("anchor_accuracy", 0.3, None)]
COUNT_KINDS = ("anchor_precision", "anchor_recall", "anchor_accuracy")


def _metric(k, name, threshold, mode):
    from lisec_amd import metrics as Mx
    cls = Mx.DETECTION_FUNCTIONS[name]
    if threshold is not None:
        return cls(threshold, name=f"m{k}")
    return cls(mode, name=f"m{k}") if mode is not None else cls(name=f"m{k}")


def _spec(terms, target_offset=1.0):
    """The DetectionLossSpec of the metrics (name, threshold, mode) in the order given: the class output's come first in
    terms, as compile() orders them."""
    from lisec_amd import losses as K
    spec, names = K.compile_loss(K.VoxelNetLoss(target_offset=target_offset),
                                 metrics=[_metric(k, *t) for k, t in enumerate(terms)])
    order = [int(n.rsplit("_m", 1)[1]) for n in names]
    return spec, [terms[k] for k in order]


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


def _inputs(pattern, M, seed):
    rng = np.random.default_rng(seed)
    head = rng.normal(0, 1.5, (M, 16)).astype(np.float32)
    for k, z in enumerate(SPECIAL_LOGITS):                         # each special logit on both anchors, and in the last cell
        head[k::13, 0] = z
        head[(k + 2)::11, 1] = z
    head[-1, 1] = SPECIAL_LOGITS[(seed + M) % len(SPECIAL_LOGITS)]
    y_cls = _labels(pattern, M, rng)
    d = rng.normal(0, 0.3, (M, 14))                                # r - t: IoUs spread over (0, 1)
    y_reg = (head[:, 2:].astype(np.float64) - d + 1.0).astype(np.float32)
    head[3::17, 5] = 1000.0                                        # r3 of anchor 0: exp overflows, IoU 0, still counted
    head[-1, 12] = 1000.0                                          # and of the last anchor
    return head, y_cls, y_reg


def _margin_ok(head, y_cls):
    """No looked-at anchor within 1e-6 of a threshold, but for p == 0.5 exactly at a logit of exactly 0 (see the top)."""
    pos, neg = R.masks(y_cls)
    z = head[:, :2].astype(np.float64)[pos | neg]
    p = R.sigmoid(z[~np.isnan(z)])
    z = z[~np.isnan(z)]
    for thr in (0.3, 0.5, 0.7):
        near = np.abs(p - thr) < 1e-6
        if thr == 0.5:
            near &= ~((z == 0.0) & (p == 0.5))
        if near.any():
            return False
    return True


def _case(pattern, M):
    """Inputs whose decisions cannot flip: the seed is drawn again until the reference alone satisfies the margin."""
    for seed in range(M + len(pattern), M + len(pattern) + 50):
        head, y_cls, y_reg = _inputs(pattern, M, seed)
        if _margin_ok(head, y_cls):
            return head, y_cls, y_reg
    raise AssertionError("no seed keeps every sigmoid 1e-6 away from the thresholds")


def _reference(terms, head, y_cls, y_reg, target_offset=1.0):
    """[(num, den)] in the order of terms; the IoUs of a mode are computed once."""
    iou = {}
    out = []
    for name, threshold, mode in terms:
        if name == "positive_iou":
            if mode not in iou:
                iou[mode] = R.positive_iou(head, y_cls, y_reg, mode, target_offset)
            out.append(iou[mode])
        else:
            out.append(R.pair(name, head, y_cls, y_reg, threshold=threshold, target_offset=target_offset))
    return out


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in arrays]


def _run(spec, dev_in, M, out=None, accumulate=False):
    """One call; out starts as NaN (every slot must be written) unless given."""
    import torch
    from lisec_amd import ops
    if out is None:
        out = torch.full((2 * spec.n_metrics,), float("nan"), dtype=torch.float64, device="cuda")
    ops.detection_metrics(spec.metrics_descriptor(), *dev_in, M, out, accumulate=accumulate)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(terms, got, ref):
    n_pos = None
    for k, ((name, _, _), (num, den)) in enumerate(zip(terms, ref)):
        g_num, g_den = got[2 * k], got[2 * k + 1]
        assert g_den == den, (name, k)
        if name in COUNT_KINDS:
            assert g_num == num, (name, k)
        elif name == "positive_mae":
            np.testing.assert_allclose(g_num, num, rtol=1e-10, atol=0)
        else:
            n_pos = den
            assert abs(g_num - num) <= 1e-9 * max(den, 1.0), (name, k, g_num, num)
    return n_pos


@pytest.mark.parametrize("pattern,M", CASES)
def test_abi_vs_fp64_oracle(pattern, M):
    import torch
    head, y_cls, y_reg = _case(pattern, M)
    assert _margin_ok(head, y_cls)
    spec, terms = _spec(EIGHT)
    assert spec.n_metrics == 8
    dev_in = _dev(head, y_cls, y_reg)
    got = _run(spec, dev_in, M)                                    # accumulate=0 over NaN: every slot overwritten
    assert np.isfinite(got).all()
    ref = _reference(terms, head, y_cls, y_reg)
    n_pos = _check(terms, got, ref)
    pos, neg = R.masks(y_cls)
    assert n_pos == pos.sum()
    if pattern == "ignored":
        assert not got.any()
    if pattern == "last_positive":
        assert n_pos == 1
    if n_pos >= 20:
        assert 0 < got[2 * terms.index(EIGHT[4])] < n_pos          # IoUs inside (0, 1), and the planted zeros
    # the same call twice: the same bits
    assert np.array_equal(got.view(np.uint64), _run(spec, dev_in, M).view(np.uint64))
    # accumulate twice from zero: twice the stored value, counts to the bit, sums to the last ulp
    acc = torch.zeros(16, dtype=torch.float64, device="cuda")
    _run(spec, dev_in, M, out=acc, accumulate=True)
    twice = _run(spec, dev_in, M, out=acc, accumulate=True)
    for k, (name, _, _) in enumerate(terms):
        assert twice[2 * k + 1] == 2 * got[2 * k + 1]
        if name in COUNT_KINDS:
            assert twice[2 * k] == 2 * got[2 * k]
        else:
            assert abs(twice[2 * k] - 2 * got[2 * k]) <= np.spacing(2 * got[2 * k])
    # fewer metrics, another target_offset: slots beyond 2 n stay untouched
    few, few_terms = _spec([EIGHT[5], EIGHT[3], EIGHT[1]], target_offset=0.75)
    out = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    got3 = _run(few, dev_in, M, out=out)
    assert np.isnan(got3[6:]).all()
    _check(few_terms, got3[:6], _reference(few_terms, head, y_cls, y_reg, target_offset=0.75))


def test_one_metric_at_a_time_equals_its_slot_among_eight():
    """Each kind alone (n_metrics == 1) gives the bits it gives as one of eight: the slots do not interact."""
    M = 300
    head, y_cls, y_reg = _case("mix", M)
    y_cls[:40] = 2.0
    assert _margin_ok(head, y_cls)
    dev_in = _dev(head, y_cls, y_reg)
    spec, terms = _spec(EIGHT)
    all8 = _run(spec, dev_in, M)
    _check(terms, all8, _reference(terms, head, y_cls, y_reg))
    for k, t in enumerate(terms):
        one, _ = _spec([t])
        assert np.array_equal(_run(one, dev_in, M).view(np.uint64), all8[2 * k:2 * k + 2].view(np.uint64)), t


def test_nan_codes_and_nan_logits():
    M = 130
    head, y_cls, y_reg = _case("mix", M)
    y_cls[::3, 0] = np.nan                                         # ignored, whatever the logit
    y_cls[1::3, 1] = 2.0
    head[1::6, 1] = np.nan                                         # positives with a NaN logit: missed
    head[2::6, 0] = np.nan                                         # whatever they are: predicted negative
    assert _margin_ok(head, y_cls)
    spec, terms = _spec(EIGHT)
    got = _run(spec, _dev(head, y_cls, y_reg), M)
    assert np.isfinite(got).all()
    _check(terms, got, _reference(terms, head, y_cls, y_reg))


def test_refusals_of_the_abi():
    """Every LISEC_EINVAL, each with a text in lisec_last_error; nothing is launched and out is untouched."""
    import torch
    from lisec_amd import _lib
    lib = _lib.load()
    M = 64
    head, y_cls, y_reg = _case("mix", M)
    d_head, d_yc, d_yr = _dev(head, y_cls, y_reg)
    need = lib.lisec_detection_metrics_workspace_bytes()
    assert need >= 16 * 8 and need % 256 == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    sentinel = -12345.0
    out = torch.full((16,), sentinel, dtype=torch.float64, device="cuda")
    spec, _ = _spec(EIGHT)
    st = _lib.current_stream()

    def call(cfg="good", head=d_head, yc=d_yc, yr=d_yr, M=M, out=out, accumulate=0, ws=ws, nbytes=need):
        cfg = spec.metrics_descriptor() if isinstance(cfg, str) else cfg
        cfg = ctypes.byref(cfg) if cfg is not None else None
        return lib.lisec_detection_metrics(cfg, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M, _lib.ptr(out), accumulate,
                                           _lib.ptr(ws), nbytes, st)

    def refused(rc):
        assert rc == EINVAL and lib.lisec_last_error().decode().strip()

    for name in ("cfg", "head", "yc", "yr", "out", "ws"):
        refused(call(**{name: None}))
    for m in (0, -5):
        refused(call(M=m))
    for field, value in (("struct_bytes", 0), ("struct_bytes", 64), ("n_metrics", 0), ("n_metrics", 9), ("n_metrics", -1)):
        bad = spec.metrics_descriptor()
        setattr(bad, field, value)
        refused(call(cfg=bad))
    # the slots in compile order: five threshold metrics, the MAE, the two IoUs
    for slot, field, value in ((0, "kind", 5), (0, "kind", -1), (7, "kind", 99), (6, "mode", 2), (7, "mode", -1),
                               (0, "threshold", 0.0), (1, "threshold", 1.0), (2, "threshold", -0.5), (3, "threshold", 1.5),
                               (4, "threshold", float("nan"))):
        bad = spec.metrics_descriptor()
        kinds = [bad.metric[k].kind for k in range(8)]
        assert (field != "mode" or kinds[slot] == 4) and (field != "threshold" or kinds[slot] < 3)
        setattr(bad.metric[slot], field, value)
        refused(call(cfg=bad))
        refused(call(cfg=bad, accumulate=1))
    refused(call(nbytes=need - 1))
    refused(call(nbytes=0))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == sentinel).all()
    # a slot beyond n_metrics is not looked at
    three, _ = _spec(EIGHT[:3])
    cfg = three.metrics_descriptor()
    cfg.metric[3].kind = 99
    assert call(cfg=cfg) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[6:] == sentinel).all() and (got[:6] != sentinel).all()
