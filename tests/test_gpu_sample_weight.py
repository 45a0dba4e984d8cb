"""Sample weights on the GPU through the C ABI: lisec_head_loss_weighted*, lisec_detection_loss_weighted* and
lisec_detection_iou_loss_weighted* (include/lisec_hip.h, lisec_sample_weights) against the unweighted entries and against
the fp64 definition of tests/sample_weight_ref.py.

Sizes.  k_head_loss and k_det_loss hold 16 cells per workgroup of 256 threads and 16384 cells per trip of their 1024
workgroups: M = 1 (one cell group), 17 (a second workgroup with a 16-lane tail) and 16384 + 3 (a second trip).  k_det_iou
holds 128 cells per workgroup and 131072 per trip: M = 17 and the 131072 + 37 of tests/detection_iou_cases.py.

Tolerances.  Those of tests/test_gpu_losses.py and tests/test_gpu_detection_loss.py for the unweighted entries -- values and
pairs rtol 1e-6 against fp64, dhead within 1e-6 * max|ref| per output: a weight is one more fp32 (or fp64) factor, one more
rounding of 2^-24 at most.  Unit weights and power-of-two maps are exact statements: bits."""
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
import sample_weight_ref as SW  # noqa: E402
from test_gpu_losses import LEGACY_CE, TERMS, _inputs, _spec  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
SIZES = [1, 17, 16384 + 3]
CANARY = 0xA5
TINY = float(np.finfo(np.float32).tiny)
ALL_METRICS = ((0, 1, 2, 3), (0, 1, 2, 3))


def _dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda") for a in arrays]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _maps(kind, M, seed):
    """(w_cls, w_reg) as numpy float32: a 0-d array is the sweep's weight, an (M,) array the map (also at M = 1)."""
    rng = np.random.default_rng(seed)
    if kind == "sweep_one":
        return np.asarray(np.float32(1.0)), np.asarray(np.float32(1.0))
    if kind == "map_ones":
        return np.ones(M, np.float32), np.ones(M, np.float32)
    if kind == "pow2":
        return tuple(rng.choice(np.float32([0.5, 1, 2, 4]), M) for _ in range(2))
    if kind == "random":                                       # [0, 3] with a block of zero-weight cells
        out = []
        for lo in (0, M // 3):
            w = rng.uniform(0, 3, M).astype(np.float32)
            w[lo:lo + max(1, M // 8)] = 0.0
            out.append(w)
        return tuple(out)
    if kind == "mixed":                                        # a sweep weight on one output, nothing on the other
        return np.asarray(np.float32(0.75)), None
    raise ValueError(kind)


class _Workspace:
    """Exactly the bytes the library asks for, in front of canary bytes."""

    def __init__(self, need):
        import torch
        self.need = need
        self.buf = torch.full((need + 256,), CANARY, dtype=torch.uint8, device="cuda")

    def intact(self):
        return bool((self.buf[self.need:] == CANARY).all().item())


def _sw(w, d_w, M, weighted=((), ()), per_cell=None):
    from lisec_amd import ops
    bits = tuple(sum(1 << j for j in ws) for ws in weighted)
    if per_cell is None:
        per_cell = [int(x is not None and np.ndim(x) == 1) for x in w]
    return ops.sample_weights(d_w[0], d_w[1], M, weighted_metrics=bits, per_cell=per_cell)


# ---- the Keras losses ---------------------------------------------------------------------------------------------------
def _head_weighted(spec, dev_in, M, w, weighted=ALL_METRICS, grad_scale=0.75, sweeps=2):
    """(dhead, loss_out, pairs (n,2), acc) of lisec_head_loss_weighted and of `sweeps` lisec_head_loss_weighted_eval."""
    import torch
    from lisec_amd import _lib
    lib = _lib.load()
    d_w = _dev(*w)
    sw = _sw(w, d_w, M, weighted)
    cfg = spec.descriptor()
    n = spec.n_metrics
    dhead = torch.full((M, 16), float("nan"), dtype=torch.float32, device="cuda")
    loss_out = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda")
    pairs = torch.full((2 * n + 2,), float("nan"), dtype=torch.float64, device="cuda")
    acc = torch.zeros(4 + 2 * n + 1, dtype=torch.float64, device="cuda")
    acc[-1] = -7.0
    ws = _Workspace(lib.lisec_head_loss_weighted_workspace_bytes())
    st = _lib.current_stream()
    d_head, d_yc, d_yr = dev_in
    _lib.check(lib.lisec_head_loss_weighted(ctypes.byref(cfg), ctypes.byref(sw), _lib.ptr(d_head), _lib.ptr(d_yc),
                                            _lib.ptr(d_yr), M, grad_scale, _lib.ptr(dhead), _lib.ptr(loss_out),
                                            _lib.ptr(pairs), _lib.ptr(ws.buf), ws.need, st))
    for _ in range(sweeps):
        _lib.check(lib.lisec_head_loss_weighted_eval(ctypes.byref(cfg), ctypes.byref(sw), _lib.ptr(d_head), _lib.ptr(d_yc),
                                                     _lib.ptr(d_yr), M, _lib.ptr(acc), _lib.ptr(ws.buf), ws.need, st))
    torch.cuda.synchronize()
    assert ws.intact()
    lo, pr, ac = loss_out.cpu().numpy(), pairs.cpu().numpy(), acc.cpu().numpy()
    assert np.isnan(lo[3]) and np.isnan(pr[2 * n:]).all() and ac[-1] == -7.0       # nothing behind the outputs is touched
    return dhead.cpu().numpy(), lo[:3], pr[:2 * n].reshape(n, 2), ac[:-1]


def _head_plain(spec, dev_in, M, grad_scale=0.75):
    """(dhead, loss_out, metric_out, acc of two sweeps) of the unweighted entries."""
    import torch
    from lisec_amd import ops
    d_head, d_yc, d_yr = dev_in
    dhead = torch.full((M, 16), float("nan"), dtype=torch.float32, device="cuda")
    loss_out = torch.zeros(3, dtype=torch.float32, device="cuda")
    met = torch.zeros(8, dtype=torch.float32, device="cuda")
    ops.head_loss(spec.descriptor(), d_head, d_yc, d_yr, M, dhead, loss_out, met, grad_scale=grad_scale)
    acc = torch.zeros(4 + spec.n_metrics, dtype=torch.float64, device="cuda")
    for _ in range(2):
        ops.head_loss_eval(spec.descriptor(), d_head, d_yc, d_yr, M, acc)
    torch.cuda.synchronize()
    return dhead.cpu().numpy(), loss_out.cpu().numpy(), met[:spec.n_metrics].cpu().numpy(), acc.cpu().numpy()


def _head_case(name, M):
    terms = LEGACY_CE if name == "legacy_ce" else (TERMS[name], TERMS[name])
    spec = _spec(*terms)
    head, yc, yr, dev_in = _inputs(M, seed=M + len(name), positive=name == "poisson")
    return spec, head, yc, yr, dev_in


def _scaled_exactly(ref_grad, w_rows):
    """The condition of the power-of-two statement, on the reference: every gradient that is not zero is fp32-normal with
    three binades to spare on either side, before and after the factor of at most 4."""
    a = np.abs(ref_grad[ref_grad != 0])
    return a.size == 0 or (a.min() >= 8 * TINY and a.max() * 4 <= float(np.finfo(np.float32).max) / 8)


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", sorted(TERMS) + ["legacy_ce"])
def test_head_loss_weighted(name, M):
    spec, head, yc, yr, dev_in = _head_case(name, M)
    n = spec.n_metrics
    assert n == 8
    plain_g, plain_lo, plain_met, plain_acc = _head_plain(spec, dev_in, M)
    # unit weights, both forms: the unweighted entry's bits; every pair gives the unweighted metric
    for kind in ("sweep_one", "map_ones"):
        g, lo, pairs, acc = _head_weighted(spec, dev_in, M, _maps(kind, M, 0))
        assert np.array_equal(_bits(g), _bits(plain_g)), kind
        assert np.array_equal(_bits(lo), _bits(plain_lo)), kind
        assert np.array_equal(acc[:3], plain_acc[:3]) and acc[3] == 2.0
        np.testing.assert_allclose(pairs[:, 0] / pairs[:, 1], plain_met, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(acc[4:].reshape(n, 2)[:, 0] / acc[4:].reshape(n, 2)[:, 1], plain_met, rtol=1e-6, atol=1e-12)
    # power-of-two maps: dhead is the unweighted dhead times w, exactly
    w = _maps("pow2", M, M)
    _, _, ref_g = SW.head_loss(spec, head, yc, yr, grad_scale=0.75)
    assert _scaled_exactly(ref_g, w)
    g, _, _, _ = _head_weighted(spec, dev_in, M, w)
    rows = np.concatenate([np.repeat(w[0][:, None], 2, 1), np.repeat(w[1][:, None], 14, 1)], 1)
    assert np.array_equal(_bits(g), _bits(plain_g * rows))
    # random weights in [0, 3] with zero-weight blocks, and a sweep weight on one output only
    for kind in ("random", "mixed"):
        w = _maps(kind, M, M + 1)
        r_lo, r_pairs, r_g = SW.head_loss(spec, head, yc, yr, w=w, weighted=ALL_METRICS, grad_scale=0.75)
        assert np.isfinite(r_g).all()
        g, lo, pairs, acc = _head_weighted(spec, dev_in, M, w)
        print(name, M, kind, "loss", lo, "ref", r_lo)
        np.testing.assert_allclose(lo, r_lo, rtol=1e-6, atol=0)
        np.testing.assert_allclose(pairs, r_pairs, rtol=1e-6, atol=1e-12)
        for o, sl in enumerate((slice(0, 2), slice(2, 16))):
            err, top = np.abs(g[:, sl] - r_g[:, sl]).max(), np.abs(r_g[:, sl]).max()
            print("  output", o, "max |dhead - ref|", err, "of", top)
            assert err <= 1e-6 * top
            if kind == "random":
                zero = w[o] == 0
                assert zero.any() and not (g[:, sl][zero] != 0).any()
        # the evaluation entry: two sweeps added are twice the training entry's bits
        vals = lo.astype(np.float64)
        assert np.array_equal(acc[:3], vals + vals) and acc[3] == 2.0
        assert np.array_equal(acc[4:], (pairs + pairs).reshape(-1))
        # the same bits on a second run
        g2, lo2, pairs2, acc2 = _head_weighted(spec, dev_in, M, w)
        assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(lo), _bits(lo2))
        assert np.array_equal(_bits(pairs), _bits(pairs2)) and np.array_equal(_bits(acc), _bits(acc2))


@pytest.mark.parametrize("M", SIZES)
def test_metrics_under_metrics_stay_unweighted_and_weights_that_sum_to_zero(M):
    from lisec_amd.network import pair_values
    spec, head, yc, yr, dev_in = _head_case("mse", M)
    _, _, plain_met, _ = _head_plain(spec, dev_in, M)
    # only metric 1 of the class output (the categorical accuracy) and metric 0 of the regression output are weighted
    weighted = ((1,), (0,))
    w = _maps("random", M, 3)
    _, _, pairs, _ = _head_weighted(spec, dev_in, M, w, weighted=weighted)
    _, r_pairs, _ = SW.head_loss(spec, head, yc, yr, w=w, weighted=weighted)
    np.testing.assert_allclose(pairs, r_pairs, rtol=1e-6, atol=1e-12)
    keep = [0, 2, 3, 5, 6, 7]
    np.testing.assert_allclose(pairs[keep, 0] / pairs[keep, 1], plain_met[keep], rtol=1e-6, atol=1e-12)
    assert pairs[keep, 1].tolist() == [float(M * c) for c in (2, 2, 2, 14, 14, 1)]
    # +1, -1, ..., and a last 0: the weights sum to exactly 0, the weighted sums do not
    z = np.zeros(M, np.float32)
    z[:M - M % 2] = np.tile(np.float32([1, -1]), M // 2)
    _, lo, pairs, acc = _head_weighted(spec, dev_in, M, (z, z))
    assert (pairs[:, 1] == 0).all() and (M == 1 or (pairs[:, 0] != 0).any())
    assert pair_values(pairs.reshape(-1)) == [0.0] * 8 and pair_values(acc[4:]) == [0.0] * 8


def test_head_loss_weighted_refusals():
    """Every LISEC_EINVAL of the weighted head entries, each with a text in lisec_last_error and every output untouched."""
    import torch
    from lisec_amd import _lib, ops
    lib = _lib.load()
    M = 64
    spec, head, yc, yr, (d_head, d_yc, d_yr) = _head_case("huber", M)
    d_w = _dev(np.ones(M), np.ones(1))
    dhead = torch.full((M, 16), 7.0, dtype=torch.float32, device="cuda")
    lo = torch.full((3,), 7.0, dtype=torch.float32, device="cuda")
    pairs = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    acc = torch.full((20,), 7.0, dtype=torch.float64, device="cuda")
    need = lib.lisec_head_loss_weighted_workspace_bytes()
    assert need % 256 == 0 and need >= lib.lisec_head_loss_workspace_bytes()
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    st = _lib.current_stream()
    good, good_sw = spec.descriptor(), ops.sample_weights(d_w[0], d_w[1], M, weighted_metrics=(0b1111, 0b0001))

    def train(cfg=good, sw=good_sw, head=d_head, yc=d_yc, yr=d_yr, M=M, dhead=dhead, lo=lo, pairs=pairs, ws=ws, nbytes=need):
        cfg, sw = (ctypes.byref(x) if x is not None else None for x in (cfg, sw))
        return lib.lisec_head_loss_weighted(cfg, sw, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M, 1.0, _lib.ptr(dhead),
                                            _lib.ptr(lo), _lib.ptr(pairs), _lib.ptr(ws), nbytes, st)

    def evaluate(cfg=good, sw=good_sw, head=d_head, yc=d_yc, yr=d_yr, M=M, acc=acc, ws=ws, nbytes=need):
        cfg, sw = (ctypes.byref(x) if x is not None else None for x in (cfg, sw))
        return lib.lisec_head_loss_weighted_eval(cfg, sw, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M, _lib.ptr(acc),
                                                 _lib.ptr(ws), nbytes, st)

    def refused(rc):
        assert rc != 0 and lib.lisec_last_error().decode().strip()

    for name in ("cfg", "sw", "head", "yc", "yr", "dhead", "lo", "pairs", "ws"):
        refused(train(**{name: None}))
    for name in ("cfg", "sw", "head", "yc", "yr", "acc", "ws"):
        refused(evaluate(**{name: None}))
    for m in (0, -5):
        refused(train(M=m))
        refused(evaluate(M=m))

    def bad_weights():
        for field, index, value in (("struct_bytes", None, 32), ("struct_bytes", None, 0), ("per_cell", 0, 2),
                                    ("per_cell", 1, -1), ("weighted_metrics", 0, 0b10000), ("weighted_metrics", 1, 1 << 31)):
            bad = ops.sample_weights(d_w[0], d_w[1], M, weighted_metrics=(1, 1))
            if index is None:
                setattr(bad, field, value)
            else:
                getattr(bad, field)[index] = value
            yield bad
    for bad in bad_weights():
        assert train(sw=bad) == EINVAL and evaluate(sw=bad) == EINVAL
        refused(train(sw=bad))
    # a metric bit at or above n_metrics of a descriptor with fewer metrics
    few = _spec(TERMS["mse"], TERMS["mse"], metrics=False).descriptor()
    bit = ops.sample_weights(d_w[0], d_w[1], M, weighted_metrics=(1, 0))
    assert train(cfg=few, sw=bit) == EINVAL and evaluate(cfg=few, sw=bit) == EINVAL
    # the refusals of lisec_head_loss
    bad = spec.descriptor()
    bad.loss[1].kind = 10
    assert train(cfg=bad) == EINVAL and evaluate(cfg=bad) == EINVAL
    bad = spec.descriptor()
    bad.loss[0].param = 0.0                                    # Huber's delta
    assert train(cfg=bad) == EINVAL and evaluate(cfg=bad) == EINVAL
    bad = spec.descriptor()
    bad.n_metrics[0] = 5
    assert train(cfg=bad) == EINVAL and evaluate(cfg=bad) == EINVAL
    refused(train(nbytes=need - 1))
    refused(evaluate(nbytes=need - 1))
    torch.cuda.synchronize()
    for t in (dhead, lo, pairs, acc):
        assert bool((t == 7.0).all().item())
    assert train() == 0 and evaluate() == 0
    torch.cuda.synchronize()
    assert lib.lisec_abi_version() == 14
    assert ctypes.sizeof(_lib.SampleWeights) == 40


# ---- the VoxelNet losses ------------------------------------------------------------------------------------------------
def _det_inputs(M, seed, b):
    """head, y_cls, y_reg (float32): logits N(0, 1.5) -- no gradient near the end of the fp32 range --, about a quarter of
    the anchors positive, a quarter ignored, residuals on both sides of |d| = b."""
    rng = np.random.default_rng(seed)
    head = rng.normal(0, 1.5, (M, 16)).astype(np.float32)
    y_cls = rng.choice(np.float32([0, 1, 2]), (M, 2), p=[0.25, 0.5, 0.25])
    y_cls[M // 2, 0] = 2.0
    d = rng.normal(0, 1.5 * b, (M, 14))
    y_reg = (head[:, 2:].astype(np.float64) - d + 1.0).astype(np.float32)
    return head, y_cls, y_reg


def _det_run(spec, dev_in, M, w=None, grad_scale=0.75, sweeps=2, per_cell=None):
    """(dhead, loss_out, counts, acc): the weighted entries of the spec's family, or with w None the unweighted ones."""
    import torch
    from lisec_amd import _lib
    from lisec_amd import losses as K
    lib = _lib.load()
    iou = isinstance(spec, K.DetectionIoULossSpec)
    stem = "lisec_detection_iou_loss" if iou else "lisec_detection_loss"
    cfg = spec.descriptor()
    dhead = torch.full((M, 16), float("nan"), dtype=torch.float32, device="cuda")
    loss_out = torch.full((4,), float("nan"), dtype=torch.float32, device="cuda")
    counts = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    acc = torch.zeros(5, dtype=torch.float64, device="cuda")
    acc[4] = -7.0
    st = _lib.current_stream()
    ptrs = [_lib.ptr(t) for t in dev_in]
    if w is None:
        ws = _Workspace(getattr(lib, stem + "_workspace_bytes")())
        _lib.check(getattr(lib, stem)(ctypes.byref(cfg), *ptrs, M, grad_scale, _lib.ptr(dhead), _lib.ptr(loss_out),
                                      _lib.ptr(counts), _lib.ptr(ws.buf), ws.need, st))
        for _ in range(sweeps):
            _lib.check(getattr(lib, stem + "_eval")(ctypes.byref(cfg), *ptrs, M, _lib.ptr(acc), _lib.ptr(ws.buf), ws.need, st))
    else:
        d_w = _dev(*w)
        sw = _sw(w, d_w, M, per_cell=per_cell)
        ws = _Workspace(getattr(lib, stem + "_weighted_workspace_bytes")())
        _lib.check(getattr(lib, stem + "_weighted")(ctypes.byref(cfg), ctypes.byref(sw), *ptrs, M, grad_scale,
                                                    _lib.ptr(dhead), _lib.ptr(loss_out), _lib.ptr(counts), _lib.ptr(ws.buf),
                                                    ws.need, st))
        for _ in range(sweeps):
            _lib.check(getattr(lib, stem + "_weighted_eval")(ctypes.byref(cfg), ctypes.byref(sw), *ptrs, M, _lib.ptr(acc),
                                                             _lib.ptr(ws.buf), ws.need, st))
    torch.cuda.synchronize()
    assert ws.intact()
    lo, cn, ac = loss_out.cpu().numpy(), counts.cpu().numpy(), acc.cpu().numpy()
    assert np.isnan(lo[3]) and cn[2] == -1 and ac[4] == -7.0
    return dhead.cpu().numpy(), lo[:3], cn[:2], ac[:4]


def _det_checks(spec, head, y_cls, y_reg, M, ref_kw, positives_rel=False):
    """The unit-weight, power-of-two, random-weight and evaluation statements for one detection spec and one input.
    positives_rel: the IoU loss's measure of test_gpu_detection_iou_loss.py for the regression output, per positive
    anchor |got - ref| / max_k |ref_k| <= 1e-6 (its reference gradient is a central difference)."""
    dev_in = _dev(head, y_cls, y_reg)
    plain_g, plain_lo, plain_cn, plain_acc = _det_run(spec, dev_in, M)
    for kind in ("sweep_one", "map_ones"):
        g, lo, cn, acc = _det_run(spec, dev_in, M, _maps(kind, M, 0))
        assert np.array_equal(_bits(g), _bits(plain_g)) and np.array_equal(_bits(lo), _bits(plain_lo)), kind
        assert np.array_equal(cn, plain_cn) and np.array_equal(_bits(acc), _bits(plain_acc))
    w = _maps("pow2", M, M)
    _, _, ref_g = SW.detection_loss(head, y_cls, y_reg, grad_scale=0.75, **ref_kw)
    assert _scaled_exactly(ref_g, w)
    g, _, cn, _ = _det_run(spec, dev_in, M, w)
    rows = np.concatenate([np.repeat(w[0][:, None], 2, 1), np.repeat(w[1][:, None], 14, 1)], 1)
    assert np.array_equal(_bits(g), _bits(plain_g * rows)) and np.array_equal(cn, plain_cn)
    pos = y_cls > 1.5
    for kind in ("random", "mixed"):
        w = _maps(kind, M, M + 1)
        r_lo, r_cn, r_g = SW.detection_loss(head, y_cls, y_reg, w=w, grad_scale=0.75, **ref_kw)
        g, lo, cn, acc = _det_run(spec, dev_in, M, w)
        print(M, kind, "loss", lo, "ref", r_lo, "counts", cn)
        assert np.array_equal(cn, r_cn) and np.array_equal(cn, plain_cn)          # the counts stay unweighted
        np.testing.assert_allclose(lo, r_lo, rtol=1e-6, atol=0)
        for o, sl in enumerate((slice(0, 2), slice(2, 16))):
            if o == 1 and positives_rel:
                got, ref = g[:, 2:].reshape(M, 2, 7)[pos].astype(np.float64), r_g[:, 2:].reshape(M, 2, 7)[pos]
                top = np.abs(ref).max(axis=1)
                err = np.abs(got - ref).max(axis=1)[top > 0] / top[top > 0]
                print("  positives", len(got), "worst |got - ref| / max_k |ref_k|", err.max(initial=0.0))
                assert err.max(initial=0.0) <= 1e-6
                assert not _bits(g[:, 2:].reshape(M, 2, 7))[~pos].any()
            else:
                err, top = np.abs(g[:, sl] - r_g[:, sl]).max(), np.abs(r_g[:, sl]).max()
                print("  output", o, "max |dhead - ref|", err, "of", top)
                assert err <= 1e-6 * top
            if kind == "random":
                zero = w[o] == 0
                assert zero.any() and not (g[:, sl][zero] != 0).any()
        vals = lo.astype(np.float64)
        assert np.array_equal(acc[:3], vals + vals) and acc[3] == 2.0
        g2, lo2, cn2, acc2 = _det_run(spec, dev_in, M, w)
        assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(lo), _bits(lo2))
        assert np.array_equal(cn, cn2) and np.array_equal(_bits(acc), _bits(acc2))


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_detection_loss_weighted(gamma, M):
    from lisec_amd import losses as K
    b = 1.0 / 9.0 if gamma else 1.0
    params = dict(alpha=1.5 if gamma == 0 else 0.5, beta=1.0 if gamma == 0 else 1.5, gamma=gamma, smooth_l1_beta=b)
    spec, _ = K.compile_loss(K.VoxelNetLoss(**params), loss_weights=[2.0, 0.5])
    head, y_cls, y_reg = _det_inputs(M, seed=M + int(gamma), b=b)
    _det_checks(spec, head, y_cls, y_reg, M, dict(weights=(2.0, 0.5), **params))


@pytest.mark.parametrize("pattern,M,combo", [("positives", 17, 1), ("mix", 17, 3), ("stride", C.STRIDE_M, 1),
                                             ("stride", C.STRIDE_M, 3)])
def test_detection_iou_loss_weighted(pattern, M, combo):
    """Both IoU modes (combo 1: 'bev', focal; combo 3: '3d') on the inputs of tests/detection_iou_cases.py, whose seeds
    keep every positive away from the kinks of the IoU: 17 cells, and one size past the single trip of k_det_iou's 1024
    workgroups of 128 cells."""
    from lisec_amd import losses as K
    det, iou = C.params(combo)
    spec, _ = K.compile_loss(K.VoxelNetIoULoss(**det, **iou), loss_weights=list(C.WEIGHTS))
    head, y_cls, y_reg = C.case(pattern, M, combo)
    _det_checks(spec, head, y_cls, y_reg, M, dict(weights=C.WEIGHTS, iou=iou, **det), positives_rel=True)


def test_detection_loss_weighted_refusals():
    """Every LISEC_EINVAL of the four weighted detection entries, with every output untouched."""
    import torch
    from lisec_amd import _lib, ops
    from lisec_amd import losses as K
    lib = _lib.load()
    M = 64
    d_head, d_yc, d_yr = _dev(*C.build("mix", M, 1, seed=1))
    d_w = _dev(np.ones(M), np.ones(1))
    dhead = torch.full((M, 16), 7.0, dtype=torch.float32, device="cuda")
    lo = torch.full((3,), 7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    acc = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    st = _lib.current_stream()
    for name, stem in (("voxelnet", "lisec_detection_loss"), ("voxelnet_iou", "lisec_detection_iou_loss")):
        need = getattr(lib, stem + "_weighted_workspace_bytes")()
        assert need == lib.lisec_detection_loss_workspace_bytes()
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        good, good_sw = K.compile_loss(name)[0].descriptor(), ops.sample_weights(d_w[0], d_w[1], M)

        def train(cfg=good, sw=good_sw, head=d_head, yc=d_yc, yr=d_yr, M=M, dhead=dhead, lo=lo, counts=counts, ws=ws,
                  nbytes=need):
            cfg, sw = (ctypes.byref(x) if x is not None else None for x in (cfg, sw))
            return getattr(lib, stem + "_weighted")(cfg, sw, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M, 1.0,
                                                    _lib.ptr(dhead), _lib.ptr(lo), _lib.ptr(counts), _lib.ptr(ws), nbytes, st)

        def evaluate(cfg=good, sw=good_sw, head=d_head, yc=d_yc, yr=d_yr, M=M, acc=acc, ws=ws, nbytes=need):
            cfg, sw = (ctypes.byref(x) if x is not None else None for x in (cfg, sw))
            return getattr(lib, stem + "_weighted_eval")(cfg, sw, _lib.ptr(head), _lib.ptr(yc), _lib.ptr(yr), M,
                                                         _lib.ptr(acc), _lib.ptr(ws), nbytes, st)

        def refused(rc):
            assert rc == EINVAL and lib.lisec_last_error().decode().strip()

        for arg in ("cfg", "sw", "head", "yc", "yr", "dhead", "lo", "counts", "ws"):
            refused(train(**{arg: None}))
        for arg in ("cfg", "sw", "head", "yc", "yr", "acc", "ws"):
            refused(evaluate(**{arg: None}))
        for m in (0, -5):
            refused(train(M=m))
            refused(evaluate(M=m))
        for field, index, value in (("struct_bytes", None, 32), ("struct_bytes", None, 0), ("per_cell", 0, 2),
                                    ("per_cell", 1, -1), ("weighted_metrics", 0, 1), ("weighted_metrics", 1, 8)):
            bad = ops.sample_weights(d_w[0], d_w[1], M)
            if index is None:
                setattr(bad, field, value)
            else:
                getattr(bad, field)[index] = value
            refused(train(sw=bad))
            refused(evaluate(sw=bad))
        # the refusals of the unweighted entries
        for field, value in (("alpha", -1.0), ("beta", -0.25), ("gamma", -2.0), ("smooth_l1_beta", 0.0), ("struct_bytes", 32)):
            bad = K.compile_loss(name)[0].descriptor()
            setattr(bad.det if name == "voxelnet_iou" else bad, field, value)
            refused(train(cfg=bad))
            refused(evaluate(cfg=bad))
        if name == "voxelnet_iou":
            for field, value in (("struct_bytes", 64), ("iou_weight", -1.0), ("iou_weight", float("nan")), ("iou_mode", 2)):
                bad = K.compile_loss(name)[0].descriptor()
                setattr(bad, field, value)
                refused(train(cfg=bad))
                refused(evaluate(cfg=bad))
            bad = K.compile_loss(name)[0].descriptor()
            bad.anchors[1][1] = -3.9
            refused(train(cfg=bad))
            refused(evaluate(cfg=bad))
        refused(train(nbytes=need - 1))
        refused(evaluate(nbytes=need - 1))
        torch.cuda.synchronize()
        for t in (dhead, lo, counts, acc):
            assert bool((t == 7).all().item())
    assert lib.lisec_abi_version() == 14


# ---- Model.fit / evaluate on createModel(16, 32, 8, 35): M = 128 cells ----------------------------------------------------
import json  # noqa: E402
import socket  # noqa: E402
import subprocess  # noqa: E402

from test_gpu_optimizers import _cloud, _data, _dump, _same, _targets  # noqa: E402

GRID = (8, 16)
W_NAMES = ["loss", "ClassificationLayer_loss", "RegressionLayer_loss", "ClassificationLayer_binary_accuracy",
           "ClassificationLayer_weighted_accuracy", "ClassificationLayer_weighted_mae", "RegressionLayer_mae",
           "RegressionLayer_weighted_mae", "RegressionLayer_weighted_mse"]


def _compile(model, loss, opt=None):
    from lisec_amd import model_training as mt
    opt = opt or mt.optimizers.SGD(lr=0.01, decay=1e-3, momentum=0.9, nesterov=True)
    if loss == "spec":
        model.compile(optimizer=opt, loss=[mt.losses.BinaryCrossentropy(from_logits=True), mt.losses.Huber(delta=0.5)],
                      loss_weights=[2.0, 0.5],
                      metrics={"ClassificationLayer": [mt.metrics.BinaryAccuracy(threshold=0.0)], "RegressionLayer": ["mae"]},
                      weighted_metrics={"ClassificationLayer": ["accuracy", "mae"], "RegressionLayer": ["mae", "mse"]})
        assert model.metrics_names == W_NAMES
    elif loss == "spec_plain":
        model.compile(optimizer=opt, loss=[mt.losses.BinaryCrossentropy(from_logits=True), mt.losses.Huber(delta=0.5)],
                      loss_weights=[2.0, 0.5])
    elif loss == "voxelnet":
        model.compile(optimizer=opt, loss="voxelnet", metrics=["anchor_recall", "positive_mae"])
    else:
        model.compile(optimizer=opt, loss=loss)


def _fit_weights(kind, n, seed=5):
    """sample_weight of n sweeps: None, per-sweep ones, maps of ones, or random maps in [0, 3] with a zero block on the class
    output and a per-sweep weight on the regression output."""
    rng = np.random.default_rng(seed)
    if kind == "none":
        return None
    if kind == "ones_sweep":
        return np.ones(n, np.float32)
    if kind == "ones_cell":
        return [np.ones((n,) + GRID, np.float32), np.ones((n,) + GRID, np.float32)]
    if kind == "random":
        wc = rng.uniform(0, 3, (n,) + GRID).astype(np.float32)
        wc[:, :2] = 0.0
        return {"ClassificationLayer": wc, "RegressionLayer": rng.uniform(0.5, 2, n).astype(np.float32)}
    raise ValueError(kind)


def _variables(model):
    import torch
    torch.cuda.synchronize()
    net = model.net
    d = dict(theta=net.params.theta.cpu().numpy().copy(), state=net.params.state.cpu().numpy().copy(),
             iterations=np.array(net.iterations))
    for name in model.optimizer.spec().slots:
        d["slot_" + name] = net.slot(name).cpu().numpy().copy()
    return d


def _fresh(loss, opt=None):
    from lisec_amd import model_training as mt
    np.random.seed(0)
    model = mt.createModel(16, 32, 8, 35)
    _compile(model, loss, opt)
    return model


@pytest.mark.parametrize("loss", ["mse", "spec_plain", "voxelnet"])
def test_fit_with_unit_weights_is_fit_without_weights(loss):
    """Per-sweep ones and maps of ones: theta, BN state, slots and History of the unweighted fit, bit for bit -- the
    weighted entries (for 'mse' the LossSpec of its two terms in place of lisec_rpn_loss) at w = 1.  The LossSpec has no
    Keras metrics here: under weights those are pooled {num, den} pairs divided once in fp64, without weights the mean of
    the sweeps' fp32 values, equal to 1e-6 (test_evaluate_and_validation_under_sample_weights) and not to the bit; the
    detection metrics of 'voxelnet' are pairs either way."""
    from lisec_amd import model_training as mt
    runs = {}
    for kind in ("none", "ones_sweep", "ones_cell"):
        model = _fresh(loss)
        x, y = _data(mt, True)
        hist = model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=2, shuffle=False, sample_weight=_fit_weights(kind, 3))
        assert model._captured is not None and (model._captured[1].wform is None) == (kind == "none")
        runs[kind] = (_variables(model), hist.history)
        model._captured[1].close()
    for kind in ("ones_sweep", "ones_cell"):
        _same(runs["none"][0], runs[kind][0])
        assert runs["none"][1] == runs[kind][1], kind
    assert int(runs["none"][0]["iterations"]) == 6


def _plan_worker(args):
    from lisec_amd import model_training as mt
    step_plan = bool(args["step_plan"])
    model = _fresh("spec")
    x, y = _data(mt, step_plan, n=4)
    hist = model.fit(x=x, y=y, batch_size=args["batch"], verbose=0, epochs=2, shuffle=False,
                     sample_weight=_fit_weights("random", 4))
    assert (getattr(model, "_captured", None) is not None) == step_plan
    assert list(hist.history) == W_NAMES
    _dump(model, args["out"])
    with open(args["out"] + ".json", "w") as f:
        json.dump(hist.history, f)


def _run_worker(tmp_path, tag, **args):
    out = str(tmp_path / f"{tag}.npz")
    args["out"] = out
    env = dict(os.environ)
    env["LISEC_TUNING"] = "step_plan=%d" % args["step_plan"]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", json.dumps(args)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out + ".json") as f:
        hist = json.load(f)
    return dict(np.load(out)), hist


@pytest.mark.parametrize("batch", [1, 2])
def test_weighted_step_plan_is_bit_identical_to_python_schedule(tmp_path, batch):
    """Random per-cell weights on the class output, per-sweep weights on the regression output: the recorded plans (two
    buffer sets, staged weights) against the Python schedule, at batch_size 1 and 2."""
    plan, hp = _run_worker(tmp_path, "plan", step_plan=1, batch=batch)
    eager, he = _run_worker(tmp_path, "eager", step_plan=0, batch=batch)
    assert int(plan["iterations"]) == 2 * 4 // batch
    _same(plan, eager)
    assert hp == he


def test_a_sweep_of_weight_zero_leaves_theta_and_counts_the_iteration():
    """Plain SGD, no regularizer: per-sweep weight 0 on both outputs is a zero gradient (of either sign), so every variable
    keeps its bits while the iteration count advances."""
    from lisec_amd import model_training as mt
    for loss in ("mse", "spec", "voxelnet"):
        model = _fresh(loss, mt.optimizers.SGD(lr=0.01, momentum=0.0))
        x, y = _data(mt, True, n=2)
        before = _variables(model)["theta"]
        hist = model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, shuffle=False, sample_weight=np.zeros(2, np.float32))
        after = _variables(model)
        assert int(after["iterations"]) == 2 and np.array_equal(before.view(np.uint32), after["theta"].view(np.uint32))
        assert hist.history["loss"] == [0.0]
        model._captured[1].close()


def _reference_logs(model, x, y, sw):
    """The compiled 'spec' loss and metrics from predict()'s outputs under the weights, in fp64 on the host: the losses
    as means over the sweeps, the weighted metrics as pooled sums divided once, the unweighted ones as sweep means."""
    cls, reg = model.predict(x)
    spec = model.loss
    weighted = tuple(tuple(j for j in range(len(spec.metrics[o])) if spec.weighted[o] >> j & 1) for o in range(2))
    losses_, pairs = [], []
    for i in range(len(cls)):
        head = np.concatenate([cls[i].reshape(-1, 2), reg[i].reshape(-1, 14)], 1)
        w = tuple(None if a is None else a[i] for a in sw)
        lo, pr, _ = SW.head_loss(spec, head, y[0][i], y[1][i], w=w, weighted=weighted)
        losses_.append(lo)
        pairs.append(pr)
    pooled = np.sum(pairs, 0)
    return list(np.mean(losses_, 0)) + [SW.div_no_nan(a, b) for a, b in pooled]


def test_evaluate_and_validation_under_sample_weights(monkeypatch):
    from lisec_amd import _lib, model_training as mt
    model = _fresh("spec")
    x, y = _data(mt, True, n=4)
    w = _fit_weights("random", 4)
    sw = [w["ClassificationLayer"], w["RegressionLayer"]]
    got = model.evaluate(x, y, verbose=0, sample_weight=w)
    d = model.evaluate(x, y, verbose=0, sample_weight=sw, return_dict=True)
    assert list(d) == W_NAMES and got == [d[k] for k in W_NAMES]
    ref = _reference_logs(model, x, y, sw)
    print("evaluate", got, "ref", ref)
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-7)
    # without weights a weighted metric is the unweighted one; with them the metrics= stay unweighted
    plain = model.evaluate(x, y, verbose=0, return_dict=True)
    assert plain["RegressionLayer_weighted_mae"] == plain["RegressionLayer_mae"]
    assert d["ClassificationLayer_binary_accuracy"] == pytest.approx(plain["ClassificationLayer_binary_accuracy"], rel=1e-6)
    assert d["RegressionLayer_mae"] == pytest.approx(plain["RegressionLayer_mae"], rel=1e-6)
    assert d["ClassificationLayer_weighted_mae"] != plain["ClassificationLayer_weighted_mae"]
    # weights that sum to zero on the class output: its weighted metrics report 0.0
    zero = model.evaluate(x, y, verbose=0, return_dict=True, sample_weight=[np.zeros(4, np.float32), None])
    assert zero["ClassificationLayer_weighted_accuracy"] == 0.0 and zero["ClassificationLayer_weighted_mae"] == 0.0
    assert zero["ClassificationLayer_loss"] == 0.0
    assert zero["RegressionLayer_weighted_mae"] == pytest.approx(plain["RegressionLayer_mae"], rel=1e-6)
    # the recorded evaluation step
    monkeypatch.setattr(_lib, "knob", lambda name, default: True if name == "eval_plan" else default)
    plan = model.evaluate(x, y, verbose=0, sample_weight=w)
    assert model._eval_captured is not None and model._eval_captured[1].wform == ("cell", "sweep")
    assert model._eval_captured[1].nacc == 4 + 2 * 6
    np.testing.assert_allclose(plan, got, rtol=1e-6)
    monkeypatch.undo()
    # validation_data=(x, y, w): the same numbers under val_*, for the variables as the epoch left them
    vx, vy, vw = x[2:], [y[0][2:], y[1][2:]], [a[2:] for a in sw]
    hist = model.fit(x=x[:2], y=[y[0][:2], y[1][:2]], batch_size=1, verbose=0, epochs=1, shuffle=False,
                     validation_data=(vx, vy, vw), sample_weight=[a[:2] for a in sw])
    assert list(hist.history) == W_NAMES + ["val_" + k for k in W_NAMES]
    after = model.evaluate(vx, vy, verbose=0, sample_weight=vw)
    np.testing.assert_allclose([hist.history["val_" + k][0] for k in W_NAMES], after, rtol=1e-6)
    np.testing.assert_allclose(after, _reference_logs(model, vx, vy, vw), rtol=1e-6, atol=1e-7)
    # validation_split splits the weights with the labels
    h2 = _fresh("spec").fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, shuffle=False, validation_split=0.5, sample_weight=w)
    h3 = _fresh("spec").fit(x=x[:2], y=[y[0][:2], y[1][:2]], batch_size=1, verbose=0, epochs=1, shuffle=False,
                            validation_data=(vx, vy, vw), sample_weight=[a[:2] for a in sw])
    assert h2.history == h3.history


class _Sweeps:
    """A keras.utils.Sequence by its interface: item i = (points, [y_cls, y_reg], sample_weight)."""

    def __init__(self, weights):
        self.weights = weights

    def __len__(self):
        return 3

    def __getitem__(self, i):
        yc, yr = _targets(i)
        w = self.weights
        if w is None:
            return _cloud(i), [yc, yr]
        return _cloud(i), [yc, yr], {k: (float(a[i]) if a.ndim == 1 else a[i]) for k, a in w.items()}

    def on_epoch_end(self):
        pass


def test_a_sequence_of_three_tuples_trains_to_the_bits_of_the_list_form():
    from lisec_amd import model_training as mt
    w = _fit_weights("random", 3)
    model = _fresh("spec")
    x = [mt.VFE_preprocessing(_cloud(i), *model._sequence_grid()) for i in range(3)]
    ys = [_targets(i) for i in range(3)]
    y = [np.stack([t[0] for t in ys]), np.stack([t[1] for t in ys])]
    h_list = model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=2, shuffle=False, sample_weight=w)
    a = _variables(model)
    model._captured[1].close()
    model = _fresh("spec")
    h_seq = model.fit(x=_Sweeps(w), batch_size=1, verbose=0, epochs=2, shuffle=False)
    assert model._captured[1].wform == ("cell", "sweep")
    _same(a, _variables(model))
    assert h_list.history == h_seq.history
    with pytest.raises(ValueError, match="sample_weight"):
        model.fit(x=_Sweeps(w), batch_size=1, verbose=0, sample_weight=np.ones(3))
    model._captured[1].close()


def test_python_refusals_come_before_any_launch():
    from lisec_amd import model_training as mt
    model = _fresh("spec")
    x, y = _data(mt, True, n=3)
    before = _variables(model)
    nan = np.ones(3, np.float32)
    nan[1] = np.nan
    inf = np.ones((3,) + GRID, np.float32)
    inf[2, 1, 1] = np.inf
    bad = [np.ones((3, 4)), np.ones((3, 16, 8)), np.ones((3, 8, 16, 1)), np.ones(2), np.ones((2,) + GRID), nan, inf,
           [np.ones(3)], [np.ones(3), np.ones(3), np.ones(3)], {"Other": np.ones(3)}, [None, np.ones((3, 2))], "heavy"]
    for w in bad:
        with pytest.raises(ValueError):
            model.fit(x=x, y=y, verbose=0, sample_weight=w)
        with pytest.raises(ValueError):
            model.evaluate(x, y, verbose=0, sample_weight=w)
        with pytest.raises(ValueError):
            model.fit(x=x, y=y, verbose=0, validation_data=(x, y, w))
    with pytest.raises(ValueError, match="class_weight"):
        model.fit(x=x, y=y, verbose=0, class_weight={0: 1.0, 1: 2.0})
    with pytest.raises(NotImplementedError):
        model.compile(optimizer="sgd", loss="voxelnet", weighted_metrics=["mae"])
    with pytest.raises(ValueError):
        model.compile(optimizer="sgd", loss="mse", metrics=["mae", "mse", "mape"], weighted_metrics=["mae", "mse"])
    assert model._captured is None
    _same(before, _variables(model))
    # [None, None] is no weighting at all
    assert mt._sample_weight_arrays([None, None], 3, GRID) is None


def _dp_worker(rank, world, port, out_dir):
    import torch
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), LISEC_DIST_BACKEND="gloo", LISEC_BENCH_DEVICE="0")   # both ranks on cuda:0
    from lisec_amd import model_training as mt
    model = _fresh("spec")
    assert model.dp is not None and model.dp.world == 2
    x, y = _data(mt, True, n=4)
    w = _fit_weights("random", 4)
    hist = model.fit(x=x, y=y, batch_size=1, verbose=0, epochs=1, steps_per_epoch=4, shuffle=False, sample_weight=w)
    ev = model.evaluate(x, y, verbose=0, sample_weight=w)
    torch.cuda.synchronize()
    _dump(model, os.path.join(out_dir, f"rank{rank}.npz"))
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(dict(history=hist.history, evaluate=ev), f)
    model.dp.barrier()
    model.dp.close()


def test_two_ranks_keep_identical_variables_under_sample_weights():
    import tempfile
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        mp.spawn(_dp_worker, args=(2, port, d), nprocs=2, join=True)
        r0, r1 = dict(np.load(os.path.join(d, "rank0.npz"))), dict(np.load(os.path.join(d, "rank1.npz")))
        j0, j1 = (json.load(open(os.path.join(d, f"rank{r}.json"))) for r in (0, 1))
    assert int(r0["iterations"]) == 2
    for k in r0:
        if k != "state":                                       # BN moving statistics are per replica
            assert np.array_equal(r0[k], r1[k]), k
    assert list(j0["history"]) == W_NAMES and j0["evaluate"] == j1["evaluate"] and len(j0["evaluate"]) == len(W_NAMES)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "worker":
    _plan_worker(json.loads(sys.argv[2]))
