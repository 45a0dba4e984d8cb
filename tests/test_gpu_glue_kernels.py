"""The kernels BETWEEN the contractions, one exported entry point at a time, against the fp64 definitions of tests/glue_ref.py
(themselves checked by tests/test_glue_ref.py), at the smallest shapes that reach every branch (tests/glue_cases.py).

No tolerance comes from the code under test.  With u = 2^-24:
  * permutations, copies, packs, the ReLU gate, the shuffle and lisec_scale: bit equality;
  * fp32 sums of n products (lisec_head_compose: n = Cup, the composite bias: Cup + 1; lisec_head_compose_backward:
    d_up_kernel and d_up_bias n = 16, d_head_w n = taps * Cin + 1):  |got - ref64| <= (n + 2) u A  elementwise, A the same
    expression over absolute values -- the worst case of any summation order with or without fma; a dropped or doubled
    term misses it by three to four orders of magnitude at these sizes (tests/test_glue_ref.py);
  * values formed in fp64 and rounded once (lisec_bn_finalize, lisec_bn_fold, g_all and the one-fma dW update of
    lisec_const_field_grads):  |got - ref64| <= 2^-23 |ref64|, plus 1e-12 A for g_all and 1e-9 max(1, |ref|) for the
    BatchNormalization state (fp64 reassociation, |mean| <= 3 and var >= 0.1).
Outputs a kernel must write completely start as NaN; memory it must leave alone starts as a sentinel and is compared
bit for bit.

Largest err / bound seen per entry point on an MI355X, over all cases (every test prints its own):
  lisec_head_compose           Wc 0.139, composite bias 0.050 (chained in place 0.046)
  lisec_head_compose_backward  d_up_kernel 0.181, d_head_w 0.046, d_up_bias 0.131
  lisec_const_field_grads      g_all 0.467, dW 0.500
  lisec_bn_finalize            bnstate 0.668, moving mean 0.481, moving variance 0.485
  lisec_bn_fold                bnstate 0.603
  everything else              bit equality (lisec_conv_tap_sums_finish: S and dy bit-equal to the fused call)
0.5 is what one correct rounding of the fp64 value costs against a bound of 2^-23 |ref| = 2u |ref|: g_all, dW and the
moving statistics sit there.  The two bnstate ratios above it come from eps: the kernels add kBnEps = 1e-3f widened to
double (0.0010000000475), not 1e-3, which moves invstd by 2.4e-8 relative where the variance is far below eps (the
clamped constant column of lisec_bn_finalize, the 1e-6 variances of lisec_bn_fold) -- a fifth of the bound, on top of
the rounding.  The momentum had the same flaw in lisec_bn_finalize ((double)0.99f, 9.5e-9 off) and did NOT fit: a moving
mean whose two terms nearly cancel missed the bound by up to 19x (test_bn_finalize, every C and nparts) until
k_bn_finalize took 0.99 itself, as the finaliser of a lisec_bn_sink always has.
"""
import ctypes

import numpy as np
import pytest
import torch

import glue_cases as K
import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENTINEL = -1234.5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _bits(t):
    """int32 view: +0.0 and -0.0, and NaN payloads, compare as what they are."""
    return t.contiguous().view(torch.int32)


def _within(got, ref, bound, what):
    """|got - ref| <= bound elementwise (a NaN in `got` fails); prints the largest err / bound."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"{what}: max err {np.nanmax(err):.3e}, max err/bound {np.nanmax(ratio):.3f}")
    assert np.isfinite(got).all(), f"{what}: not every element was written"
    assert (err <= bound).all(), f"{what}: max err/bound {np.nanmax(ratio):.3f}"


# ---- lisec_head_compose -------------------------------------------------------------------------------------------------------
def _wc_layout(layout, taps, cin):
    """(tap stride, c stride, offset, floats) of a composite-kernel buffer; (payload index array) comes from _wc_index."""
    if layout == "tap_c_j":                                    # Wc[tap][c][j]: the transposed convolutions (kernel 3, stride 1)
        return cin * 16, 16, 0, taps * cin * 16
    if layout == "c_tap_j":                                    # Wc[c][tap*16 + j]: the kernel == stride branches as 1x1
        return 16, taps * 16, 0, taps * cin * 16
    # tap_c_j with gaps, inside a larger buffer: 4 floats behind every (tap, c) row, 12 behind every tap, 8 in front
    return cin * 20 + 12, 20, 8, 8 + taps * (cin * 20 + 12) + 40


def _wc_index(ts, cs, off, taps, cin):
    return (off + np.arange(taps)[:, None, None] * ts + np.arange(cin)[None, :, None] * cs + np.arange(16)[None, None, :])


@pytest.mark.parametrize("layout", ["tap_c_j", "c_tap_j", "gaps"])
@pytest.mark.parametrize("taps,cin,cup", K.HEAD_CASES)
def test_head_compose(taps, cin, cup, layout):
    """Dead pairs in the last workgroup ((9,8,256): 8, (1,20,17): 12), Cup not a multiple of the 16 n-slices (40, 17), Cup
    at kMaxUp (512); both layouts of the network, and one with gaps in a larger NaN buffer where a stray store shows."""
    from lisec_amd import ops
    d = K.head_inputs(taps, cin, cup)
    ts, cs, off, floats = _wc_layout(layout, taps, cin)
    buf = _nan(floats)
    ops.head_compose(_dev(d["up_kernel"]), None, _dev(d["head_w"]), taps, cin, cup, buf[off:], ts, cs)
    got = _host(buf)
    idx = _wc_index(ts, cs, off, taps, cin)
    ref, A = R.head_compose(d["up_kernel"], d["head_w"])
    _within(got[idx], ref, R.sum_bound(cup, A), f"head_compose Wc {layout}")
    rest = np.ones(floats, bool)
    rest[idx.reshape(-1)] = False
    assert np.isnan(got[rest]).all()                           # nothing outside the (tap, c, j) elements was stored


@pytest.mark.parametrize("taps,cin,cup", K.HEAD_CASES)
def test_head_compose_bias_chain(taps, cin, cup):
    """bias_out from bias_in = NULL; chained through a second call with bias_out aliasing bias_in (LisecNet._compose_all);
    bias_out = NULL leaves the buffer alone.  n = Cup + 1 terms."""
    from lisec_amd import ops
    d, e = K.head_inputs(taps, cin, cup), K.head_inputs(taps, cin, cup, seed=1)
    wc = _nan(taps * cin * 16)
    bias = _nan(16)
    ops.head_compose(_dev(d["up_kernel"]), _dev(d["up_bias"]), _dev(d["head_w"]), taps, cin, cup, wc, cin * 16, 16,
                     bias_in=None, bias_out=bias)
    first = _host(bias).copy()
    ref, A = R.head_compose_bias(d["up_bias"], d["head_w"])
    _within(first, ref, R.sum_bound(cup + 1, A), "head_compose bias from NULL")
    ops.head_compose(_dev(e["up_kernel"]), _dev(e["up_bias"]), _dev(e["head_w"]), taps, cin, cup, wc, cin * 16, 16,
                     bias_in=bias, bias_out=bias)
    ref, A = R.head_compose_bias(e["up_bias"], e["head_w"], first)           # the definition, applied to what came in
    second = _host(bias).copy()
    _within(second, ref, R.sum_bound(cup + 1, A), "head_compose bias chained in place")
    wc.fill_(NAN)
    ops.head_compose(_dev(d["up_kernel"]), _dev(d["up_bias"]), _dev(d["head_w"]), taps, cin, cup, wc, cin * 16, 16,
                     bias_in=bias, bias_out=None)
    assert np.array_equal(_host(bias), second) and np.isfinite(_host(wc)).all()


def test_head_compose_rejects_what_it_cannot_hold():
    from lisec_amd import _lib, ops
    taps, cin = 2, 4
    wc, bias = _nan(taps * cin * 16), torch.full((16,), SENTINEL, device=DEV)
    w, h, b = torch.randn(taps, 513, cin, device=DEV), torch.randn(513, 16, device=DEV), torch.randn(513, device=DEV)
    with pytest.raises(_lib.LisecError):                        # Cup = 513 > kMaxUp: H does not fit its LDS copy
        ops.head_compose(w, b, h, taps, cin, 513, wc, cin * 16, 16, bias_out=bias)
    with pytest.raises(_lib.LisecError):                        # a composite bias without the branch bias
        ops.head_compose(w, None, h, taps, cin, 512, wc, cin * 16, 16, bias_out=bias)
    assert np.isnan(_host(wc)).all() and (_host(bias) == SENTINEL).all()


# ---- lisec_head_compose_backward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("layout", ["tap_c_j", "c_tap_j"])
@pytest.mark.parametrize("taps,cin,cup", K.HEAD_CASES)
def test_head_compose_backward(taps, cin, cup, layout, with_bias):
    """Cup = 40 and 17: the ragged last 32-row block of k_head_compose_bwd_w.  |up_bias| ~ 1 and |S| ~ 4: d_head_w without
    its up_bias[n] * S[j] term is > 1000 bounds away.  up_bias and d_up_bias may be NULL (the entry point checks neither):
    then d_head_w has no bias term and nothing else changes.  Two runs give equal bits (fixed summation order)."""
    from lisec_amd import ops
    d = K.head_inputs(taps, cin, cup)
    ts, cs, off, floats = _wc_layout(layout, taps, cin)
    g_buf = np.zeros(floats, np.float32)
    g_buf[_wc_index(ts, cs, off, taps, cin)] = d["G"]
    G, W, H, S = _dev(g_buf), _dev(d["up_kernel"]), _dev(d["head_w"]), _dev(d["S"])
    b = _dev(d["up_bias"]) if with_bias else None
    runs = []
    for _ in range(2):
        dk, dh = _nan(taps, cup, cin), _nan(cup, 16)
        db = _nan(cup) if with_bias else None
        ops.head_compose_backward(G, ts, cs, W, b, H, S, taps, cin, cup, dk, db, dh)
        runs.append((dk, dh, db))
    (rk, Ak), (rh, Ah), (rb, Ab) = R.head_compose_backward(d["G"], d["up_kernel"], d["up_bias"] if with_bias else None,
                                                           d["head_w"], d["S"])
    _within(_host(runs[0][0]), rk, R.sum_bound(16, Ak), "head_compose_backward d_up_kernel")
    _within(_host(runs[0][1]), rh, R.sum_bound(taps * cin + 1, Ah), "head_compose_backward d_head_w")
    if with_bias:
        _within(_host(runs[0][2]), rb, R.sum_bound(16, Ab), "head_compose_backward d_up_bias")
        assert torch.equal(_bits(runs[0][2]), _bits(runs[1][2]))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))


# ---- lisec_head_shuffle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strides", [(2,), (2, 4), (1, 2, 4)], ids=["s2", "s2_s4", "s1_s2_s4"])
@pytest.mark.parametrize("Ho,Wo", [(4, 8), (12, 20), (100, 200)])
def test_head_shuffle(Ho, Wo, strides):
    """Ho*Wo*4 float4s: 128 and 960 are no multiples of the 256-thread workgroup (a dead tail), 80 000 is many workgroups.
    Forward adds the branches in index order -- plain fp32 adds in a fixed order, so torch's fp32 sum is the exact value;
    backward is a gather."""
    from lisec_amd import ops
    g = torch.Generator().manual_seed(Ho + len(strides))
    head0 = torch.randn(Ho * Wo, 16, generator=g)
    Ts = [torch.randn((Ho // s) * (Wo // s), s * s * 16, generator=g) for s in strides]
    gather = []
    for s in strides:
        pos, tap = R.head_shuffle_index(Ho, Wo, s)
        gather.append((torch.from_numpy(pos), torch.from_numpy(tap)))
    want = head0.clone()
    for T, s, (pos, tap) in zip(Ts, strides, gather):
        want = want + T.reshape(-1, s * s, 16)[pos, tap]
    head = head0.to(DEV)
    dT = [t.to(DEV) for t in Ts]
    ops.HeadShuffle(Ho, Wo, list(zip(dT, strides))).run(head)
    torch.cuda.synchronize()
    assert torch.equal(_bits(head.cpu()), _bits(want))
    assert all(torch.equal(_bits(a.cpu()), _bits(b)) for a, b in zip(dT, Ts))        # the branches are only read
    dhead = head0.to(DEV)
    out = [_nan(*t.shape) for t in Ts]
    ops.HeadShuffle(Ho, Wo, list(zip(out, strides))).run(dhead, backward=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dhead.cpu()), _bits(head0))                             # dL/dhead is only read
    for o, s, (pos, tap) in zip(out, strides, gather):
        w = torch.full((o.shape[0], s * s, 16), NAN)
        w[pos, tap] = head0
        assert torch.equal(_bits(o.cpu()), _bits(w.reshape(o.shape)))


def test_head_shuffle_rejects_a_stride_that_does_not_divide_the_map_and_a_fifth_branch():
    from lisec_amd import _lib, ops
    head = torch.full((4 * 8, 16), SENTINEL, device=DEV)
    T = torch.full((64, 16 * 9), SENTINEL, device=DEV)
    with pytest.raises(_lib.LisecError):
        ops.HeadShuffle(4, 8, [(T, 3)]).run(head)
    with pytest.raises(_lib.LisecError):
        ops.HeadShuffle(4, 8, [(T, 1)] * 5).run(head)
    assert (_host(head) == SENTINEL).all() and (_host(T) == SENTINEL).all()


# ---- lisec_const_field_grads --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntaps,cin,cout", K.CONST_FIELD_CASES)
def test_const_field_grads(ntaps, cin, cout):
    """(9,12,20): ntaps*Cout = 180 < the 256 threads of k_const_field_gall; (27,160,128): 552 960 elements, the grid-stride
    loop of k_const_field_dw runs twice.  The two outputs alone, as the network asks for them; dW accumulates; the row
    index *cvec_row below, at and above cvec_row_max -- above must CLAMP: the table's next row exists and is NaN."""
    from lisec_amd import ops
    d = K.const_field_inputs(ntaps, cin, cout)
    W, S, table = _dev(d["W"]), _dev(d["S"]), _dev(d["table"])
    g_all = _nan(cin)
    ops.const_field_grads(W, S, None, ntaps, cin, cout, g_all=g_all)                     # g_all alone
    ref, A = R.const_field_g_all(d["W"], d["S"])
    _within(_host(g_all), ref, R.once_bound(ref) + 1e-12 * A, "const_field_grads g_all")
    dW = _dev(d["dW_old"])
    ops.const_field_grads(None, S, table[1], ntaps, cin, cout, dW=dW)                    # dW alone, a plain vector
    ref = R.const_field_dw(d["table"][1], d["S"], d["dW_old"])
    _within(_host(dW), ref, R.once_bound(ref), "const_field_grads dW += cvec S")
    for row, used in ((2, 2), (K.CVEC_ROW_MAX, K.CVEC_ROW_MAX), (K.CVEC_ROW_MAX + 1, K.CVEC_ROW_MAX)):
        dW = _dev(d["dW_old"])
        row_dev = torch.tensor([row], dtype=torch.int32, device=DEV)
        ops.const_field_grads(None, S, table, ntaps, cin, cout, dW=dW, cvec_row=row_dev, cvec_row_max=K.CVEC_ROW_MAX)
        ref = R.const_field_dw(d["table"][used], d["S"], d["dW_old"])
        _within(_host(dW), ref, R.once_bound(ref), f"const_field_grads dW, *cvec_row = {row}")
    both_dw, both_g = _dev(d["dW_old"]), _nan(cin)                                       # both in one call
    ops.const_field_grads(W, S, table[0], ntaps, cin, cout, dW=both_dw, g_all=both_g)
    assert torch.equal(_bits(both_g), _bits(g_all))
    ref = R.const_field_dw(d["table"][0], d["S"], d["dW_old"])
    _within(_host(both_dw), ref, R.once_bound(ref), "const_field_grads dW beside g_all")


def test_const_field_grads_rejects_an_output_without_its_operand():
    from lisec_amd import _lib, ops
    S = torch.randn(9, 8, device=DEV)
    dW, g_all = torch.full((9, 4, 8), SENTINEL, device=DEV), torch.full((4,), SENTINEL, device=DEV)
    with pytest.raises(_lib.LisecError):
        ops.const_field_grads(None, S, None, 9, 4, 8, g_all=g_all)
    with pytest.raises(_lib.LisecError):
        ops.const_field_grads(None, S, None, 9, 4, 8, dW=dW)
    assert (_host(dW) == SENTINEL).all() and (_host(g_all) == SENTINEL).all()


# ---- lisec_conv_tap_sums_bn(S = NULL) + lisec_conv_tap_sums_finish ----------------------------------------------------------
@pytest.mark.parametrize("ind,outd,stride,pad,C", K.TAP_SUM_CASES, ids=["s2_16x24", "p0_12x40", "ho5_c32"])
def test_tap_sums_split_pair_equals_the_fused_call(ind, outd, stride, pad, C):
    """The two halves on their own (the second runs on the side stream of the mid1 backward) against the one call, bit for
    bit, and against the independent tap-inside sum at the tolerance test_gpu_backward_ops.py holds the fused call to.
    ho5_c32: Ho = 5 is odd and below the 16 line lanes of k_tap_sums."""
    from lisec_amd import ops
    geo = ops.geom(0, ind, outd, (3, 3, 3), stride, pad, C, C)
    M = outd[0] * outd[1] * outd[2]
    g = torch.Generator().manual_seed(23 + C)
    dz = torch.randn(M, C, generator=g).to(DEV)
    y = (torch.randn(M, C, generator=g) * 1.5 + 0.2).to(DEV)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    inv = torch.rsqrt(var + 1e-3)
    gamma, beta = torch.rand(C, generator=g).to(DEV) + 0.5, torch.randn(C, generator=g).to(DEV)
    st = torch.cat([gamma * inv, beta - mean * gamma * inv, mean, inv]).contiguous()
    coef = torch.cat([dz.mean(0), (dz * (y - mean) * inv).mean(0)]).contiguous()
    nbytes = ops.tap_sums_workspace_bytes(geo)
    ws_fused = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)                 # every float a NaN
    ws_split = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    dy_fused, S_fused = dz.clone(), _nan(27, C)
    ops.tap_sums_bn(geo, dy_fused, y, st, coef, dy_fused, S_fused, ws_fused)
    dy_split, S_split = dz.clone(), _nan(27, C)
    ops.tap_sums_bn(geo, dy_split, y, st, coef, dy_split, None, ws_split)
    torch.cuda.synchronize()
    assert torch.isnan(S_split).all()                                                   # S = NULL: the first half stops
    ops.tap_sums_finish(geo, ws_split, S_split)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dy_split), _bits(dy_fused)) and torch.equal(_bits(S_split), _bits(S_fused))
    want_dy = torch.empty_like(dz)
    ops.bn_backward_apply_coef(dz, C, y, st, M, C, False, coef, want_dy)
    assert torch.equal(_bits(dy_split), _bits(want_dy))
    ref, _ = R.tap_inside_sums(_host(dy_split).reshape(*outd, C), ind, (3, 3, 3), stride, pad)
    np.testing.assert_allclose(_host(S_split), ref, rtol=1e-5, atol=1e-4)


# ---- lisec_fold_depth -----------------------------------------------------------------------------------------------------------
# the last: 2 * 2100 * 64 = 268 800 elements > kEwBlocks * kEwThreads = 1024 * 256: ew_blocks saturates, the loop repeats
@pytest.mark.parametrize("D,HW,C", [(1, 35, 64), (2, 77, 64), (3, 50, 8), (2, 2100, 64)])
def test_fold_depth(D, HW, C):
    from lisec_amd import ops
    g = torch.Generator().manual_seed(D * 1000 + HW)
    x = torch.randn(D, HW, C, generator=g)
    want = x.permute(1, 2, 0).reshape(HW, C * D)                                         # (H,W,C,D) flattened: c*D + d
    assert np.array_equal(want.numpy(), R.fold_depth(x.numpy()))
    out = _nan(HW, C * D)
    ops.fold_depth(x.to(DEV), out, D, HW, C)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out.cpu()), _bits(want))
    back = _nan(D, HW, C)
    ops.fold_depth(out, back, D, HW, C, inverse=True)                                    # no mask: the exact inverse
    torch.cuda.synchronize()
    assert torch.equal(_bits(back.cpu()), _bits(x))
    # the gate: positive, negative, +0.0 and -0.0 in the mask; the gradient itself holds negative values and a -0.0
    mask = torch.randn(D, HW, C, generator=g)
    mask.view(-1)[::7] = 0.0
    mask.view(-1)[3::11] = -0.0
    grad = torch.randn(HW, C * D, generator=g)
    grad.view(-1)[5] = -0.0
    gated = _nan(D, HW, C)
    ops.fold_depth(grad.to(DEV), gated, D, HW, C, inverse=True, mask=mask.to(DEV))
    torch.cuda.synchronize()
    unfolded = torch.from_numpy(R.unfold_depth(grad.numpy(), D))
    want = torch.where(mask > 0, unfolded, torch.zeros(()))
    assert torch.equal(gated.cpu(), want)
    assert torch.equal(_bits(gated.cpu()), _bits(want))                                  # closed gate: +0.0, not -0.0


# ---- lisec_copy2d_batched -------------------------------------------------------------------------------------------------------
def test_copy2d_batched():
    """One table, five descriptors: 1-D, contiguous 2-D, a column slice [:, 2:16] of a (768, 16) buffer and the way back
    (LisecNet's head merge / split), and 300 x 20 = 6000 > 16 y-blocks x 256 threads elements (the stride loop repeats)."""
    from lisec_amd import ops
    g = torch.Generator().manual_seed(5)

    def sent(*shape):
        return torch.full(shape, SENTINEL, device=DEV)
    src1, dst1 = torch.randn(37, generator=g).to(DEV), sent(50)
    src2, dst2 = torch.randn(7, 16, generator=g).to(DEV), sent(9, 16)
    src3, dst3 = torch.randn(768, 16, generator=g).to(DEV), sent(768, 14)
    src4, dst4 = torch.randn(768, 14, generator=g).to(DEV), sent(768, 16)
    src5, dst5 = torch.randn(300, 24, generator=g).to(DEV), sent(301, 22)
    pairs = [(src1, dst1[5:42]), (src2, dst2[1:8]), (src3[:, 2:16], dst3), (src4, dst4[:, 2:16]),
             (src5[:, 1:21], dst5[:300, 2:22])]
    before = [s.clone() for s in (src1, src2, src3, src4, src5)]
    ops.CopyTable(pairs, DEV).run()
    torch.cuda.synchronize()
    want = [sent(50), sent(9, 16), sent(768, 14), sent(768, 16), sent(301, 22)]
    want[0][5:42] = src1
    want[1][1:8] = src2
    want[2][:] = src3[:, 2:16]
    want[3][:, 2:16] = src4
    want[4][:300, 2:22] = src5[:, 1:21]
    for got, w in zip((dst1, dst2, dst3, dst4, dst5), want):
        assert torch.equal(_bits(got), _bits(w))                                         # payload and sentinels
    for s, b in zip((src1, src2, src3, src4, src5), before):
        assert torch.equal(_bits(s), _bits(b))


# ---- the weight packs -------------------------------------------------------------------------------------------------------------
def _pack_sources(ntaps, Kk, N, edge=None):
    """(name, device tensor, tap/k/n strides, the (taps, K, N) values it holds) for every source order of the case;
    edge: values written over the kernel's elements 1, 2, ... (in (tap, K, N) order)."""
    r = np.random.default_rng(ntaps * 1000 + Kk)
    w = r.standard_normal((ntaps, Kk, N)).astype(np.float32)
    w[0, 0, 0], w[-1, -1, -1] = -0.0, 0.0                                                # a -0.0 payload stays -0.0
    if edge is not None:
        w.reshape(-1)[1:1 + len(edge)] = edge
    out = [("keras", _dev(w), (Kk * N, N, 1), w),                                        # (tap, K, N)
           ("transposed", _dev(w.transpose(0, 2, 1)), (N * Kk, 1, Kk), w)]               # (tap, N, K): the deconv kernels
    if ntaps == 1:
        out.append(("tap_stride_0", _dev(w[0]), (0, N, 1), w))
    return out


@pytest.mark.parametrize("ntaps,Kk,N", K.PACK_CASES)
def test_pack_weights_zero_fills_the_padding(ntaps, Kk, N):
    """dst[tap][k/4][n][k%4] = src for k < K, n < N and exactly +0.0 on the padding to multiples of 64, whatever the buffer
    held before (NaN here); nothing behind the packed image is touched."""
    from lisec_amd import ops
    n = ops.packed_floats(ntaps, Kk, N)
    assert n == ntaps * (-(-Kk // 64) * 64) * (-(-N // 64) * 64)
    for name, src, (ts, ks, ns), w in _pack_sources(ntaps, Kk, N):
        dst = _nan(n + 64)
        ops.pack_weights(src, ntaps, Kk, N, ts, ks, ns, out=dst)
        torch.cuda.synchronize()
        want = torch.from_numpy(np.concatenate([R.packed_layout(w, 4), np.full(64, np.nan, np.float32)]))
        assert torch.equal(torch.isnan(dst.cpu()), torch.isnan(want)), name
        assert torch.equal(_bits(dst.cpu())[:n], _bits(want)[:n]), name


def test_pack_weights_batched_equals_the_single_packs():
    """Every case and source order in ONE table: bit-equal to the one-by-one packs, padding included (NaN before)."""
    from lisec_amd import ops
    entries, singles = [], []
    for ntaps, Kk, N in K.PACK_CASES:
        n = ops.packed_floats(ntaps, Kk, N)
        for name, src, (ts, ks, ns), w in _pack_sources(ntaps, Kk, N):
            entries.append((src, _nan(n), ntaps, Kk, N, ts, ks, ns))
            singles.append((ops.pack_weights(src, ntaps, Kk, N, ts, ks, ns, out=_nan(n)), R.packed_layout(w, 4)))
    ops.PackTable(entries, DEV).run()
    torch.cuda.synchronize()
    for e, (single, want) in zip(entries, singles):
        assert torch.equal(_bits(single.cpu()), _bits(torch.from_numpy(want)))
        assert torch.equal(_bits(e[1]), _bits(single))


@pytest.mark.parametrize("ntaps,Kk,N", K.PACK_CASES)
def test_pack_weights_bf16_rounds_to_nearest_even_and_zero_fills(ntaps, Kk, N):
    """dst[tap][k/8][n][k%8] bf16, bit-equal to torch's fp32 -> bfloat16 conversion (round to nearest, ties to even), +0
    on the padding.  The kernel's first values are exact halves of both parities, neighbours of a half, signed zeros,
    subnormals and the largest finite float (K.bf16_edge_values)."""
    from lisec_amd import ops
    for name, src, (ts, ks, ns), w in _pack_sources(ntaps, Kk, N, edge=K.bf16_edge_values()):
        nbytes = ops.packed_bf16_bytes(ntaps, Kk, N)
        dst = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)            # bf16 0xFFFF: a NaN
        ops.pack_weights_bf16(src, ntaps, Kk, N, ts, ks, ns, out=dst)
        torch.cuda.synchronize()
        rounded = torch.from_numpy(w).to(torch.bfloat16).view(torch.int16).numpy()
        want = R.packed_layout(rounded, 8)
        got = dst.cpu().view(torch.int16).numpy()
        bad = np.flatnonzero(got[:want.size] != want)
        assert bad.size == 0, f"{name}: {bad.size} differ, first at {bad[:4]}: got {got[bad[:4]]}, want {want[bad[:4]]}"
        assert (got[want.size:] == -1).all(), name


# ---- lisec_bn_finalize ----------------------------------------------------------------------------------------------------------
def _bn_bound(ref):
    return R.once_bound(ref) + 1e-9 * np.maximum(1.0, np.abs(ref))


@pytest.mark.parametrize("nparts", K.BN_NPARTS)
@pytest.mark.parametrize("C", K.BN_C)
def test_bn_finalize(C, nparts):
    """C = 24: columns 24..31 of the second workgroup are dead.  nparts 63 / 64 / 65: the 64 row groups; 512 / 513: the
    8-deep batched loop (b + 7*64 < nparts) runs for 0 / 1 row group; 1030: two batches for some and a tail.  Column 5 is
    a constant whose sums give a slightly NEGATIVE variance: it must clamp to 0, invstd = 1/sqrt(1e-3).  The moving
    statistics with and without N/(N-1); without both pointers nothing but bnstate is written."""
    from lisec_amd import ops
    d = K.bn_inputs(C, nparts, negative_var_column=5)
    N = K.BN_ROWS
    parts, gamma, beta = _dev(d["partials"].reshape(-1)), _dev(d["gamma"]), _dev(d["beta"])
    st = _nan(4 * C)
    ops.bn_finalize(parts, nparts, C, N, gamma, beta, None, None, True, st)
    ref = R.bn_finalize(d["partials"], N, d["gamma"], d["beta"])[0]
    assert ref[3 * C + 5] == 1 / np.sqrt(1e-3)
    _within(_host(st), ref, _bn_bound(ref), "bn_finalize bnstate")
    for unbiased in (False, True):
        mm, mv, st2 = _dev(d["moving_mean"]), _dev(d["moving_var"]), _nan(4 * C)
        ops.bn_finalize(parts, nparts, C, N, gamma, beta, mm, mv, unbiased, st2)
        _, rm, rv = R.bn_finalize(d["partials"], N, d["gamma"], d["beta"], d["moving_mean"], d["moving_var"], unbiased)
        assert torch.equal(_bits(st2), _bits(st))
        _within(_host(mm), rm, _bn_bound(rm), f"bn_finalize moving mean (unbiased={unbiased})")
        _within(_host(mv), rv, _bn_bound(rv), f"bn_finalize moving variance (unbiased={unbiased})")


def test_bn_finalize_of_one_row_does_not_divide_by_zero():
    """n_rows = 1: the batch variance is 0 and the unbiased factor N/(N-1) must not be formed."""
    from lisec_amd import ops
    C = 16
    d = K.bn_inputs(C, 1, rows=1)
    mm, mv, st = _dev(d["moving_mean"]), _dev(d["moving_var"]), _nan(4 * C)
    ops.bn_finalize(_dev(d["partials"].reshape(-1)), 1, C, 1, _dev(d["gamma"]), _dev(d["beta"]), mm, mv, True, st)
    ref, rm, rv = R.bn_finalize(d["partials"], 1, d["gamma"], d["beta"], d["moving_mean"], d["moving_var"], True)
    _within(_host(st), ref, _bn_bound(ref), "bn_finalize bnstate, one row")
    _within(_host(mm), rm, _bn_bound(rm), "bn_finalize moving mean, one row")
    _within(_host(mv), rv, _bn_bound(rv), "bn_finalize moving variance, one row")


def test_bn_finalize_rejects_one_moving_pointer_alone():
    from lisec_amd import _lib, ops
    C = 16
    d = K.bn_inputs(C, 1)
    m, st = torch.full((C,), SENTINEL, device=DEV), torch.full((4 * C,), SENTINEL, device=DEV)
    for mm, mv in ((m, None), (None, m)):
        with pytest.raises(_lib.LisecError):
            ops.bn_finalize(_dev(d["partials"].reshape(-1)), 1, C, K.BN_ROWS, _dev(d["gamma"]), _dev(d["beta"]), mm, mv, True, st)
    assert (_host(m) == SENTINEL).all() and (_host(st) == SENTINEL).all()


# ---- lisec_bn_fold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", K.BN_FOLD_C)
def test_bn_fold(C):
    """C = 100: the second 64-thread workgroup has 28 dead threads.  Moving variances from 1e-6 (eps decides) to 1e3."""
    from lisec_amd import ops
    d = K.bn_fold_inputs(C)
    mm, mv = _dev(d["moving_mean"]), _dev(d["moving_var"])
    st = _nan(4 * C)
    ops.bn_fold(_dev(d["gamma"]), _dev(d["beta"]), mm, mv, C, st)
    ref = R.bn_fold(d["gamma"], d["beta"], d["moving_mean"], d["moving_var"])
    _within(_host(st), ref, _bn_bound(ref), "bn_fold bnstate")
    assert np.array_equal(_host(mm), d["moving_mean"]) and np.array_equal(_host(mv), d["moving_var"])


# ---- lisec_scale ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0.5, 1.0 / 3.0])
@pytest.mark.parametrize("n", [4, 1028, 4 * (2 ** 20 + 1)])
def test_scale(n, s):
    """One float4, a ragged last workgroup (257 float4s), and 2^20 + 1 float4s > 1024 x 256: the grid-stride loop repeats.
    s is passed as the fp32 nearest to it, so the fp32 product is the exact value.  Sentinels sit behind the n elements."""
    from lisec_amd import ops
    x = torch.randn(n + 4, generator=torch.Generator().manual_seed(n))
    got = x.to(DEV)
    ops.scale_(got[:n], s)
    torch.cuda.synchronize()
    want = x.clone()
    want[:n] = x[:n] * torch.tensor(s, dtype=torch.float32)
    assert torch.equal(_bits(got.cpu()), _bits(want))


def test_scale_of_nothing_and_of_a_ragged_count():
    from lisec_amd import _lib
    x = torch.full((8,), SENTINEL, device=DEV)
    lib = _lib.load()
    _lib.check(lib.lisec_scale(_lib.ptr(x), 0, ctypes.c_float(0.5), _lib.current_stream()))          # n = 0: no-op
    with pytest.raises(_lib.LisecError):
        _lib.check(lib.lisec_scale(_lib.ptr(x), 6, ctypes.c_float(0.5), _lib.current_stream()))      # n % 4 != 0
    assert (_host(x) == SENTINEL).all()
