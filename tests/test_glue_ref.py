"""The fp64 references of the between-layer kernels (tests/glue_ref.py) against torch autograd, torch batch_norm and
oracle/conv_ref.py, and the reach of the rounding bounds on the inputs the GPU tests use (tests/glue_cases.py).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as K
import glue_ref as R
from oracle import conv_ref


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ---- the composite head ---------------------------------------------------------------------------------------------------
def _branch_graph(k, s, seed):
    """Conv2DTranspose(k, s, 'same') + the 1x1 heads of ONE branch in torch fp64, every variable a leaf."""
    g = torch.Generator().manual_seed(seed)
    cin, cup, h, w = 5, 7, 4, 6
    d = dict(x=torch.randn(1, cin, h, w, generator=g, dtype=torch.float64),
             W=torch.randn(k, k, cup, cin, generator=g, dtype=torch.float64).requires_grad_(True),   # Keras (kh,kw,out,in)
             bias=torch.randn(cup, generator=g, dtype=torch.float64).requires_grad_(True),
             H=torch.randn(cup, 16, generator=g, dtype=torch.float64).requires_grad_(True),
             b=torch.randn(16, generator=g, dtype=torch.float64))
    pad = (k - s) // 2
    up = F.conv_transpose2d(d["x"], d["W"].permute(3, 2, 0, 1), d["bias"], stride=s, padding=pad)      # (1, cup, h*s, w*s)
    d["head"] = up[0].permute(1, 2, 0) @ d["H"] + d["b"]                                               # (h*s, w*s, 16)
    d["pad"] = pad
    return d


@pytest.mark.parametrize("k,s", [(3, 1), (2, 2), (4, 4)])
def test_head_compose_reference_is_the_transposed_convolution_to_sixteen_channels(k, s):
    d = _branch_graph(k, s, 3 * k + s)
    W = d["W"].detach().numpy().reshape(k * k, *d["W"].shape[2:])
    Wc, _ = R.head_compose(W, d["H"].detach().numpy())
    bp, _ = R.head_compose_bias(d["bias"].detach().numpy(), d["H"].detach().numpy(), d["b"].numpy())
    kern = _t(Wc).reshape(k, k, -1, 16).permute(2, 3, 0, 1)                                            # (in, 16, kh, kw)
    got = F.conv_transpose2d(d["x"], kern, _t(bp), stride=s, padding=d["pad"])[0].permute(1, 2, 0)
    assert (got - d["head"].detach()).abs().max().item() <= 1e-12 * max(1.0, d["head"].abs().max().item())


@pytest.mark.parametrize("k,s", [(3, 1), (2, 2), (4, 4)])
def test_head_compose_backward_reference_equals_autograd(k, s):
    """G = dL/dWc comes from autograd through the 16-channel contraction; the reference must turn it and S into autograd's
    gradients of the ORIGINAL variables -- d_head_w only matches with its bias_b[n] * S[j] term."""
    d = _branch_graph(k, s, 5 * k + s)
    dhead = torch.randn(d["head"].shape, generator=torch.Generator().manual_seed(k), dtype=torch.float64)
    d["head"].backward(dhead)
    W = d["W"].detach().numpy().reshape(k * k, *d["W"].shape[2:])
    H, bias = d["H"].detach().numpy(), d["bias"].detach().numpy()
    Wc = _t(R.head_compose(W, H)[0]).requires_grad_(True)
    kern = Wc.reshape(k, k, -1, 16).permute(2, 3, 0, 1)
    F.conv_transpose2d(d["x"], kern, None, stride=s, padding=d["pad"])[0].permute(1, 2, 0).backward(dhead)
    S = dhead.sum((0, 1)).numpy()
    (dk, _), (dh, _), (db, _) = R.head_compose_backward(Wc.grad.numpy(), W, bias, H, S)
    for got, want in ((dk.reshape(d["W"].shape), d["W"].grad), (db, d["bias"].grad), (dh, d["H"].grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-12 * max(1.0, want.abs().max().item())
    without = R.head_compose_backward(Wc.grad.numpy(), W, None, H, S)[1][0]
    assert np.abs(without - d["H"].grad.numpy()).max() > 1e-3                   # the bias term is not optional


def test_head_shuffle_index_is_the_pixel_shuffle_of_a_kernel_equals_stride_branch():
    """A kernel == stride transposed convolution writes input position (h, w), tap (kh, kw) at (h*ps + kh, w*ps + kw)."""
    Ho, Wo, ps = 8, 12, 4
    pos, tap = R.head_shuffle_index(Ho, Wo, ps)
    for m in range(Ho * Wo):
        h, w = divmod(m, Wo)
        hi, wi = divmod(int(pos[m]), Wo // ps)
        kh, kw = divmod(int(tap[m]), ps)
        assert (hi * ps + kh, wi * ps + kw) == (h, w)


# ---- tap-inside sums and the constant-field gradients ---------------------------------------------------------------------
@pytest.mark.parametrize("ind,kernel,stride,pad", [((5, 6, 7), (3, 3, 3), (2, 1, 1), (1, 1, 1)),      # 3D, strided
                                                   ((1, 9, 10), (1, 3, 3), (1, 2, 2), (0, 1, 1))])    # 2D, strided
def test_const_field_reference_is_the_convolution_of_a_constant_map(ind, kernel, stride, pad):
    r = np.random.default_rng(ind[1])
    cin, cout = 6, 5
    outd = tuple((n + 2 * p - k) // s + 1 for n, p, k, s in zip(ind, pad, kernel, stride))
    taps = kernel[0] * kernel[1] * kernel[2]
    cvec, W = r.standard_normal(cin), r.standard_normal((taps, cin, cout))
    dy = r.standard_normal((*outd, cout))
    x = np.broadcast_to(cvec, (*ind, cin))
    S, A = R.tap_inside_sums(dy, ind, kernel, stride, pad)
    assert (A >= np.abs(S)).all()
    # the data gradient of the mode-0 convolution: the transposed gather of dy with K and N swapped
    dx = conv_ref.conv_forward(dy, W.transpose(0, 2, 1), ind, kernel, stride, pad, mode=1)
    g_all, _ = R.const_field_g_all(W, S)
    np.testing.assert_allclose(g_all, dx.reshape(-1, cin).sum(0), rtol=0, atol=1e-12 * np.abs(dx).sum())
    dW = conv_ref.conv_wgrad(x, dy, outd, kernel, stride, pad)
    np.testing.assert_allclose(R.const_field_dw(cvec, S), dW, rtol=0, atol=1e-12 * np.abs(dy).sum())
    old = r.standard_normal(dW.shape)
    np.testing.assert_array_equal(R.const_field_dw(cvec, S, old), old + R.const_field_dw(cvec, S))


# ---- the depth fold -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3])
def test_fold_depth_reference_is_permute_and_reshape(D):
    H, W, C = 3, 5, 4
    x = torch.arange(D * H * W * C, dtype=torch.float32).reshape(D, H, W, C)
    want = x.permute(1, 2, 3, 0).reshape(H, W, C * D)
    got = R.fold_depth(x.reshape(D, H * W, C).numpy())
    np.testing.assert_array_equal(got, want.reshape(H * W, C * D).numpy())
    assert got[7, 2 * D + (D - 1)] == x[D - 1].reshape(H * W, C)[7, 2]                  # channel c*D + d
    np.testing.assert_array_equal(R.unfold_depth(got, D), x.reshape(D, H * W, C).numpy())
    mask = np.where(np.arange(D * H * W * C).reshape(D, H * W, C) % 3 == 0, -1.0, 1.0).astype(np.float32)
    mask[0, 0, 1] = 0.0
    gated = R.unfold_depth(got, D, mask)
    np.testing.assert_array_equal(gated, np.where(mask > 0, x.reshape(D, H * W, C).numpy(), 0.0))
    assert gated[0, 0, 1] == 0.0 and not np.signbit(gated[0, 0, 1])


# ---- BatchNormalization -------------------------------------------------------------------------------------------------------
def test_bn_finalize_reference_is_torch_batch_norm_in_training_mode():
    C, nparts = 24, 65
    d = K.bn_inputs(C, nparts)
    y, N = _t(d["y"]), d["y"].shape[0]
    rm, rv = _t(d["moving_mean"]).clone(), _t(d["moving_var"]).clone()
    z = F.batch_norm(y, rm, rv, _t(d["gamma"]), _t(d["beta"]), training=True, momentum=1 - 0.99, eps=1e-3)
    st, mm, mv = R.bn_finalize(d["partials"], N, d["gamma"], d["beta"], d["moving_mean"], d["moving_var"], unbiased=True)
    scale, shift, mean, inv = st.reshape(4, C)
    np.testing.assert_allclose(y.numpy() * scale + shift, z.numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(mean, y.mean(0).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(inv, 1 / np.sqrt(y.var(0, unbiased=False).numpy() + 1e-3), rtol=1e-11)
    np.testing.assert_allclose(mm, rm.numpy(), rtol=0, atol=1e-12)               # torch updated them in place,
    np.testing.assert_allclose(mv, rv.numpy(), rtol=0, atol=1e-11)               # with the UNBIASED batch variance
    st0, mm0, mv0 = R.bn_finalize(d["partials"], N, d["gamma"], d["beta"], d["moving_mean"], d["moving_var"], unbiased=False)
    np.testing.assert_array_equal(st0, st)
    np.testing.assert_array_equal(mm0, mm)
    want = d["moving_var"].astype(np.float64) * 0.99 + y.var(0, unbiased=False).numpy() * 0.01
    np.testing.assert_allclose(mv0, want, rtol=0, atol=1e-11)
    assert (np.abs(mv - mv0) > 1e-8).all()                                       # N/(N-1) is visible: 0.01 * var / 2096
    assert R.bn_finalize(d["partials"], N, d["gamma"], d["beta"])[1:] == (None, None)


def test_bn_finalize_reference_at_the_edges():
    """One row: the unbiased factor N/(N-1) is not applied.  A constant column whose sums give a negative variance: 0."""
    d = K.bn_inputs(16, 1, rows=1)
    st, mm, mv = R.bn_finalize(d["partials"], 1, d["gamma"], d["beta"], d["moving_mean"], d["moving_var"], unbiased=True)
    assert np.isfinite(st).all() and np.isfinite(mv).all()
    np.testing.assert_allclose(mv, d["moving_var"].astype(np.float64) * 0.99, rtol=0, atol=1e-13)     # batch variance 0
    d = K.bn_inputs(16, 63, negative_var_column=5)
    s = d["partials"].sum(0)
    assert s[1, 5] / K.BN_ROWS - (s[0, 5] / K.BN_ROWS) ** 2 < 0                   # the draw does what it says
    st, _, _ = R.bn_finalize(d["partials"], K.BN_ROWS, d["gamma"], d["beta"])
    assert st.reshape(4, 16)[3, 5] == 1 / np.sqrt(1e-3)


@pytest.mark.parametrize("C", K.BN_FOLD_C)
def test_bn_fold_reference_is_torch_batch_norm_in_eval_mode(C):
    d = K.bn_fold_inputs(C)
    assert d["moving_var"].min() <= 1.01e-6 and d["moving_var"].max() >= 0.99e3
    x = torch.randn(50, C, generator=torch.Generator().manual_seed(C), dtype=torch.float64)
    z = F.batch_norm(x, _t(d["moving_mean"]), _t(d["moving_var"]), _t(d["gamma"]), _t(d["beta"]), training=False, eps=1e-3)
    scale, shift, mean, inv = R.bn_fold(d["gamma"], d["beta"], d["moving_mean"], d["moving_var"]).reshape(4, C)
    np.testing.assert_allclose(x.numpy() * scale + shift, z.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_array_equal(mean, d["moving_mean"].astype(np.float64))
    np.testing.assert_allclose(inv, 1 / np.sqrt(d["moving_var"].astype(np.float64) + 1e-3), rtol=1e-15)


# ---- the packed layouts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [4, 8])
def test_packed_layout_reference_is_the_index_formula_of_the_header(group):
    taps, Kk, N = 2, 70, 9
    w = np.arange(1, taps * Kk * N + 1, dtype=np.float32).reshape(taps, Kk, N)
    p = R.packed_layout(w, group).reshape(taps, 128 // group, 64, group)
    assert p.size == taps * 128 * 64
    for tap, k, n in [(0, 0, 0), (1, 69, 8), (0, 5, 3), (1, 64, 0), (0, 63, 8)]:
        assert p[tap, k // group, n, k % group] == w[tap, k, n]
    assert np.count_nonzero(p) == w.size and not np.signbit(p).any()             # the rest is +0.0


# ---- the bounds reach the inputs: an fp32 evaluation in ANOTHER order stays inside, a dropped term does not ---------------
def _f32_sum_reversed(terms):
    """fp32 running sum of terms[..., i] from the LAST index down (the references sum in fp64, pairwise or by BLAS)."""
    acc = np.zeros(terms.shape[:-1], dtype=np.float32)
    for i in range(terms.shape[-1] - 1, -1, -1):
        acc = acc + terms[..., i]
    return acc


@pytest.mark.parametrize("taps,cin,cup", K.HEAD_CASES)
def test_sum_bounds_hold_for_an_fp32_evaluation_in_another_order(taps, cin, cup):
    d = K.head_inputs(taps, cin, cup)
    W, H, G, S, b = d["up_kernel"], d["head_w"], d["G"], d["S"], d["up_bias"]
    Wc, A = R.head_compose(W, H)
    got = _f32_sum_reversed(W.transpose(0, 2, 1)[:, :, None, :] * H.T[None, None])          # (taps, Cin, 16, Cup)
    assert (np.abs(got - Wc) <= R.sum_bound(cup, A)).all()
    # a dropped row (n < Cup - 1) is far outside: the bound is not vacuous
    dropped = np.abs(W[:, cup - 1, :, None].astype(np.float64) * H[cup - 1].astype(np.float64))
    assert np.median(dropped / R.sum_bound(cup, A)) > 30
    bp, Ab = R.head_compose_bias(b, H, d["bias_in"])
    got = _f32_sum_reversed(np.concatenate([b[None, :] * H.T, d["bias_in"][:, None]], axis=1))
    assert (np.abs(got - bp) <= R.sum_bound(cup + 1, Ab)).all()
    (dk, Ak), (dh, Ah), (db, Adb) = R.head_compose_backward(G, W, b, H, S)
    got = _f32_sum_reversed(G[:, None, :, :] * H[None, :, None, :])                           # (taps, Cup, Cin, 16)
    assert (np.abs(got - dk) <= R.sum_bound(16, Ak)).all()
    terms = np.concatenate([(W[:, :, :, None] * G[:, None, :, :]).transpose(1, 3, 0, 2).reshape(cup, 16, taps * cin),
                            (b[:, None] * S[None, :])[:, :, None]], axis=2)
    assert (np.abs(_f32_sum_reversed(terms) - dh) <= R.sum_bound(taps * cin + 1, Ah)).all()
    assert np.median(np.abs(np.outer(b, S)) / R.sum_bound(taps * cin + 1, Ah)) > 1000         # the bias term, if missing
    assert (np.abs(_f32_sum_reversed(H * S[None, :]) - db) <= R.sum_bound(16, Adb)).all()


@pytest.mark.parametrize("ntaps,cin,cout", K.CONST_FIELD_CASES[:2])
def test_once_rounded_bounds_hold_for_fp64_evaluations_in_another_order(ntaps, cin, cout):
    d = K.const_field_inputs(ntaps, cin, cout)
    g_all, A = R.const_field_g_all(d["W"], d["S"])
    other = np.zeros(cin)
    for t in range(ntaps - 1, -1, -1):                                            # fp64, taps from the last down
        other += d["W"][t].astype(np.float64) @ d["S"][t].astype(np.float64)
    assert (np.abs(other.astype(np.float32) - g_all) <= R.once_bound(g_all) + 1e-12 * A).all()
    cvec = d["table"][1]
    dW = R.const_field_dw(cvec, d["S"], d["dW_old"])
    fma = (d["dW_old"].astype(np.float64) + cvec.astype(np.float64)[None, :, None] * d["S"].astype(np.float64)[:, None, :])
    assert (np.abs(fma.astype(np.float32) - dW) <= R.once_bound(dW)).all()        # one fma = one rounding of the fp64 value


@pytest.mark.parametrize("nparts", [1, 65, 1030])
def test_bn_bound_holds_for_a_differently_ordered_fp64_reduction(nparts):
    C = 24
    d = K.bn_inputs(C, nparts, negative_var_column=7)
    s = np.zeros((2, C))
    for p in d["partials"][::-1]:
        s += p
    mean = s[0] / K.BN_ROWS
    var = np.maximum(s[1] / K.BN_ROWS - mean * mean, 0.0)
    assert np.abs(mean).max() <= 3.0 + 1e-6 and np.delete(var, 7).min() >= 0.1
    other = R.bn_state(mean, var, d["gamma"], d["beta"]).astype(np.float32)
    ref = R.bn_finalize(d["partials"], K.BN_ROWS, d["gamma"], d["beta"])[0]
    assert (np.abs(other - ref) <= R.once_bound(ref) + 1e-9 * np.maximum(1.0, np.abs(ref))).all()
