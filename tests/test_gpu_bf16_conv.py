"""The bf16-MFMA inference contraction (lisec_conv_forward_bf16, csrc/igemm_bf16.hip) against fp64 CPU convolutions.

The kernel's contract: fp32 buffers; the gathered value gets affine + ReLU in fp32, is rounded to bf16 to nearest-even,
the kernel likewise; products (exact in fp32) are accumulated in fp32; bias and the output ReLU are fp32.  Three checks
per geometry, each with a tolerance that does not come from the kernel:
  1. operands that ARE bf16 values: only fp32 summation order is left, so the fp32 kernels' tolerance
     (tests/test_gpu_conv.py::_close: rtol 1e-4, atol 1e-4 * max|ref|) holds against the fp64 convolution;
  2. general operands: the same tolerance against the fp64 convolution of torch's RNE-rounded operands (the rounding of
     x applied after affine + ReLU) -- a truncating conversion misses it by ~2^-9;
  3. against the unrounded fp64 result: |got - ref| <= (2u + u^2) (|x| conv |w|) + 1e-4 max|ref|, u = 2^-9 (each operand
     carries one relative rounding of at most u, so each product at most 2u + u^2).
Geometries: those of test_gpu_conv.py::test_conv3d_mid_layers / ::test_conv2d_rpn_layers plus Lyft-sized RPN maps, and two
with a channel count that is no multiple of 64 (RAGGED_CASES).  Every kernel is packed over a NaN-filled buffer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -9

# (D, H, W, Cin, Cout, k, stride, pad, in_bn(+IN_RELU), out_relu, bias, seed)
CASES = [
    (8, 12, 20, 64, 64, (3, 3, 3), (2, 1, 1), (1, 1, 1), False, False, True, 0),
    (4, 12, 20, 64, 64, (3, 3, 3), (1, 1, 1), (0, 1, 1), False, True, True, 1),
    (2, 9, 21, 64, 64, (3, 3, 3), (2, 1, 1), (1, 1, 1), False, False, False, 2),          # ragged M (189)
    (1, 24, 40, 64, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1), False, False, True, 0),
    (1, 12, 20, 128, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1), True, False, True, 3),
    (1, 7, 13, 128, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1), True, True, True, 4),
    (1, 5, 7, 256, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1), True, False, False, 5),
    (1, 50, 100, 128, 128, (1, 3, 3), (1, 1, 1), (0, 1, 1), True, False, True, 6),       # Lyft RPN block 2: 5 000 rows, K-sliced
    (1, 50, 100, 128, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1), True, False, True, 7),       # Lyft RPN block 3: 1 250 rows, K-sliced
]
IDS = ["mid_s2", "mid_p0_orelu", "mid_ragged_nobias", "rpn_s2_64", "rpn_128_bn", "rpn_s2_256_bn_orelu", "rpn_256_bn_nobias",
       "lyft_rpn2", "lyft_rpn3"]
# Channel counts that are no multiple of 64: the only reason the packed kernel is zero padded.  They go through the three
# operand checks below (the list above is also indexed by position).
RAGGED_CASES = [
    (2, 6, 20, 80, 64, (3, 3, 3), (2, 1, 1), (1, 1, 1), True, False, True, 8),           # Cin 80: the second 64-channel slab is a quarter full
    (1, 9, 21, 64, 40, (1, 3, 3), (1, 1, 1), (0, 1, 1), False, True, True, 9),           # Cout 40: the second 32-column accumulator is partly dead
]
RAGGED_IDS = ["mid_cin80_bn", "rpn_cout40_orelu"]
ALL_CASES, ALL_IDS = CASES + RAGGED_CASES, IDS + RAGGED_IDS


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _conv64(x, w, b, stride, pad):
    """fp64 convolution; x (D,H,W,Cin), w Keras (kd,kh,kw,in,out) -> (Do,Ho,Wo,Cout)."""
    y = F.conv3d(x.double().permute(3, 0, 1, 2)[None], w.double().permute(4, 3, 0, 1, 2),
                 None if b is None else b.double(), stride=stride, padding=pad)[0]
    return y.permute(1, 2, 3, 0)


def _close(got, ref, what, rtol=1e-4):
    got, ref = got.double().cpu(), ref.double().cpu()
    atol = rtol * ref.abs().max().item()
    err = (got - ref).abs()
    print(f"{what}: max err {err.max().item():.3e}, atol {atol:.3e}, max|ref| {ref.abs().max().item():.3e}")
    assert (err <= atol + rtol * ref.abs()).all(), f"{what}: max err {err.max().item():.3e}, atol {atol:.3e}"


def _draw(case, exact_affine):
    """x, w, bias, (scale, shift) on the CPU.  exact_affine: x and the shifts are multiples of 2^-6 in [-4, 4] and the
    scales powers of two, so that x*scale + shift is exact in fp32 whether it is one fma or two operations (a one-ulp
    difference there would flip a bf16 rounding for no fault of the kernel) and still needs more than 8 bits."""
    D, H, W, Cin, Cout, k, stride, pad, in_bn, out_relu, bias, seed = case
    g = torch.Generator().manual_seed(seed)
    if in_bn and exact_affine:
        x = torch.randint(-256, 257, (D, H, W, Cin), generator=g).float() / 64
        sc = 2.0 ** torch.randint(-1, 2, (Cin,), generator=g).float() * (torch.randint(0, 2, (Cin,), generator=g).float() * 2 - 1)
        sh = torch.randint(-256, 257, (Cin,), generator=g).float() / 64
    else:
        x = torch.randn(D, H, W, Cin, generator=g)
        sc, sh = torch.randn(Cin, generator=g), torch.randn(Cin, generator=g)
    w = torch.randn(*k, Cin, Cout, generator=g) * 0.1
    b = torch.randn(Cout, generator=g) if bias else None
    return x, w, b, ((sc, sh) if in_bn else None)


def _run(case, x, w, b, bn, splitk=True, in_relu=None):
    """in_relu: LISEC_CONV_IN_RELU; by default it goes with in_bn, as in the network."""
    from lisec_amd import ops
    D, H, W, Cin, Cout, k, stride, pad, in_bn, out_relu, bias, seed = case
    Do, Ho, Wo = ((n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((D, H, W), pad, k, stride))
    geo = ops.geom(0, (D, H, W), (Do, Ho, Wo), k, stride, pad, Cin, Cout)
    ntaps = k[0] * k[1] * k[2]
    # packed over NaNs (bf16 0xFFFF): the zero padding of ragged Cin / Cout is the pack's to write
    wp = torch.full((ops.packed_bf16_bytes(ntaps, Cin, Cout),), 0xFF, dtype=torch.uint8, device=DEV)
    ops.pack_weights_bf16(w.to(DEV), ntaps, Cin, Cout, Cin * Cout, Cout, 1, out=wp)
    out = torch.full((Do, Ho, Wo, Cout), float("nan"), device=DEV)
    bnstate = None if bn is None else torch.cat([bn[0], bn[1], torch.zeros(2 * Cin)]).to(DEV)
    flags = (ops.IN_RELU if (in_bn if in_relu is None else in_relu) else 0) | (ops.OUT_RELU if out_relu else 0)
    ops.conv_forward_bf16(geo, x.to(DEV), wp, out, bias=None if b is None else b.to(DEV), in_bn=bnstate, flags=flags,
                          splitk=splitk)
    torch.cuda.synchronize()
    return out


def _activated(x, bn, relu=True):
    """The fp32 value the kernel rounds: relu(fma(x, scale, shift)); fp64 here, compared where that is exact or bounded."""
    if bn is None:
        return x.double()
    a = x.double() * bn[0].double() + bn[1].double()
    return F.relu(a) if relu else a


@pytest.mark.parametrize("case", [c for c in ALL_CASES if not c[8]], ids=[i for c, i in zip(ALL_CASES, ALL_IDS) if not c[8]])
def test_representable_operands_leave_only_fp32_summation(case):
    x, w, b, bn = _draw(case, True)
    x, w = _bf16(x), _bf16(w)
    ref = _conv64(x, w, b, case[6], case[7])
    if case[9]:
        ref = F.relu(ref)
    _close(_run(case, x, w, b, bn), ref, "bf16-representable operands")


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_operands_are_rounded_to_nearest_even(case):
    x, w, b, bn = _draw(case, True)
    a = _activated(x, bn)
    assert torch.equal(a.float().double(), a)                    # the affine is exact in fp32: no double rounding
    if bn is not None:
        assert (_bf16(a.float()).double() != a).float().mean() > 0.05     # and the rounding has work to do
    ref = _conv64(_bf16(a.float()), _bf16(w), b, case[6], case[7])
    if case[9]:
        ref = F.relu(ref)
    _close(_run(case, x, w, b, bn), ref, "RNE-rounded operands")


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_a_priori_bound_against_the_unrounded_result(case):
    x, w, b, bn = _draw(case, False)
    a = _activated(x, bn)
    ref = _conv64(a, w, b, case[6], case[7])
    mag = _conv64(a.abs(), w.abs(), None, case[6], case[7])
    if case[9]:
        ref = F.relu(ref)                                        # 1-Lipschitz: the bound carries over
    got = _run(case, x, w, b, bn).double().cpu()
    err = (got - ref).abs()
    bound = (2 * U + U * U) * mag + 1e-4 * ref.abs().max()
    print(f"a-priori bound: max err {err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}, "
          f"max|ref| {ref.abs().max().item():.3e}")
    assert (err <= bound).all(), f"max err/bound {(err / bound).max().item():.3f}"


def test_in_bn_without_in_relu_is_the_affine_alone():
    """in_bnstate without LISEC_CONV_IN_RELU (relu_lo = -inf): every other case sets the two together.  The exact-affine draw
    on the rpn_128_bn geometry: about half of the affine's values are negative and must reach the contraction."""
    case = CASES[4]
    x, w, b, bn = _draw(case, True)
    a = _activated(x, bn, relu=False)
    assert torch.equal(a.float().double(), a) and 0.3 < (a < 0).float().mean() < 0.7
    assert (_bf16(a.float()).double() != a).float().mean() > 0.05
    ref = _conv64(_bf16(a.float()), _bf16(w), b, case[6], case[7])
    _close(_run(case, x, w, b, bn, in_relu=False), ref, "RNE-rounded operands, affine without ReLU")


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[7], CASES[8]], ids=["mid_s2", "rpn_128_bn", "lyft_rpn2", "lyft_rpn3"])
def test_two_calls_give_equal_bits_and_slices_change_only_summation_order(case):
    x, w, b, bn = _draw(case, False)
    one = _run(case, x, w, b, bn)
    two = _run(case, x, w, b, bn)
    assert torch.equal(one, two)
    unsliced = _run(case, x, w, b, bn, splitk=False)
    _close(one, unsliced, "K-sliced vs one pass")


def test_the_lyft_rpn_maps_are_k_sliced():
    """The determinism test above must cover slices that meet: the plan of the two Lyft-sized cases asks for a workspace."""
    import ctypes
    from lisec_amd import _lib, ops
    for case in CASES[7:]:
        D, H, W, Cin, Cout, k, stride, pad = case[:8]
        Do, Ho, Wo = ((n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((D, H, W), pad, k, stride))
        geo = ops.geom(0, (D, H, W), (Do, Ho, Wo), k, stride, pad, Cin, Cout)
        assert _lib.load().lisec_conv_forward_bf16_workspace_bytes(ctypes.byref(geo)) > 0


def test_unserved_geometry_is_an_error_not_an_fp32_run():
    from lisec_amd import _lib, ops
    x = torch.randn(1, 8, 8, 64, device=DEV)
    wp = ops.pack_weights_bf16(torch.randn(9, 64, 64, device=DEV), 9, 64, 64, 64 * 64, 64, 1)
    out = torch.full((1, 16, 16, 64), 7.0, device=DEV)
    transposed = ops.geom(1, (1, 8, 8), (1, 16, 16), (1, 3, 3), (1, 2, 2), (0, 1, 1), 64, 64)
    with pytest.raises(_lib.LisecError):
        ops.conv_forward_bf16(transposed, x, wp, out)
    shuffled = ops.geom(0, (1, 8, 8), (1, 8, 8), (1, 1, 1), (1, 1, 1), (0, 0, 0), 64, 4 * 64, out_stride=64, ps=2, ps_channels=64)
    with pytest.raises(_lib.LisecError):
        ops.conv_forward_bf16(shuffled, x, wp, out)
    fwd = ops.geom(0, (1, 8, 8), (1, 8, 8), (1, 3, 3), (1, 1, 1), (0, 1, 1), 64, 64)
    with pytest.raises(_lib.LisecError):
        ops.conv_forward_bf16(fwd, x, wp, out[:, :8, :8].contiguous(), flags=ops.ACCUMULATE)
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                    # nothing ran
