"""The K loop of k_wino (csrc/wino.hip) splits its side work between the two waves of a SIMD: waves 4-7 move the raw window and
the U image, waves 0-3 read, gate and transform the patches.  Layer-local cases through ops.conv_forward_winograd against the
fp64 restatement oracle/conv_ref.py with the bound of tests/test_gpu_winograd.py (relative L2 <= 2e-6, forward and data
gradient), at geometries that exercise what moved between the halves:
  * interior blocks (no gate) and edge blocks (gated) in one launch,
  * odd H and W: pmask gates inside the last tile,
  * Cin = 16: one two-chunk window group, the loop runs once and the window is never reloaded,
  * Cin = 128, Cout = 128: eight window groups per depth tap, two column blocks of U images,
  * KD = 3 with planes that have fewer live depth taps: the walks skip dead taps, one launch per tap count,
each without and with BatchNormalization + ReLU on load, and with LISEC_CONV_ACCUMULATE and the out_mask gate.
Inputs are built on the CPU from a fixed seed."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-6

# name, mode, in dims, out dims, KD, depth stride, depth pad, cin, cout
CASES = [
    ("interior and edge blocks 40x72", 0, (1, 40, 72), (1, 40, 72), 1, 1, 0, 32, 64),
    ("odd map 37x53", 0, (1, 37, 53), (1, 37, 53), 1, 1, 0, 32, 64),
    ("cin 16, one window group", 0, (1, 40, 72), (1, 40, 72), 1, 1, 0, 16, 64),
    ("cin 128 cout 128, two column blocks", 0, (1, 24, 40), (1, 24, 40), 1, 1, 0, 128, 128),
    ("3d depth pad 1: planes with 2 and 3 live taps", 0, (4, 20, 36), (4, 20, 36), 3, 1, 1, 32, 64),
    ("3d depth stride 2 pad 1: 2 of 3 taps live", 0, (2, 21, 35), (1, 21, 35), 3, 2, 1, 16, 64),
    ("data gradient 40x72", 1, (1, 40, 72), (1, 40, 72), 1, 1, 0, 32, 64),
    ("data gradient odd map, cin 128 cout 128", 1, (1, 19, 37), (1, 19, 37), 1, 1, 0, 128, 128),
    ("data gradient 3d valid depth: 1, 2, 2, 1 live taps", 1, (2, 20, 36), (4, 20, 36), 3, 1, 0, 16, 64),
    ("data gradient 3d depth stride 2 pad 1", 1, (1, 21, 35), (2, 21, 35), 3, 2, 1, 32, 72),
]


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def build(name, mode, ind, outd, KD, sd, pd, cin, cout, xf, dev):
    """operands (CPU, fixed seed), their device copies and the fp64 result"""
    from lisec_amd import ops
    from oracle import conv_ref
    rng = np.random.default_rng(zlib.crc32(f"staging {name} {xf}".encode()))
    k, s, p = (KD, 3, 3), (sd, 1, 1), (pd, 1, 1)
    ntaps = KD * 9
    x = rng.normal(0, 1, (*ind, cin)).astype(np.float32)
    Wt = (rng.normal(0, 1, (ntaps, cin, cout)) / np.sqrt(ntaps * cin)).astype(np.float32)
    b = rng.normal(0, 0.1, cout).astype(np.float32)
    bn_dev, bn_ref = None, None
    if xf:
        st = np.concatenate([rng.uniform(0.5, 1.5, cin), rng.normal(0, 0.3, cin), rng.normal(0, 0.2, cin),
                             rng.uniform(0.7, 1.4, cin)]).astype(np.float32)
        bn_dev, bn_ref = torch.from_numpy(st).to(dev), (st[:cin].astype(np.float64), st[cin:2 * cin].astype(np.float64))
    g = ops.geom(mode, ind, outd, k, s, p, cin, cout)
    wu = ops.pack_weights_winograd(torch.from_numpy(Wt).to(dev), KD, cin, cout, cin * cout, cout, 1, flip=(mode == 1))
    ref = conv_ref.conv_forward(x, Wt, outd, k, s, p, mode=mode, bias=b, in_bn=bn_ref, relu=xf)
    return g, torch.from_numpy(x).to(dev), torch.from_numpy(b).to(dev), bn_dev, wu, ref, rng


@pytest.mark.parametrize("xf", [False, True], ids=["plain", "bn-relu-on-load"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_split_staging_against_the_oracle(case, xf):
    from lisec_amd import ops
    name, mode, ind, outd, KD, sd, pd, cin, cout = case
    dev = torch.device("cuda")
    g, x, b, bn_dev, wu, ref, _ = build(*case, xf, dev)
    flags = ops.IN_RELU if xf else 0
    assert ops.winograd_supported(g, in_bn=xf, flags=flags)
    out = torch.full((*outd, cout), float("nan"), device=dev)
    ops.conv_forward_winograd(g, x, wu, out, bias=b, in_bn=bn_dev, flags=flags)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), f"{name}: positions left unwritten"
    e = rel_l2(got, ref)
    print(f"{name} (bn + relu on load: {xf}): relative L2 {e:.2e}")
    assert e <= TOL, f"{name}: relative L2 {e:.2e}"


ACC_CASES = [CASES[0], CASES[4], CASES[7], CASES[8]]


@pytest.mark.parametrize("xf", [False, True], ids=["plain", "bn-relu-on-load"])
@pytest.mark.parametrize("case", ACC_CASES, ids=[c[0] for c in ACC_CASES])
def test_split_staging_accumulate_and_gate(case, xf):
    """LISEC_CONV_ACCUMULATE onto an existing tensor and the out_mask gate: (+ bias, + previous, gate) in that order."""
    from lisec_amd import ops
    name, mode, ind, outd, KD, sd, pd, cin, cout = case
    dev = torch.device("cuda")
    g, x, b, bn_dev, wu, ref, rng = build(*case, xf, dev)
    prev = rng.normal(0, 1, ref.shape).astype(np.float32)
    act = rng.normal(0, 1, ref.shape).astype(np.float32)
    flags = ops.ACCUMULATE | (ops.IN_RELU if xf else 0)
    out = torch.from_numpy(prev.copy()).to(dev)
    ops.conv_forward_winograd(g, x, wu, out, bias=b, in_bn=bn_dev, flags=flags, out_mask=torch.from_numpy(act).to(dev))
    torch.cuda.synchronize()
    want = np.where(act > 0, ref + prev.astype(np.float64), 0.0)
    e = rel_l2(out.cpu().numpy(), want)
    print(f"{name} accumulate + gate (bn + relu on load: {xf}): relative L2 {e:.2e}")
    assert e <= TOL, f"{name}: relative L2 {e:.2e}"
