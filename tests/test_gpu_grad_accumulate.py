"""lisec_grad_accumulate alone (csrc/grad_accumulate.hip): begin, two adds and end over five ranges of one buffer, bit
for bit against the same sequence of numpy.float32 operations -- the contract of include/lisec_hip.h: fp32 adds in call
order, then ONE fp32 multiply by the device scale, never contracted; floats outside the ranges and the buffer a form only
reads keep their bits; malformed arguments are LISEC_EINVAL with nothing enqueued."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (offset, length) in floats: offsets are multiples of 4 with gaps between the ranges; the lengths straddle one workgroup
# pass (256 threads x 4 floats = 1024), 4096 and its neighbours, and 3*4096 + 8 (several blocks with a ragged end)
RANGES = [(8, 4), (20, 4092), (4120, 4096), (8224, 4100), (12332, 3 * 4096 + 8)]
TOTAL = 12332 + 3 * 4096 + 8 + 12


def _values(seed):
    """Both signs, exact zeros of both signs, one denormal, magnitudes spread over 2^-20 .. 2^20."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(TOTAL) * np.exp2(rng.integers(-20, 21, TOTAL))).astype(np.float32)
    v[rng.integers(0, TOTAL, TOTAL // 16)] = 0.0
    v[rng.integers(0, TOTAL, TOTAL // 64)] = -0.0
    for off, n in RANGES:
        v[off] = -0.0                                      # (-0) + (-0) = -0, and -0 * s = -0: begin must not start from +0
        v[off + 1] = 0.0 if seed % 2 else -0.0             # zeros of a sign that varies by sweep
        v[off + n - 1] = np.float32(1e-41) * (seed + 1)    # a denormal at the end of every range; the sums stay denormal
    return v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("divisor", [4, 3])
def test_begin_add_add_end_matches_numpy_float32_bit_for_bit(divisor):
    import torch
    from lisec_amd import _lib, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    sweeps = [_values(s) for s in range(4)]
    s32 = np.float32(1.0) / np.float32(divisor)
    scale = torch.tensor([float(s32)], dtype=torch.float32, device=dev)
    acc0 = _values(99)                                     # what the accumulator held before: begin overwrites it
    g = torch.from_numpy(sweeps[0].copy()).to(dev)
    acc = torch.from_numpy(acc0.copy()).to(dev)
    want_acc, want_g = acc0.copy(), None
    for k, (sweep, mode) in enumerate(zip(sweeps, (_lib.ACC_BEGIN, _lib.ACC_ADD, _lib.ACC_ADD, _lib.ACC_END))):
        g.copy_(torch.from_numpy(sweep))                   # the backward of sweep k wrote its gradient
        for off, n in RANGES:
            ops.grad_accumulate(g[off:off + n], acc[off:off + n], mode, scale)
        torch.cuda.synchronize()
        if mode != _lib.ACC_END:
            assert np.array_equal(_bits(g.cpu().numpy()), _bits(sweep)), "begin / add must only read the gradient"
        for off, n in RANGES:
            sl = slice(off, off + n)
            if mode == _lib.ACC_BEGIN:
                want_acc[sl] = sweep[sl]
            elif mode == _lib.ACC_ADD:
                want_acc[sl] = want_acc[sl] + sweep[sl]                    # numpy.float32 + numpy.float32: one rounding
            else:
                want_g = sweep.copy()
                for off2, n2 in RANGES:
                    sl2 = slice(off2, off2 + n2)
                    want_g[sl2] = (want_acc[sl2] + sweep[sl2]) * s32       # the add rounded, then the multiply rounded
                break
        assert want_acc.dtype == np.float32
        assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want_acc)), f"acc after call {k}"
    got = g.cpu().numpy()
    assert want_g.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want_g))
    # the multiply did round for 1/3 (the test would not see a contracted or reassociated form otherwise)
    inside = np.concatenate([np.arange(off, off + n) for off, n in RANGES])
    exact = (want_acc[inside].astype(np.float64) + sweeps[3][inside].astype(np.float64)) * np.float64(s32)
    if divisor == 3:
        assert np.count_nonzero(exact != want_g[inside].astype(np.float64)) > len(inside) // 4
    # floats outside the ranges kept their bits in both buffers (checked above for acc; here for the gradient)
    outside = np.ones(TOTAL, bool)
    outside[inside] = False
    assert outside.sum() == TOTAL - sum(n for _, n in RANGES) > 0
    assert np.array_equal(_bits(got[outside]), _bits(sweeps[3][outside]))
    # the denormals and signed zeros went through as IEEE says
    assert np.any((np.abs(want_g[inside]) < np.finfo(np.float32).tiny) & (want_g[inside] != 0))
    assert np.any(np.signbit(want_g[inside]) & (want_g[inside] == 0))


def test_the_scale_is_read_from_the_device_when_the_kernel_runs():
    import torch
    from lisec_amd import _lib, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    a, b = _values(5)[:4096], _values(6)[:4096]
    scale = torch.tensor([0.5], dtype=torch.float32, device=dev)
    outs = []
    for s in (0.5, 0.125):
        g, acc = torch.from_numpy(b.copy()).to(dev), torch.from_numpy(a.copy()).to(dev)
        scale.fill_(s)                                     # same address, new contents: what a recorded plan relies on
        ops.grad_accumulate(g, acc, _lib.ACC_END, scale)
        torch.cuda.synchronize()
        outs.append(g.cpu().numpy())
        assert np.array_equal(_bits(outs[-1]), _bits((a + b) * np.float32(s)))
    assert not np.array_equal(outs[0], outs[1])


def test_malformed_arguments_are_einval_and_enqueue_nothing():
    import torch
    from lisec_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, s = _lib.load(), _lib.current_stream()
    g0 = _values(1)[:64]
    g = torch.from_numpy(g0.copy()).to(dev)
    acc = torch.from_numpy(_values(2)[:64].copy()).to(dev)
    acc0 = acc.cpu().numpy().copy()
    scale = torch.ones(1, dtype=torch.float32, device=dev)
    P = lambda t, byte_offset=0: t.data_ptr() + byte_offset      # noqa: E731
    E = -1                                                       # LISEC_EINVAL
    bad = [
        (P(g), P(acc), 6, _lib.ACC_ADD, P(scale)),               # n % 4
        (P(g), P(acc), -4, _lib.ACC_ADD, P(scale)),              # n < 0
        (P(g, 4), P(acc), 8, _lib.ACC_ADD, P(scale)),            # grad misaligned
        (P(g), P(acc, 8), 8, _lib.ACC_ADD, P(scale)),            # acc misaligned
        (P(g), P(acc), 8, 3, P(scale)),                          # unknown form
        (P(g), P(acc), 8, _lib.ACC_END, None),                   # end without the scale
        (None, P(acc), 8, _lib.ACC_BEGIN, None),
        (P(g), None, 8, _lib.ACC_BEGIN, None),
        (P(g), P(g), 8, _lib.ACC_ADD, None),                     # one buffer for both
    ]
    for args in bad:
        rc = lib.lisec_grad_accumulate(*args, s)
        assert rc == E, args
    assert lib.lisec_grad_accumulate(P(g), P(acc), 0, _lib.ACC_ADD, None, s) == 0      # n == 0: valid, nothing to do
    torch.cuda.synchronize()
    assert np.array_equal(_bits(g.cpu().numpy()), _bits(g0)) and np.array_equal(_bits(acc.cpu().numpy()), _bits(acc0))
