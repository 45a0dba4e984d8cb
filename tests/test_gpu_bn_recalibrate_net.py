"""LisecNet.recalibrate_batchnorm on the small grid (LisecNet(16, 32, 8, 35), randomised BatchNormalization variables,
three sweeps of 3000 points and an empty one): the numpy definition bit for bit over what the forward itself leaves in
a zeroed buffer; one sweep against the batch statistics the same forward reports (derived bounds: this is what tells a
wrong coefficient); the fp64 oracle; nothing of training moves; a failure restores the statistics."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_recalibrate_ref as R  # noqa: E402
from test_gpu_network import SMALL, small_cloud  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BN_EPS = 1e-3
# Largest relative error of a recalibrated variance against the fp64 oracle, |got - ref| / ref over every channel of
# every layer and both rules, measured on the MI355X (this file's sweeps and weights): MEASURED_VAR_ERR.  The test
# asserts 4x that -- the margin for other seeds and sweeps on a toy grid -- and never more than 1e-2.
MEASURED_VAR_ERR = 2.33e-5                           # 'mean' 2.18e-5, 'pooled' 2.33e-5
VAR_BOUND = min(4 * MEASURED_VAR_ERR, 1e-2)


def close(got, ref, rtol=1e-3, what=""):
    """The activation bound of tests/test_gpu_network.py, copied."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    atol = rtol * np.abs(ref).max()
    err = np.abs(got - ref)
    assert (err <= atol + rtol * np.abs(ref)).all(), f"{what}: max err {err.max():.3e}, atol {atol:.3e}"
    return err.max() / max(np.abs(ref).max(), 1e-30)


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def _table(net):
    """The net's table as the rows the definition takes: (mean_off, var_off, C, coef)."""
    table = net.bn_recal_table()[0]
    return [(r.mean_off, r.var_off, r.C, r.coef) for r in table.records[:table.n_entries]]


class _Setup:
    def __init__(self):
        from lisec_amd.network import LisecNet
        from lisec_amd.params import ParamStore
        from lisec_amd.voxelizer import Voxelizer
        from oracle import model_ref as M
        self.M = M
        self.op = M.glorot_params(seed=21, randomize_bn=True)
        self.dev = torch.device("cuda")
        self.vox = Voxelizer(**SMALL)
        self.points = [small_cloud(seed) for seed in (1, 2, 3)] + [np.zeros((0, 3), np.float32)]
        self.samples = [self.vox(p) for p in self.points]
        self.net = LisecNet(16, 32, 8, 35, params=ParamStore(self.dev, init=self.op))
        self.table = _table(self.net)
        self.initial = _host(self.net.params.state)
        # what each sweep's training forward leaves in a zeroed buffer, read once and shared
        self.states = []
        for s in self.samples:
            self.net.params.state.zero_()
            self.net.forward(s, training=True)
            self.states.append(_host(self.net.params.state))
        self.net.params.state.copy_(torch.from_numpy(self.initial))
        self.net.state_version += 1

    def fresh_net(self, init=None):
        from lisec_amd.network import LisecNet
        from lisec_amd.params import ParamStore
        return LisecNet(16, 32, 8, 35, params=ParamStore(self.dev, init=init if init is not None else self.op))


@pytest.fixture(scope="module")
def setup():
    return _Setup()


def test_the_table_covers_every_layer(setup):
    from lisec_amd import _lib
    lib = _lib.load()
    t = setup.table
    assert len(t) == 22 and sum(r[2] for r in t) == 16 + 32 + 64 + 3 * 64 + 4 * 128 + 6 * 128 + 6 * 256
    vfe, conv = lib.lisec_bn_recalibrate_coef(_lib.BN_FINALIZER_VFE), lib.lisec_bn_recalibrate_coef(_lib.BN_FINALIZER_CONV)
    assert [r[3] for r in t] == [vfe] * 3 + [conv] * 19 and (vfe, conv) == (R.COEF_VFE, R.COEF_CONV)


@pytest.mark.parametrize("statistics", ["mean", "pooled"])
def test_the_pass_is_the_definition_bit_for_bit(setup, statistics):
    net = setup.net
    want, _ = R.recalibrate(setup.states, setup.table, statistics)
    version = net.state_version
    net.recalibrate_batchnorm(setup.samples, statistics=statistics)
    got = _host(net.params.state)
    assert np.array_equal(R.bits(got), R.bits(want))
    assert net.state_version > version and not np.array_equal(R.bits(got), R.bits(setup.initial))
    # the empty sweep took part: without it the statistics are others
    three, _ = R.recalibrate(setup.states[:3], setup.table, statistics)
    assert not np.array_equal(R.bits(three), R.bits(want))


def _reported(net):
    """{layer: (batch mean, 1/invstd^2 - eps, rows M or None)} of the LAST training forward, from the bnstate it wrote:
    the conv layers' in net.bnstate, the VFE layers' at the head of the VFE's saved buffer (4*16, 4*32, 4*64 floats)."""
    out, convs = {}, {}
    for L in net.layers:
        c = L["conv"]
        if c.bn:
            convs[c.bn] = c
    saved, off = _host(net.vfe._saved[:4 * (16 + 32 + 64)]), 0
    for name, C in (("vfe1.bn", 16), ("vfe2.bn", 32), ("fcn.bn", 64)):
        b = saved[off:off + 4 * C].astype(np.float64)
        out[name] = (b[2 * C:3 * C], 1.0 / b[3 * C:] ** 2 - BN_EPS, None)
        off += 4 * C
    for name, c in convs.items():
        C = c.g.Cout
        b = _host(net.bnstate[name]).astype(np.float64)
        out[name] = (b[2 * C:3 * C], 1.0 / b[3 * C:] ** 2 - BN_EPS, float(c.M))
    return out


@pytest.mark.parametrize("sweep", [0, 3])
def test_one_sweep_gives_the_batch_statistics_the_forward_reports(setup, sweep):
    """K = 1.  Derived, not measured: the moving mean went through fl32(mean * c) and one final rounding, the reported
    one through one rounding: 3 * 2^-24 relative (1e-36: where mean * c is a float32 denormal).  The reported invstd
    is rounded once (2^-24), so 1/invstd^2 carries 2^-23 of (var + eps); the moving variance two roundings more of var;
    the factor M/(M - 1) is exact to 2^-53: under 2^-21 * (var + eps).  A layer given the other family's coefficient
    is 9.5e-7 = 16 * 2^-24 off in its mean."""
    net = setup.net
    net.recalibrate_batchnorm([setup.samples[sweep]])
    got = net.params.to_dict()
    reported = _reported(net)
    assert len(reported) == 22
    worst_m = worst_v = 0.0
    bad = []
    for name, (mean, var, M) in reported.items():
        if M is not None:
            var = var * (M / (M - 1.0))
        gm, gv = got[name + ".moving_mean"].astype(np.float64), got[name + ".moving_variance"].astype(np.float64)
        em, ev = np.abs(gm - mean) - 1e-36, np.abs(gv - var)
        worst_m = max(worst_m, float((em / np.maximum(np.abs(mean), 1e-300)).max()))
        worst_v = max(worst_v, float((ev / (var + BN_EPS)).max()))
        if not ((em <= 3 * U * np.abs(mean)).all() and (ev <= 2.0 ** -21 * (var + BN_EPS)).all()):
            bad.append(name)
    print(f"K = 1, sweep {sweep}: mean error {worst_m / U:.2f} x 2^-24 (bound 3), variance error "
          f"{worst_v / 2.0 ** -21:.3f} x 2^-21 (bound 1)")
    assert not bad, bad


def test_the_same_sweep_twice(setup):
    """'mean': the bits of K = 1 (x + x and 2x / 2 are exact in fp64).  'pooled': S2/2 + Sq/2 - mean^2 = var + (m^2 -
    m^2) up to the fp64 roundings of m^2 ~ 2^-52 m^2 -- against var + eps that stays under 2^-22 for |m| up to 1e4 *
    sqrt(var + eps), which every layer here keeps; the rest of the bound is the one float32 ulp (2^-23) by which two
    nearly equal doubles may round apart."""
    net, s = setup.net, setup.samples[0]
    net.recalibrate_batchnorm([s])
    one = _host(net.params.state)
    net.recalibrate_batchnorm([s, s], statistics="mean")
    assert np.array_equal(R.bits(_host(net.params.state)), R.bits(one))
    net.recalibrate_batchnorm([s, s], statistics="pooled")
    two = _host(net.params.state)
    for mean_off, var_off, C, _ in setup.table:
        assert np.array_equal(R.bits(two[mean_off:mean_off + C]), R.bits(one[mean_off:mean_off + C]))
        v1, v2 = one[var_off:var_off + C].astype(np.float64), two[var_off:var_off + C].astype(np.float64)
        assert (np.abs(v2 - v1) <= 2.0 ** -22 * (v1 + BN_EPS)).all()


def _oracle_rule(setup, statistics):
    """oracle.model_ref.forward(training=True, stats=...) per sweep in fp64, then the rule in fp64."""
    from oracle import voxel_ref
    if not hasattr(setup, "oracle_stats"):
        per = []
        p64 = {k: v.double() for k, v in setup.op.items()}
        for pts in setup.points:
            vox = voxel_ref.voxelize_ref(pts.astype(np.float64), **SMALL)
            dense = torch.from_numpy(voxel_ref.to_dense(vox, (8, 16, 32, 35, 6)))[None].double()
            stats = {}
            setup.M.forward(p64, dense, training=True, stats=stats)
            per.append({k: (m.numpy(), (v * (n / (n - 1.0)) if fused else v).numpy()) for k, (m, v, n, fused) in stats.items()})
        setup.oracle_stats = per
    out = {}
    for name in setup.oracle_stats[0]:
        m = np.stack([s[name][0] for s in setup.oracle_stats])
        v = np.stack([s[name][1] for s in setup.oracle_stats])
        mean, var = m.mean(0), v.mean(0)
        if statistics == "pooled":
            var = np.maximum(0.0, var + (m * m).mean(0) - mean * mean)
        out[name] = (mean, var)
    return out


@pytest.mark.parametrize("statistics", ["mean", "pooled"])
def test_against_the_fp64_oracle(setup, statistics):
    """Means: the project's activation bound (close, rtol 1e-3).  Variances: no bound follows from the activation bound
    alone; the largest relative error measured on the MI355X is MEASURED_VAR_ERR and the test asserts 4x that, at most
    1e-2."""
    net = setup.net
    net.recalibrate_batchnorm(setup.samples, statistics=statistics)
    got = net.params.to_dict()
    ref = _oracle_rule(setup, statistics)
    assert len(ref) == 22
    worst = 0.0
    for name, (mean, var) in ref.items():
        close(got[name + ".moving_mean"], mean, what=name + ".moving_mean")
        gv = got[name + ".moving_variance"].astype(np.float64)
        assert (var > 0).all(), name
        worst = max(worst, float((np.abs(gv - var) / var).max()))
    print(f"largest relative error of a recalibrated variance against the fp64 oracle ({statistics}): {worst:.3e}; "
          f"bound {VAR_BOUND:.3e}")
    assert worst <= VAR_BOUND


def test_nothing_else_moves_and_the_statistics_travel(setup):
    net = setup.net
    net._prepare_training()
    gen = torch.Generator(device="cpu").manual_seed(3)
    for name in ("velocity", "m", "v"):
        net.slot(name).copy_(torch.randn(net.params.n_theta, generator=gen))
    net.average.copy_(torch.randn(net.params.n_theta, generator=gen))
    net.iterations = 7
    before = dict(theta=_host(net.params.theta), average=_host(net.average), iter_dev=_host(net._iter_dev),
                  momentum_cache=_host(net.momentum_cache), **{k: _host(t) for k, t in net.slots().items()})
    params_version = net.params_version
    net.params.state.copy_(torch.from_numpy(setup.initial))
    net.state_version += 1
    sample = setup.samples[1]
    old = [_host(t) for t in net.forward(sample, training=False)]
    net.recalibrate_batchnorm(setup.samples[:3], statistics="pooled")
    after = dict(theta=_host(net.params.theta), average=_host(net.average), iter_dev=_host(net._iter_dev),
                 momentum_cache=_host(net.momentum_cache), **{k: _host(t) for k, t in net.slots().items()})
    assert sorted(before) == sorted(after) and len(before) >= 7
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    assert net.iterations == 7 and net.params_version == params_version and net._early is None
    new = [_host(t) for t in net.forward(sample, training=False)]
    assert any(not np.array_equal(a, b) for a, b in zip(old, new))
    twin = setup.fresh_net(init=net.params.to_dict())
    for a, b in zip(new, [_host(t) for t in twin.forward(sample, training=False)]):
        assert np.array_equal(R.bits(a), R.bits(b))


def test_a_failure_restores_the_statistics(setup):
    from lisec_amd.voxelizer import Voxelizer
    net = setup.net
    other = Voxelizer(**dict(SMALL, maxVoxelX=4))(setup.points[0])          # a sweep of another grid
    before = _host(net.params.state)
    version = net.state_version
    with pytest.raises(ValueError, match="grid"):
        net.recalibrate_batchnorm([setup.samples[0], other, setup.samples[1]])
    assert np.array_equal(R.bits(_host(net.params.state)), R.bits(before)) and net.state_version > version
    # refused before any launch
    for bad in (dict(samples=[]), dict(samples=setup.samples, statistics="median")):
        with pytest.raises(ValueError):
            net.recalibrate_batchnorm(**bad)
    assert np.array_equal(R.bits(_host(net.params.state)), R.bits(before))
    from lisec_amd.network import LisecNet
    from lisec_amd.params import ParamStore
    bf16 = LisecNet(16, 32, 8, 35, params=ParamStore(setup.dev, init=setup.op), compute_dtype="bfloat16")
    with pytest.raises(NotImplementedError):
        bf16.recalibrate_batchnorm(setup.samples[:1])


def test_a_pending_early_update_is_refused(setup):
    """Between early_update() and apply_gradients() a part of theta is ahead of the rest: RuntimeError, nothing launched,
    and the pass runs once the step has ended."""
    from lisec_amd.network import OptimizerSpec
    net, spec = setup.fresh_net(), OptimizerSpec()
    yc = torch.zeros(8, 16, 2, dtype=torch.float32, device=setup.dev)
    yr = torch.zeros(8, 16, 14, dtype=torch.float32, device=setup.dev)
    net.forward(setup.samples[0], training=True)
    net.backward(yc, yr, loss="mse", rpn_grads_ready=lambda lo, hi: net.early_update(lo, hi, opt=spec))
    assert net._early is not None
    before = _host(net.params.state)
    with pytest.raises(RuntimeError, match="early update"):
        net.recalibrate_batchnorm(setup.samples[:1])
    assert np.array_equal(R.bits(_host(net.params.state)), R.bits(before))
    net.apply_gradients(opt=spec)
    net.recalibrate_batchnorm(setup.samples[:1])
    assert not np.array_equal(R.bits(_host(net.params.state)), R.bits(before))
