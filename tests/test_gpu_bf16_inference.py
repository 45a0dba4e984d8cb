"""The 'mixed_bfloat16' policy at model level: predict() / evaluate() with the bf16-MFMA contractions, on the GPU.

Tolerance of the parity checks -- measured against the ORACLE, not against the code under test: the fp64 oracle forward is
run a second time with oracle.model_ref.F replaced by a shim whose conv2d, and conv3d from the second call of a forward
on, round input and weight through torch.bfloat16 (exactly the layers the policy runs in bf16: mid2, mid3 and the sixteen
RPN Conv2Ds; rounding of the input after BatchNormalization + ReLU, as the kernel does).  With ref the plain fp64 forward
and emu the emulated one, E = ||emu - ref||_2 / ||ref||_2 over the 16 head channels, and the requirement is
    ||predict_bf16 - ref||_2 / ||ref||_2 <= 2 E + 1e-3.
The kernel sums in another order than the CPU, which flips individual bf16 roundings of later layers: kernel and
emulation are two draws of the same error, not the same numbers -- the factor 2 covers two independent draws, and 1e-3 is
the project's inference-parity rtol (test_gpu_evaluate.py).  On the CPU (seeds 7 and 11, clouds 0-2) E = 1.3e-3 .. 1.8e-3.
Small grid and fixtures as in test_gpu_evaluate.py (16x32x8x35, glorot_params(seed, randomize_bn=True), _cloud seeds)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu
SMALL = dict(xSize=0.5, ySize=0.25, zSize=0.25, sampleSize=35, maxVoxelX=8, maxVoxelY=16, maxVoxelZ=8)


@pytest.fixture(autouse=True)
def _restore_policy():
    from lisec_amd import mixed_precision as mp
    before = mp.global_policy()
    yield
    mp.set_global_policy(before)


def _cloud(seed, n=2500, pad_to=None):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-4.2, 4.2, n), rng.uniform(-4.2, 4.2, n), rng.uniform(0.0, 2.1, n)], 1).astype(np.float32)
    if pad_to:
        out = np.full((pad_to, 3), 1.0e6, np.float32)
        out[:n] = pts
        pts = out
    return pts


def _targets(seed):
    rng = np.random.default_rng(100 + seed)
    return rng.integers(0, 3, (8, 16, 2)).astype(np.float32), rng.normal(0, 1, (8, 16, 14)).astype(np.float32)


def _data(seeds, pad_to=None):
    from lisec_amd import model_training as mt
    x = [mt.VFE_preprocessing(_cloud(s, pad_to=pad_to), **SMALL) for s in seeds]
    ys = [_targets(s) for s in seeds]
    return x, [np.stack([y[0] for y in ys]), np.stack([y[1] for y in ys])]


def _model(policy, seed=7):
    from lisec_amd import mixed_precision as mp
    from lisec_amd import model_training as mt
    from lisec_amd.params import ParamStore
    from oracle import model_ref as M
    mp.set_global_policy(policy)
    m = mt.Model(16, 32, 8, 35, params=ParamStore(torch.device("cuda"), init=M.glorot_params(seed=seed, randomize_bn=True)))
    m.compile(optimizer=mt.optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True), loss=['mse', 'mse'])
    return m


class _Bf16F:
    """torch.nn.functional with the policy's bf16 layers emulated: conv2d always, conv3d from the second call after
    begin() on (the first Conv3D stays fp32); everything else passes through."""

    def __init__(self):
        self.conv3d_calls = 0

    def begin(self):
        self.conv3d_calls = 0

    @staticmethod
    def _r(t):
        return t.to(torch.bfloat16).to(t.dtype)

    def conv3d(self, x, w, *a, **k):
        self.conv3d_calls += 1
        if self.conv3d_calls >= 2:
            x, w = self._r(x), self._r(w)
        return TF.conv3d(x, w, *a, **k)

    def conv2d(self, x, w, *a, **k):
        return TF.conv2d(self._r(x), self._r(w), *a, **k)

    def __getattr__(self, name):
        return getattr(TF, name)


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _heads(cls, reg):
    return np.concatenate([np.asarray(cls, np.float64).reshape(-1, 2), np.asarray(reg, np.float64).reshape(-1, 14)], 1)


@pytest.mark.parametrize("seed", [7, 11])
def test_predict_within_twice_the_emulated_bf16_error_of_the_oracle(seed, monkeypatch):
    from oracle import model_ref as M
    from oracle import voxel_ref
    model = _model("mixed_bfloat16", seed)
    x, _ = _data(range(3))
    probs, regs = model.predict(x)
    assert model.net.bf16_launches == 3 * 18          # mid2, mid3 and the sixteen RPN Conv2Ds, every sweep
    p64 = {k: v.double() for k, v in M.glorot_params(seed=seed, randomize_bn=True).items()}
    shim = _Bf16F()
    for k in range(3):
        vox = voxel_ref.voxelize_ref(_cloud(k).astype(np.float64), **SMALL)
        dense = torch.from_numpy(voxel_ref.to_dense(vox, (8, 16, 32, 35, 6)))[None].double()
        with torch.no_grad():
            ref = _heads(*M.forward(p64, dense, training=False))
            with monkeypatch.context() as mctx:
                mctx.setattr(M, "F", shim)
                shim.begin()
                emu = _heads(*M.forward(p64, dense, training=False))
            assert shim.conv3d_calls == 3
        E = _rel(emu, ref)
        got = _rel(_heads(probs[k], regs[k]), ref)
        worst = np.abs(_heads(probs[k], regs[k]) - ref).max() / np.abs(ref).max()
        print(f"seed {seed} cloud {k}: E(emulation) {E:.3e}  achieved {got:.3e}  bound {2 * E + 1e-3:.3e}  "
              f"max err / max|ref| {worst:.3e}")
        assert 5e-4 < E < 1e-2                         # the emulation rounds (and the bound is not vacuous)
        assert got <= 2 * E + 1e-3


def test_the_policy_is_on_and_float32_is_untouched():
    from lisec_amd import mixed_precision as mp
    x, _ = _data(range(2))
    before = _model("float32")                         # built before 'mixed_bfloat16' is ever set in this test
    want = before.predict(x)
    bf = _model("mixed_bfloat16")
    assert bf.dtype_policy.name == "mixed_bfloat16" and bf.net.compute_dtype == "bfloat16" and len(bf.net.packed_bf16) == 18
    assert sorted(bf.net.packed_bf16) == sorted(
        ["mid2.conv", "mid3.conv"] + [f"rpn{b}.conv{j}" for b, q in ((1, 4), (2, 6), (3, 6)) for j in range(q)])
    got = bf.predict(x)
    assert bf.net.bf16_launches == 2 * 18
    assert got[0].dtype == np.float32 and got[1].dtype == np.float32
    assert not np.array_equal(got[0], want[0]) and not np.array_equal(got[1], want[1])
    # the global policy is still 'mixed_bfloat16': a float32 model built earlier does not care, nor does one built now
    assert mp.global_policy().name == "mixed_bfloat16" and before.dtype_policy.name == "float32"
    again = before.predict(x)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    assert before.net.bf16_launches == 0 and not before.net.packed_bf16
    after = _model("float32")
    now = after.predict(x)
    assert np.array_equal(now[0], want[0]) and np.array_equal(now[1], want[1])
    # ... and changing the global policy does not change the bf16 model
    mp.set_global_policy("float32")
    same = bf.predict(x)
    assert bf.dtype_policy.name == "mixed_bfloat16"
    assert np.array_equal(same[0], got[0]) and np.array_equal(same[1], got[1])


def test_two_policies_in_one_process_share_nothing():
    x, _ = _data(range(3))
    f32, bf = _model("float32"), _model("mixed_bfloat16")
    want32, want16 = f32.predict(x), bf.predict(x)
    for _ in range(2):                                 # alternately: a shared pack, fold or workspace state would show
        a, b = bf.predict(x), f32.predict(x)
        assert np.array_equal(a[0], want16[0]) and np.array_equal(a[1], want16[1])
        assert np.array_equal(b[0], want32[0]) and np.array_equal(b[1], want32[1])
    assert not f32.net.packed_bf16
    assert all(bf.net.packed[k].data_ptr() != f32.net.packed[k].data_ptr() for k in bf.net.packed)


def test_evaluate_is_the_mean_of_predicts_losses_and_the_plan_agrees(monkeypatch):
    model = _model("mixed_bfloat16")
    x, y = _data(range(20, 24), pad_to=4096)
    monkeypatch.setenv("LISEC_TUNING", "eval_plan=0")
    res = model.evaluate(x, y, verbose=0)
    assert model._eval_captured is None
    probs, regs = model.predict(x)
    mine = []
    for k in range(4):
        dc = (probs[k] - y[0][k]).astype(np.float64)
        dr = (regs[k] - y[1][k]).astype(np.float64)
        mine.append([(dc ** 2).mean() + (dr ** 2).mean(), (dc ** 2).mean(), (dr ** 2).mean()])
    np.testing.assert_allclose(res, np.mean(mine, 0), rtol=1e-5)
    # the recorded evaluation step replays the same launches on the same padded sweeps: the eager value, bit for bit
    # (test_gpu_evaluate.py::test_eval_plan_replay_equals_eager_across_training states the rule)
    monkeypatch.setenv("LISEC_TUNING", "eval_plan=1")
    launches = model.net.bf16_launches
    replay = model.evaluate(x, y, verbose=0)
    assert model._eval_captured is not None and model._eval_captured[0][-1] == "bfloat16"
    assert model.net.bf16_launches > launches          # the plan was recorded from the bf16 forward
    assert replay == res
    # unpadded sweeps: the plan pads them to its capacity, the eager path does not -- equal within rounding
    xu, yu = _data(range(20, 24))
    replay = model.evaluate(xu, yu, verbose=0)
    monkeypatch.setenv("LISEC_TUNING", "eval_plan=0")
    np.testing.assert_allclose(replay, model.evaluate(xu, yu, verbose=0), rtol=1e-6)


def test_fit_is_refused_and_touches_nothing():
    model = _model("mixed_bfloat16")
    x, y = _data(range(2))
    net = model.net
    torch.cuda.synchronize()

    def state():
        torch.cuda.synchronize()
        return dict(theta=net.params.theta.cpu().numpy().copy(), state=net.params.state.cpu().numpy().copy(),
                    it=net._iter_dev.cpu().numpy().copy(), iterations=net.iterations,
                    **{"slot_" + k: t.cpu().numpy().copy() for k, t in net.slots().items()})

    before = state()
    with pytest.raises(NotImplementedError, match="mixed_bfloat16"):
        model.fit(x, y, verbose=0, epochs=1, steps_per_epoch=2)
    sample = model._as_samples(x)[0]
    with pytest.raises(NotImplementedError):
        net.forward(sample, training=True)
    with pytest.raises(NotImplementedError):
        net.train_step(sample, torch.from_numpy(y[0][0]).cuda(), torch.from_numpy(y[1][0]).cuda())
    after = state()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert model._captured is None


def test_save_writes_float32_variables_and_load_takes_the_policy_in_force(tmp_path):
    from lisec_amd import mixed_precision as mp
    from lisec_amd import model_training as mt
    x, _ = _data(range(2))
    bf = _model("mixed_bfloat16")
    want16 = bf.predict(x)
    path16, path32 = str(tmp_path / "bf16.h5"), str(tmp_path / "f32.h5")
    bf.save(path16)
    f32 = _model("float32")
    want32 = f32.predict(x)
    f32.save(path32)
    assert open(path16, "rb").read() == open(path32, "rb").read()      # the policy is not persisted
    back = mt.load_model(path16)                                        # global policy: 'float32'
    assert back.dtype_policy.name == "float32"
    got = back.predict(x)
    assert np.array_equal(got[0], want32[0]) and np.array_equal(got[1], want32[1])
    mp.set_global_policy("mixed_bfloat16")
    back16 = mt.load_model(path32)
    assert back16.dtype_policy.name == "mixed_bfloat16"
    got = back16.predict(x)
    assert np.array_equal(got[0], want16[0]) and np.array_equal(got[1], want16[1])
    made = mt.createModel(16, 32, 8, 35)
    assert made.dtype_policy.name == "mixed_bfloat16" and made.net.compute_dtype == "bfloat16"


def test_full_lyft_grid_bf16_inference_within_twice_the_emulated_error(monkeypatch):
    """The same comparison once at the real grid (8,200,400,35), through forward_from_grid as
    test_gpu_network.py::test_full_lyft_grid_inference_vs_oracle does for fp32."""
    from conftest import LYFT
    from lisec_amd.network import LisecNet
    from lisec_amd.params import ParamStore
    from lisec_amd.voxelizer import Voxelizer
    from oracle import model_ref as M
    from test_gpu_network import _hybrid_oracle_lyft, u20k
    pts = u20k(5)
    op = M.glorot_params(seed=77, randomize_bn=True)
    net = LisecNet(200, 400, 8, 35, params=ParamStore(torch.device("cuda"), init=op), compute_dtype="bfloat16")
    cls, reg = net.forward(Voxelizer(**LYFT)(pts), training=False)
    got = _heads(cls.cpu().numpy(), reg.cpu().numpy())
    assert net.bf16_launches == 18
    ref = _heads(*(t.numpy() for t in _hybrid_oracle_lyft(op, pts, training=False)[:2]))
    shim = _Bf16F()
    with monkeypatch.context() as mctx:
        mctx.setattr(M, "F", shim)
        shim.begin()
        emu = _heads(*(t.numpy() for t in _hybrid_oracle_lyft(op, pts, training=False)[:2]))
    assert shim.conv3d_calls == 3
    E, achieved = _rel(emu, ref), _rel(got, ref)
    worst = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"Lyft grid: E(emulation) {E:.3e}  achieved {achieved:.3e}  bound {2 * E + 1e-3:.3e}  max err / max|ref| {worst:.3e}")
    assert achieved <= 2 * E + 1e-3
