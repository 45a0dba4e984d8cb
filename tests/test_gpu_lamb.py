"""lisec_lamb_step_dev / lisec_lamb_step_sched on the GPU, through lisec_amd.ops and the C ABI, on a synthetic theta
against the fp64 definition of tests/lamb_ref.py: the formula over five steps, the descriptor entry, a split update,
determinism and every refusal.  The table holds, at the smallest sizes, every way the per-variable reduction can go
wrong (see VARIABLES)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lamb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
CHUNK = 4096                               # LISEC_REG_CHUNK
N_MODEL = 6_491_024                        # trainable variables of the Lisec network (params.py)
GAP = 8                                    # untouched floats in front of every variable and behind the last
CANARY = F(-7.25)
START = 7
LR, DECAY = 0.01, 1e-3                     # as tests/test_gpu_optimizers.py::test_update_kernels_match_formula
# the entries take beta_1, beta_2, epsilon and weight_decay_rate as C floats: the definition gets the values the kernels get
B1, B2, EPS = (float(F(x)) for x in (0.9, 0.999, 1e-6))
WD = float(F(0.01))


def _grid():
    from lisec_amd import ops
    return ops.LAMB_BLOCKS


def _variables():
    """[(name, count, decayed, adapted)]: the variables of the synthetic table, in buffer order."""
    return [
        ("four", 4, True, True),                                   # a 4-float variable
        ("one_chunk", CHUNK, True, True),                          # exactly one chunk
        ("tail", CHUNK + 4, True, True),                           # a tail chunk of 4
        ("zero_w", 64, True, True),                                # an all-zero variable: r = 1
        ("still", 100, True, True),                                # g = m = v = 0: u = 0 and r = 1, or u = wd*w
        ("unadapted", 5000, True, False),                          # excluded from layer adaptation: r = 1
        ("long", (_grid() + 1) * CHUNK + 4, True, True),           # more chunks than the grid is wide
        ("undecayed", 300, False, True),                           # excluded from weight decay
    ]


def _layout():
    """(rows [(offset, count, decayed, adapted)], names, n): GAP floats outside every variable."""
    rows, names, at = [], [], GAP
    for name, count, decayed, adapted in _variables():
        rows.append((at, count, decayed, adapted))
        names.append(name)
        at += count + GAP
    return rows, names, at


def _tables(rows):
    """The host tables of rows, as ops.lamb_chunks makes them for a network."""
    from lisec_amd import _lib
    chunks, variables = [], []
    for j, (off, count, decayed, adapted) in enumerate(rows):
        flags = (_lib.LAMB_DECAYED if decayed else 0) | (_lib.LAMB_ADAPTED if adapted else 0)
        first = len(chunks)
        for start in range(0, count, CHUNK):
            chunks.append((off + start, min(CHUNK, count - start), j, flags))
        variables.append((first, len(chunks) - first))
    return chunks, variables


_CACHE = {}


def _inputs():
    """theta, m, v at the start (float32, canaries outside the variables) and the five gradients; made once, read-only."""
    if "in" not in _CACHE:
        rows, names, n = _layout()
        rng = np.random.default_rng(23)
        theta = rng.standard_normal(n).astype(F)
        m = (rng.standard_normal(n) * 0.1).astype(F)
        v = (np.abs(rng.standard_normal(n)) * 0.01).astype(F)
        grads = [(rng.standard_normal(n) * (1 + s)).astype(F) for s in range(5)]
        inside = np.zeros(n, bool)
        for off, count, _, _ in rows:
            inside[off:off + count] = True
        for a in (theta, m, v, *grads):
            a[~inside] = CANARY
        off, count = rows[names.index("zero_w")][:2]
        theta[off:off + count] = 0
        off, count = rows[names.index("still")][:2]
        for a in (m, v, *grads):
            a[off:off + count] = 0
        for a in (theta, m, v, *grads, inside):
            a.setflags(write=False)
        _CACHE["in"] = (theta, m, v, grads, inside)
    return _CACHE["in"]


def _reference(wd):
    """The five steps of the definition from the shared inputs: [(theta, m, v, ratios)] after each, float64."""
    key = ("ref", wd)
    if key not in _CACHE:
        rows, _, _ = _layout()
        theta, m, v, grads, _ = _inputs()
        th, mm, vv = (a.astype(np.float64) for a in (theta, m, v))
        out = []
        for s, g in enumerate(grads):
            th, mm, vv, r = R.step(th, mm, vv, g, rows, START + s, LR, DECAY, B1, B2, EPS, wd)
            out.append((th, mm, vv, r))
        _CACHE[key] = out
    return _CACHE[key]


class _Run:
    """The device side of one run over the synthetic table."""

    def __init__(self, rows, theta, m, v, start=START):
        import torch
        from lisec_amd import ops
        self.chunks, self.variables = _tables(rows)
        self.table = ops.lamb_table(self.chunks, self.variables, "cuda")
        self.theta, self.m, self.v = (torch.from_numpy(np.array(a)).cuda() for a in (theta, m, v))
        self.state = torch.tensor([start, 0], dtype=torch.int64, device="cuda")
        self.ratios = torch.full((len(rows),), -3.0, dtype=torch.float32, device="cuda")
        self.ws = ops.lamb_workspace(len(self.chunks), len(rows), "cuda")

    def step(self, grad, wd, advance=True, sched=None, **rng):
        from lisec_amd import ops
        if sched is None:
            ops.lamb_step_dev(self.theta, grad, self.m, self.v, LR, DECAY, wd, B1, B2, EPS, self.state, advance=advance,
                              table=self.table, ratios=self.ratios, workspace=self.ws, **rng)
        else:
            ops.lamb_step_sched(self.theta, grad, self.m, self.v, sched, wd, B1, B2, EPS, self.state, advance=advance,
                                table=self.table, ratios=self.ratios, workspace=self.ws, **rng)

    def host(self):
        return [t.cpu().numpy() for t in (self.theta, self.m, self.v, self.ratios)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_against(got, want, rows, inside, start_arrays):
    theta, m, v, ratios = got
    th, mm, vv, r = want
    err = np.abs(theta[inside].astype(np.float64) - th[inside]) / np.maximum(1.0, np.abs(th[inside]))
    print("theta: max |d| / max(1, |ref|) =", float(err.max()))
    for name, a, b in (("m", m, mm), ("v", v, vv)):
        d = np.abs(a[inside].astype(np.float64) - b[inside])
        print(name, ": max |d| =", float(d.max()), "max |ref| =", float(np.abs(b[inside]).max()))
    print("ratios:", ratios.tolist(), "max rel =", float(np.max(np.abs(ratios - r) / np.abs(r))))
    assert err.max() <= 1e-6, float(err.max())
    for a, b in ((m, mm), (v, vv)):
        np.testing.assert_allclose(a[inside].astype(np.float64), b[inside], rtol=1e-5, atol=1e-7 * np.abs(b[inside]).max())
    np.testing.assert_allclose(ratios.astype(np.float64), r, rtol=1e-5, atol=0)
    # the floats in the gaps keep their bits in all three buffers
    for a, a0 in zip((theta, m, v), start_arrays):
        assert np.array_equal(_bits(a[~inside]), _bits(a0[~inside]))


def test_the_table_is_longer_than_the_grid_and_has_every_case():
    rows, names, n = _layout()
    chunks, variables = _tables(rows)
    long_ = variables[names.index("long")]
    assert long_[1] > _grid() and len(chunks) > _grid()
    assert variables[names.index("tail")][1] == 2 and chunks[variables[names.index("tail")][0] + 1][1] == 4
    assert variables[names.index("four")] == (0, 1) and chunks[0][:2] == (GAP, 4)
    assert all(o % 4 == 0 and c % 4 == 0 and 0 < c <= CHUNK for o, c, _, _ in chunks)
    assert sum(c for _, c, _, _ in rows) + GAP * (len(rows) + 1) == n
    theta, m, v, grads, inside = _inputs()
    assert inside.sum() == sum(c for _, c, _, _ in rows) and (theta[~inside] == CANARY).all()


@pytest.mark.parametrize("wd", [0.0, WD], ids=["no_decay", "decay"])
def test_formula(wd):
    import torch
    rows, names, n = _layout()
    theta0, m0, v0, grads, inside = _inputs()
    want = _reference(wd)
    run = _Run(rows, theta0, m0, v0)
    special = {names.index("unadapted")}
    if wd == 0:
        special.add(names.index("still"))
    for s, g in enumerate(grads):
        gd = torch.from_numpy(g.copy()).cuda()
        run.step(gd, wd)
        torch.cuda.synchronize()
        assert run.state.cpu().tolist() == [START + s + 1, 0]                 # one increment per step, ticket reset
        assert np.array_equal(_bits(gd.cpu().numpy()), _bits(g))                # grad is only read
        ratios = run.ratios.cpu().numpy()
        np.testing.assert_allclose(ratios.astype(np.float64), want[s][3], rtol=1e-5, atol=0)
        for j in special | ({names.index("zero_w")} if s == 0 else set()):
            assert ratios[j] == F(1.0) and want[s][3][j] == 1.0, (s, names[j])
        if wd > 0:                                                              # u = wd*w: r = 1 / wd
            assert abs(ratios[names.index("still")] * wd - 1) < 1e-5
    _check_against(run.host(), want[-1], rows, inside, (theta0, m0, v0))
    off, count = rows[names.index("still")][:2]
    got = run.host()
    assert not got[1][off:off + count].any() and not got[2][off:off + count].any()
    if wd == 0:                                                                 # u = 0: the variable keeps its bits
        assert np.array_equal(_bits(got[0][off:off + count]), _bits(theta0[off:off + count]))


def test_formula_on_the_network_table():
    """Once more at the network's own size, with its real variable table: the biases, gammas and betas excluded from
    decay and from adaptation."""
    import torch
    from lisec_amd import _lib, ops
    from lisec_amd.params import ParamStore
    store = ParamStore(torch.device("cpu"))
    n = store.n_theta                                                           # N_MODEL and the padding to 16 bytes
    assert store.n_trainable() == N_MODEL <= n < N_MODEL + 4 * len(store.trainable_names())
    no = ("bias", "gamma", "beta")
    chunks, variables = ops.lamb_chunks(store, no)
    rows = [(off, sum(c[1] for c in chunks[first:first + k]), bool(chunks[first][3] & _lib.LAMB_DECAYED),
             bool(chunks[first][3] & _lib.LAMB_ADAPTED)) for first, k, off, _ in variables]
    assert sum(r[1] for r in rows) == n and any(not r[3] for r in rows) and any(r[3] for r in rows)
    rng = np.random.default_rng(29)
    theta0 = rng.standard_normal(n).astype(F)
    z = np.zeros(n, F)
    run = _Run(rows, theta0, z, z)
    assert run.chunks == chunks and run.variables == [v[:2] for v in variables]
    th, mm, vv = theta0.astype(np.float64), z.astype(np.float64), z.astype(np.float64)
    for s in range(2):
        g = (rng.standard_normal(n) * (1 + s)).astype(F)
        run.step(torch.from_numpy(g.copy()).cuda(), WD)
        th, mm, vv, r = R.step(th, mm, vv, g, rows, START + s, LR, DECAY, B1, B2, EPS, WD)
    torch.cuda.synchronize()
    got = run.host()
    _check_against(got, (th, mm, vv, r), rows, np.ones(n, bool), (theta0, z, z))
    assert all(got[3][j] == F(1.0) for j, row in enumerate(rows) if not row[3])


def _three_steps(split_at=None, sched=False, wd=WD):
    """Three steps from the shared inputs; split_at: the variable the early part (advance=0) starts at."""
    import torch
    from lisec_amd import _lib, lr_schedules, ops
    rows, names, n = _layout()
    theta0, m0, v0, grads, _ = _inputs()
    run = _Run(rows, theta0, m0, v0, start=41)
    desc = None
    if sched:
        desc = torch.zeros(ctypes.sizeof(_lib.LrSchedule), dtype=torch.uint8, device="cuda")
        ops.lr_schedule_set(desc, lr_schedules.descriptor(LR, DECAY))
    all_ratios = []
    for g in grads[:3]:
        gd = torch.from_numpy(g.copy()).cuda()
        if split_at is None:
            run.step(gd, wd, sched=desc)
        else:
            fc = run.variables[split_at][0]
            run.step(gd, wd, advance=False, sched=desc, first=fc, first_var=split_at)
            run.step(gd, wd, advance=True, sched=desc, first=0, n_chunks=fc, first_var=0, n_vars=split_at)
        all_ratios.append(run.ratios.cpu().numpy())
    torch.cuda.synchronize()
    assert run.state.cpu().tolist() == [44, 0]
    return run.host() + all_ratios


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_by_value_equals_descriptor():
    assert _same_bits(_three_steps(), _three_steps(sched=True))


@pytest.mark.parametrize("split_at", [1, 6, 7])
def test_part_then_rest_is_bit_identical_to_one_launch(split_at):
    """advance=0 over the chunks from a variable boundary on (the early update), then advance=1 over the rest: the bits
    of one launch, and the count advances once per step.  Boundaries: behind the first variable, in front of the long
    one, and in front of the last."""
    assert _same_bits(_three_steps(), _three_steps(split_at=split_at))


def test_the_closing_part_may_be_empty():
    """advance=1 over no chunk at all still ends the step."""
    import torch
    rows, names, n = _layout()
    theta0, m0, v0, grads, _ = _inputs()
    run = _Run(rows, theta0, m0, v0)
    gd = torch.from_numpy(grads[0].copy()).cuda()
    run.step(gd, WD, advance=False)
    run.step(gd, WD, advance=True, first=0, n_chunks=0, first_var=0, n_vars=0)
    torch.cuda.synchronize()
    assert run.state.cpu().tolist() == [START + 1, 0]
    whole = _Run(rows, theta0, m0, v0)
    whole.step(gd, WD)
    assert _same_bits(run.host(), whole.host())


def test_two_runs_agree_bit_for_bit():
    assert _same_bits(_three_steps(), _three_steps())


def test_refusals_leave_everything_untouched():
    import torch
    from lisec_amd import _lib, lr_schedules, ops
    rows, names, n = _layout()
    rows = rows[:4]                                                             # (a small table is enough here)
    n = rows[-1][0] + rows[-1][1] + GAP
    theta0, m0, v0, grads, _ = _inputs()
    run = _Run(rows, theta0[:n], m0[:n], v0[:n])
    g = torch.from_numpy(grads[0][:n].copy()).cuda()
    desc = torch.zeros(ctypes.sizeof(_lib.LrSchedule), dtype=torch.uint8, device="cuda")
    ops.lr_schedule_set(desc, lr_schedules.descriptor(LR, DECAY))
    lib, P, V, st = _lib.load(), _lib.ptr, ctypes.c_void_p, _lib.current_stream()
    EINVAL = -1                                                                 # LISEC_EINVAL
    nc, nv = len(run.chunks), len(rows)
    base = dict(theta=P(run.theta), grad=P(g), m=P(run.m), v=P(run.v), chunks=P(run.table.chunks), first_chunk=0,
                n_chunks=nc, vars=P(run.table.variables), first_var=0, n_vars=nv, ratios=P(run.ratios),
                workspace=P(run.ws), workspace_bytes=run.ws.numel(), wd=WD, b1=B1, b2=B2, eps=EPS, state=P(run.state),
                advance=1)

    def dev(**kw):
        a = dict(base, **kw)
        return lib.lisec_lamb_step_dev(a["theta"], a["grad"], a["m"], a["v"], a["chunks"], a["first_chunk"], a["n_chunks"],
                                       a["vars"], a["first_var"], a["n_vars"], a["ratios"], a["workspace"],
                                       a["workspace_bytes"], LR, DECAY, a["wd"], a["b1"], a["b2"], a["eps"], a["state"],
                                       a["advance"], st)

    def sched(**kw):
        a = dict(dict(base, sched=P(desc)), **kw)
        return lib.lisec_lamb_step_sched(a["theta"], a["grad"], a["m"], a["v"], a["chunks"], a["first_chunk"],
                                         a["n_chunks"], a["vars"], a["first_var"], a["n_vars"], a["ratios"],
                                         a["workspace"], a["workspace_bytes"], a["sched"], a["wd"], a["b1"], a["b2"],
                                         a["eps"], a["state"], a["advance"], st)

    bad = [dict(n_chunks=-1), dict(n_vars=-1), dict(first_chunk=-1), dict(first_var=-1), dict(n_chunks=0),
           dict(n_vars=0), dict(workspace_bytes=lib.lisec_lamb_workspace_bytes(nc, nv) - 1), dict(workspace_bytes=0),
           dict(b1=1.0), dict(b1=-0.5), dict(b2=1.0), dict(b2=float("nan")), dict(eps=-1e-6), dict(wd=-0.1),
           dict(advance=2)]
    bad += [{k: None} for k in ("theta", "grad", "m", "v", "chunks", "vars", "ratios", "workspace", "state")]
    bad += [{k: V(t.data_ptr() + 4)} for k, t in (("theta", run.theta), ("grad", g), ("m", run.m), ("v", run.v),
                                                  ("state", run.state), ("workspace", run.ws))]
    bad += [dict(theta=V(run.theta.data_ptr() + 8))]
    for kw in bad:
        assert dev(**kw) == EINVAL, kw
        assert sched(**kw) == EINVAL, kw
    assert sched(sched=None) == EINVAL
    assert lib.lisec_lamb_workspace_bytes(nc, nv) == 16 * nc and lib.lisec_lamb_workspace_bytes(0, 0) > 0
    torch.cuda.synchronize()
    got = run.host()
    for a, a0 in zip(got[:3], (theta0[:n], m0[:n], v0[:n])):
        assert np.array_equal(_bits(a), _bits(a0))
    assert (got[3] == F(-3.0)).all() and run.state.cpu().tolist() == [START, 0]
    assert np.array_equal(_bits(g.cpu().numpy()), _bits(grads[0][:n]))
    with pytest.raises(ValueError):                                             # ops refuses a range outside the table
        run.step(g, WD, first=1, n_chunks=nc)
    with pytest.raises(ValueError):
        run.step(g, WD, first_var=1, n_vars=nv)
    assert dev() == 0                                                           # and the good call goes through
    torch.cuda.synchronize()
    assert run.state.cpu().tolist() == [START + 1, 0]
