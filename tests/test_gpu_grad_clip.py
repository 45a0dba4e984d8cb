"""The gradient-clipping passes (csrc/grad_clip.hip) through the C ABI on a synthetic table, against the numpy definition
(tests/grad_clip_ref.py): variables of 4 floats, of 1 float and 3 pad floats, of exactly one chunk, of two chunks (the
second of 4 floats), of 66 chunks (lanes 0 and 1 of the scales wave add two partials each) and 2100 variables of 4 floats
-- 2171 chunks, more than the 2048-wide grid and than the 256 threads of the global finish --, with floats between the
variables that must keep their bits."""
import ctypes

import numpy as np
import pytest

import grad_clip_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
CHUNK = 4096
GAP = 8                                    # floats between two variables, in no chunk
SIZES = [4, 1, CHUNK, CHUNK + 4, 65 * CHUNK + 4] + [4] * 2100
SPLITS = [1, 4, 5, 1000]                   # a part ends in front of these variables, the rest follows
C_NORM, C_VALUE = 5.0, 0.5


def _layout():
    """(chunk rows, variable rows, [(offset, padded count)], total floats): the chunk rules on SIZES, GAP floats apart."""
    chunks, variables, spans, at = [], [], [], GAP
    for j, n in enumerate(SIZES):
        padded = (n + 3) // 4 * 4
        first = len(chunks)
        for start in range(0, padded, CHUNK):
            chunks.append((at + start, min(CHUNK, padded - start), j, 0))
        variables.append((first, len(chunks) - first))
        spans.append((at, padded))
        at += padded + GAP
    return chunks, variables, spans, at


def _gradient(finite):
    """The values: see the cases in the comments.  finite: no inf, no NaN (the global norm of the other is NaN)."""
    chunks, variables, spans, total = _layout()
    rng = np.random.default_rng(7)
    g = rng.standard_normal(total).astype(F)                    # the gaps hold something, and must keep it
    var = lambda j: g[spans[j][0]:spans[j][0] + spans[j][1]]    # a view
    var(0)[:] = [3, 4, 0, 0]                                    # norm exactly 5: scale 1 at c = 5, bits kept
    var(1)[:] = [7, 0, 0, 0]                                    # one float above c, three pad floats
    var(2)[:] *= F(0.01)                                        # one chunk, norm ~0.64: below c
    var(2)[:8] = np.array([1e-45, -1e-45, 1e-40, -3e-39, -0.0, 0.0, 1e-38, -1e-38], F)      # denormals, signed zeros
    var(4)[:] *= F(0.5)                                         # 66 chunks, norm ~258; var(3): two chunks, norm ~64
    for k in range(2100):
        v = var(5 + k)
        if k % 5 == 0:
            v[:] = 0                                            # all zero: scale 1, no NaN
        elif k % 5 == 1:
            v[:] *= F(10.0)                                     # mostly above c
        elif k % 5 == 2:
            v[:] *= F(1e-3)                                     # far below
        elif k % 5 == 3:
            v[:] = np.array([1e-42, -2e-41, 0, -0.0], F)        # denormals alone: the sum of squares is ~1e-82, not 0
    var(5 + 4)[:] = [2.5, -2.5, 2.5, -2.5]                      # norm exactly 5 again
    if not finite:
        var(5 + 9)[1] = np.inf
        var(5 + 14)[2] = -np.inf
        var(5 + 19)[0] = np.nan
        var(5 + 24)[:] = np.array([0x7fc12345, 0xffc00001, 0x7f800001, 0x3f800000], np.uint32).view(F)   # NaN payloads
        var(3)[CHUNK + 1] = np.inf                              # in the 4-float second chunk of a two-chunk variable
    return g


@pytest.fixture(scope="module")
def env():
    import torch
    from lisec_amd import _lib, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    chunks, variables, spans, total = _layout()
    assert len(chunks) == 2171 and variables[4][1] == 66 and chunks[variables[3][0] + 1][1] == 4
    table = ops.lamb_table(chunks, variables, dev)
    ws = ops.clip_workspace(table.n_chunks, dev)
    assert ws.numel() == _lib.load().lisec_grad_clip_workspace_bytes(len(chunks)) == 8 * len(chunks)
    ref = {}
    for finite in (False, True):
        g = _gradient(finite)
        ref[finite] = dict(g=g, value=R.clip_by_value(g, C_VALUE, spans), norm=R.clip_by_norm(g, C_NORM, spans),
                           glob=R.clip_by_global_norm(g, C_NORM, spans), loose=R.clip_by_global_norm(g, 1e6, spans))
        for v in ref[finite].values():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    torch.cuda.synchronize()
    return dict(torch=torch, lib=_lib.load(), _lib=_lib, ops=ops, dev=dev, table=table, ws=ws, chunks=chunks,
                variables=variables, spans=spans, total=total, ref=ref)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _dev(env, a):
    return env["torch"].from_numpy(np.array(a, copy=True)).to(env["dev"])


def _host(env, t):
    env["torch"].cuda.synchronize()
    return t.cpu().numpy()


def _bufs(env, fill=-3.0):
    t = env["torch"]
    nv = len(env["variables"])
    return (t.full((nv,), fill, dtype=t.float32, device=env["dev"]), t.full((nv,), fill, dtype=t.float32, device=env["dev"]))


def _same(got, want):
    """Bit for bit -- except where the definition gives a NaN from a multiply (a NaN scale, or a NaN scaled): which
    payload such a product carries is the multiplier's business, so there only the NaN itself is asked for."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def _ulps(a, b):
    """The distance in float32 steps between two arrays of positive finite floats."""
    return np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64))


def _check_scales(got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    nan, one = np.isnan(want), want == F(1.0)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got[one]), _bits(want[one]))              # exactly 1.0f where the rule says so
    rest = ~nan & ~one
    assert (got[rest] < 1).all() and (got[rest] > 0).all()
    d = _ulps(got[rest], want[rest])
    print("scales: %d NaN, %d exactly one, %d below one, at most %d ulp from the definition" % (nan.sum(), one.sum(),
                                                                                               rest.sum(), d.max()))
    assert d.max() <= 1


def _check_norms(got, want):
    got, want = np.asarray(got, F), np.asarray(want, F)
    fin = np.isfinite(want)
    assert np.array_equal(_bits(got[~fin & ~np.isnan(want)]), _bits(want[~fin & ~np.isnan(want)]))       # the infinities
    assert np.array_equal(np.isnan(got), np.isnan(want))
    pos = fin & (want > 0)
    assert (got[fin & (want == 0)] == 0).all() and _ulps(got[pos], want[pos]).max() <= 1


@pytest.mark.parametrize("finite", [False, True], ids=["specials", "finite"])
def test_clipvalue_is_the_definition_bit_for_bit(env, finite):
    ref = env["ref"][finite]
    grad = _dev(env, ref["g"])
    env["ops"].grad_clip_value(grad, C_VALUE, table=env["table"])
    got = _host(env, grad)
    assert np.array_equal(_bits(got), _bits(ref["value"]))
    assert not np.array_equal(_bits(got), _bits(ref["g"]))
    if not finite:                                                          # +-inf became +-c, the NaNs kept their payloads
        a = env["spans"][5 + 24][0]
        assert _bits(got[a:a + 4]).tolist() == [0x7fc12345, 0xffc00001, 0x7f800001, _bits([C_VALUE])[0]]
        a = env["spans"][5 + 9][0]
        assert got[a + 1] == F(C_VALUE) and got[env["spans"][5 + 14][0] + 2] == F(-C_VALUE)
    # a part, then the rest: the bits of one launch
    for k in SPLITS:
        first = env["variables"][k][0]
        grad = _dev(env, ref["g"])
        env["ops"].grad_clip_value(grad, C_VALUE, table=env["table"], first=first)
        part = _host(env, grad)
        lo = env["spans"][k][0]
        assert np.array_equal(_bits(part[:lo]), _bits(ref["g"][:lo])) and np.array_equal(_bits(part[lo:]), _bits(got[lo:]))
        env["ops"].grad_clip_value(grad, C_VALUE, table=env["table"], first=0, n_chunks=first)
        assert np.array_equal(_bits(_host(env, grad)), _bits(got))


@pytest.mark.parametrize("finite", [False, True], ids=["specials", "finite"])
def test_clipnorm_scales_every_variable_by_the_definition(env, finite):
    ops, table, ref = env["ops"], env["table"], env["ref"][finite]
    want_g, want_s, want_n = ref["norm"]
    grad = _dev(env, ref["g"])
    scales, norms = _bufs(env)
    ops.grad_clip_norm(grad, C_NORM, table=table, scales=scales, norms=norms, workspace=env["ws"])
    got, s, n = _host(env, grad), _host(env, scales), _host(env, norms)
    _check_scales(s, want_s)
    _check_norms(n, want_n)
    assert s[0] == 1 and n[0] == 5 and s[5 + 4] == 1 and n[5 + 4] == 5 and s[5] == 1 and n[5] == 0      # 3-4-5, 2.5 x 4, zeros
    assert s[1] == F(5.0 / 7.0) and s[2] == 1
    assert 0 < s[3] < 1 if finite else np.isnan(s[3])                       # (the inf sits in its 4-float second chunk)
    assert 0 < s[4] < 0.03 and s[5 + 3] == 1 and 0 < n[5 + 3] < 1e-40
    # the clipped gradient is the float32 product with the scale read back, bit for bit; a scale of one (and every gap) keeps
    # its bits
    expect = np.array(ref["g"], copy=True)
    for (off, cnt), sc in zip(env["spans"], s):
        expect[off:off + cnt] = R.scaled(expect[off:off + cnt], sc)
    assert _same(got, expect)
    kept = [j for j, sc in enumerate(s) if sc == 1]
    assert len(kept) > 400
    for j in kept:
        off, cnt = env["spans"][j]
        assert np.array_equal(_bits(got[off:off + cnt]), _bits(ref["g"][off:off + cnt]))
    close = np.isfinite(want_g)
    np.testing.assert_allclose(got[close], want_g[close], rtol=2e-7, atol=0)
    # two runs agree bit for bit
    grad2 = _dev(env, ref["g"])
    s2, n2 = _bufs(env, 9.0)
    ops.grad_clip_norm(grad2, C_NORM, table=table, scales=s2, norms=n2, workspace=env["ws"])
    assert np.array_equal(_bits(_host(env, grad2)), _bits(got))
    assert np.array_equal(_bits(_host(env, s2)), _bits(s)) and np.array_equal(_bits(_host(env, n2)), _bits(n))
    # a part followed by the rest is one launch, bit for bit: slots of their own
    for k in SPLITS:
        first = env["variables"][k][0]
        grad2 = _dev(env, ref["g"])
        s2, n2 = _bufs(env)
        ops.grad_clip_norm(grad2, C_NORM, table=table, scales=s2, norms=n2, workspace=env["ws"], first=first, first_var=k)
        assert (_host(env, s2)[:k] == -3).all() and (_host(env, n2)[:k] == -3).all()
        lo = env["spans"][k][0]
        assert np.array_equal(_bits(_host(env, grad2)[:lo]), _bits(ref["g"][:lo]))
        ops.grad_clip_norm(grad2, C_NORM, table=table, scales=s2, norms=n2, workspace=env["ws"], first=0, n_chunks=first,
                           first_var=0, n_vars=k)
        assert np.array_equal(_bits(_host(env, grad2)), _bits(got)), k
        assert np.array_equal(_bits(_host(env, s2)), _bits(s)) and np.array_equal(_bits(_host(env, n2)), _bits(n))


def _global(env, g, c, parts=None):
    ops, table = env["ops"], env["table"]
    grad = _dev(env, g)
    scales, norms = _bufs(env)
    env["ws"].zero_()
    if parts is None:
        ops.grad_clip_global_norm(grad, c, table=table, scales=scales, norms=norms, workspace=env["ws"])
    else:
        ops.grad_clip_global_norm_partials(grad, table=table, workspace=env["ws"], first=parts)
        ops.grad_clip_global_norm_partials(grad, table=table, workspace=env["ws"], first=0, n_chunks=parts)
        ops.grad_clip_global_norm_finish(grad, c, table=table, scales=scales, norms=norms, workspace=env["ws"])
    return _host(env, grad), _host(env, scales), _host(env, norms)


def test_global_norm_scales_everything_by_one_factor(env):
    ref = env["ref"][True]
    want_g, want_s, want_n = ref["glob"]
    got, s, n = _global(env, ref["g"], C_NORM)
    _check_scales(s[:1], [want_s])
    _check_norms(n[:1], [want_n])
    assert 0 < s[0] < 0.02 and (s[1:] == -3).all() and (n[1:] == -3).all()             # slot 0 alone
    expect = np.array(ref["g"], copy=True)
    for off, cnt in env["spans"]:
        expect[off:off + cnt] = R.scaled(expect[off:off + cnt], s[0])
    assert np.array_equal(_bits(got), _bits(expect))
    np.testing.assert_allclose(got, want_g, rtol=2e-7, atol=0)
    # the sum of squares in two parts, and again in one: the same bits
    for k in SPLITS:
        g2, s2, n2 = _global(env, ref["g"], C_NORM, parts=env["variables"][k][0])
        assert np.array_equal(_bits(g2), _bits(got)) and s2[0] == s[0] and n2[0] == n[0], k
    g2, s2, n2 = _global(env, ref["g"], C_NORM)
    assert np.array_equal(_bits(g2), _bits(got)) and _bits(s2[:1]) == _bits(s[:1]) and _bits(n2[:1]) == _bits(n[:1])
    # finish over a chunk range scales that range alone
    grad = _dev(env, ref["g"])
    scales, norms = _bufs(env)
    first = env["variables"][5][0]
    env["ops"].grad_clip_global_norm_partials(grad, table=env["table"], workspace=env["ws"])
    env["ops"].grad_clip_global_norm_finish(grad, C_NORM, table=env["table"], scales=scales, norms=norms,
                                            workspace=env["ws"], first=first)
    part, lo = _host(env, grad), env["spans"][5][0]
    assert np.array_equal(_bits(part[:lo]), _bits(ref["g"][:lo])) and np.array_equal(_bits(part[lo:]), _bits(got[lo:]))
    # a threshold above the norm: scale exactly one, every bit kept
    got, s, n = _global(env, ref["g"], 1e6)
    assert s[0] == 1 and _ulps(n[:1], [ref["loose"][2]]).max() <= 1 and np.array_equal(_bits(got), _bits(ref["g"]))
    # an inf or a NaN anywhere: the scale is NaN, and so is every float of every chunk -- the gaps keep their bits
    bad = env["ref"][False]
    got, s, n = _global(env, bad["g"], C_NORM)
    assert np.isnan(s[0]) and np.isnan(n[0]) == np.isnan(bad["glob"][2]) and not np.isfinite(n[0])
    inside = np.zeros(env["total"], bool)
    for off, cnt in env["spans"]:
        inside[off:off + cnt] = True
    assert np.isnan(got[inside]).all() and np.array_equal(_bits(got[~inside]), _bits(bad["g"][~inside]))


def test_every_refusal_leaves_everything_untouched(env):
    lib, t, P = env["lib"], env["torch"], env["_lib"].ptr
    table, ws = env["table"], env["ws"]
    g0 = env["ref"][True]["g"]
    grad = _dev(env, g0)
    scales, norms = _bufs(env)
    ws.fill_(0x5a)
    ws0 = _host(env, ws).copy()
    nc, nv, st = table.n_chunks, table.n_vars, env["_lib"].current_stream()
    off = lambda x, b: ctypes.c_void_p(x.data_ptr() + b)
    G, T, V, S, N, W, B = P(grad), P(table.chunks), P(table.variables), P(scales), P(norms), P(ws), ws.numel()
    bad_c = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
    calls = []
    calls += [lambda c=c: lib.lisec_grad_clip_value(G, T, 0, nc, c, st) for c in bad_c]
    calls += [lambda: lib.lisec_grad_clip_value(None, T, 0, nc, 1.0, st), lambda: lib.lisec_grad_clip_value(G, None, 0, nc, 1.0, st),
              lambda: lib.lisec_grad_clip_value(off(grad, 4), T, 0, nc, 1.0, st),
              lambda: lib.lisec_grad_clip_value(G, off(table.chunks, 4), 0, nc, 1.0, st),
              lambda: lib.lisec_grad_clip_value(G, T, -1, nc, 1.0, st), lambda: lib.lisec_grad_clip_value(G, T, 0, -1, 1.0, st)]
    norm = lambda g=G, tb=T, fc=0, n=nc, v=V, fv=0, m=nv, c=1.0, s=S, no=N, w=W, b=B: lib.lisec_grad_clip_norm(
        g, tb, fc, n, v, fv, m, c, s, no, w, b, st)
    calls += [lambda c=c: norm(c=c) for c in bad_c]
    calls += [lambda: norm(g=None), lambda: norm(tb=None), lambda: norm(v=None), lambda: norm(s=None), lambda: norm(no=None),
              lambda: norm(w=None), lambda: norm(g=off(grad, 8)), lambda: norm(w=off(ws, 4)), lambda: norm(s=off(scales, 2)),
              lambda: norm(no=off(norms, 1)), lambda: norm(v=off(table.variables, 2)), lambda: norm(fc=-1), lambda: norm(n=-2),
              lambda: norm(fv=-1), lambda: norm(m=-1), lambda: norm(n=0), lambda: norm(m=0), lambda: norm(n=3, m=4),
              lambda: norm(b=B - 8), lambda: norm(b=0)]
    parts = lambda g=G, tb=T, fc=0, n=nc, w=W, b=B: lib.lisec_grad_clip_global_norm_partials(g, tb, fc, n, w, b, st)
    calls += [lambda: parts(g=None), lambda: parts(tb=None), lambda: parts(w=None), lambda: parts(g=off(grad, 4)),
              lambda: parts(w=off(ws, 4)), lambda: parts(fc=-1), lambda: parts(n=-1), lambda: parts(b=B - 1),
              lambda: parts(fc=1, n=nc)]
    fin = lambda g=G, tb=T, tc=nc, fc=0, n=nc, c=1.0, s=S, no=N, w=W, b=B: lib.lisec_grad_clip_global_norm_finish(
        g, tb, tc, fc, n, c, s, no, w, b, st)
    calls += [lambda c=c: fin(c=c) for c in bad_c]
    calls += [lambda: fin(g=None), lambda: fin(tb=None), lambda: fin(s=None), lambda: fin(no=None), lambda: fin(w=None),
              lambda: fin(g=off(grad, 4)), lambda: fin(w=off(ws, 4)), lambda: fin(s=off(scales, 2)), lambda: fin(tc=-1),
              lambda: fin(fc=-1), lambda: fin(n=-1), lambda: fin(fc=1, n=nc), lambda: fin(tc=nc - 1), lambda: fin(b=B - 8)]
    for i, call in enumerate(calls):
        assert call() == -1, i                               # LISEC_EINVAL
    t.cuda.synchronize()
    assert np.array_equal(_bits(_host(env, grad)), _bits(g0))
    assert (_host(env, scales) == -3).all() and (_host(env, norms) == -3).all() and np.array_equal(_host(env, ws), ws0)
    # what is valid and enqueues nothing: an empty range
    assert lib.lisec_grad_clip_value(G, T, 5, 0, 1.0, st) == 0 and norm(n=0, m=0) == 0 and parts(n=0) == 0
    t.cuda.synchronize()
    assert np.array_equal(_bits(_host(env, grad)), _bits(g0)) and (_host(env, scales) == -3).all()
    assert lib.lisec_grad_clip_workspace_bytes(0) == 8 and lib.lisec_grad_clip_workspace_bytes(-4) == 8
