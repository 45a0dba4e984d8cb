"""The shared pieces of the chunk tables (lisec_amd.ops): ChunkTable.span / at on the network's real layout for the
regulariser's, the decay's and LAMB's tables, and select_variables.  No GPU: the tables are built on "cpu"."""
import pytest

from lisec_amd import _lib, ops
from lisec_amd.params import TRAINABLE_KINDS


@pytest.fixture(scope="module")
def store():
    import torch
    from lisec_amd.params import ParamStore
    return ParamStore(torch.device("cpu"))


def _boundaries(store):
    """Every variable boundary of theta, 0 and n_theta included."""
    return sorted({off for which, off, _ in store.offsets.values() if which == "theta"} | {store.n_theta})


def _reg(store):
    # kernels and betas only, one of them with a (0, 0) pair: the table has holes
    coeffs = {n: (0.0, 1e-4) for n, _, k in store.specs if k == "kernel"}
    coeffs.update({n: (0.5, 0.0) for n, _, k in store.specs if k == "beta"})
    coeffs["rpn2.conv3.kernel"] = (0.0, 0.0)
    return ops.reg_table(ops.reg_chunks(store, coeffs, unwritten=("mid2.conv.bias",)), "cpu")


def _decay(store):
    return ops.decay_table(ops.decay_chunks(store, ("kernel", "gamma")), "cpu")


def _lamb_chunks(store):
    return ops.lamb_table(*ops.lamb_chunks(store, ("bias", "gamma", "beta")), "cpu").chunks


TABLES = {"regularize": _reg, "decay": _decay, "lamb": _lamb_chunks}


@pytest.mark.parametrize("kind", sorted(TABLES))
def test_span_cuts_a_table_in_two_at_every_variable_boundary(store, kind):
    table = TABLES[kind](store)
    n, rows = store.n_theta, table.rows
    assert len(table) == len(rows) == len(table.offsets) > 0 and table.offsets == [r[0] for r in rows]
    assert table.records.numel() == len(rows) * {"regularize": 24, "decay": 16, "lamb": 24}[kind]
    if kind != "lamb":                                           # holes: variables without a row
        assert sum(r[1] for r in rows) < n
    bounds = _boundaries(store)
    assert bounds[0] == 0 and bounds[-1] == n and len(bounds) == len(store.trainable_names()) + 1
    assert table.span(0, n) == (0, len(rows))
    for b in bounds:
        first_a, count_a = table.span(0, b)
        first_b, count_b = table.span(b, n)
        assert first_a == 0 and first_b == count_a and count_a + count_b == len(rows)      # adjacent, and every row
        assert all(off + count <= b for off, count, *_ in rows[:count_a])
        assert all(off >= b for off, *_ in rows[first_b:first_b + count_b])
        assert table.span(b, b) == (first_b, 0)                                            # empty


def test_lamb_chunk_span_is_the_chunks_of_the_variable_span(store):
    table = ops.lamb_table(*ops.lamb_chunks(store, ("bias", "gamma", "beta")), "cpu")
    n, variables = store.n_theta, table.variables.rows
    assert (table.n_chunks, table.n_vars) == (len(table.chunks), len(table.variables)) == (len(table.chunks.rows), len(variables))
    assert table.names == [v[3] for v in variables] == sorted(store.trainable_names(), key=lambda x: store.offsets[x][1])
    assert table.variables.offsets == [v[2] for v in variables]
    for b in _boundaries(store):
        for lo, hi in ((0, b), (b, n)):
            first, n_chunks = table.chunks.span(lo, hi)
            first_var, n_vars = table.variables.span(lo, hi)
            part = variables[first_var:first_var + n_vars]
            assert n_chunks == sum(v[1] for v in part)
            assert first == (variables[first_var][0] if first_var < len(variables) else len(table.chunks))
            assert all(lo <= v[2] < hi for v in part)
        first_var, n_vars = table.variables.span(0, b)
        assert first_var == 0 and table.variables.span(b, n) == (n_vars, len(variables) - n_vars)
        assert table.variables.span(b, b)[1] == 0 and table.chunks.span(b, b)[1] == 0
    # variable rows of two fields (no offset, no name) are keyed by their first chunk all the same
    bare = ops.lamb_table(table.chunks.rows, [v[:2] for v in variables], "cpu")
    assert bare.variables.offsets == table.variables.offsets and bare.names == []


def test_a_table_without_rows_spans_nothing(store):
    for table in (ops.reg_table([], "cpu"), ops.decay_table(ops.decay_chunks(store, ()), "cpu"),
                  ops.lamb_table([], [], "cpu").chunks, ops.lamb_table([], [], "cpu").variables):
        assert len(table) == 0 and table.rows == [] and table.offsets == []
        for lo, hi in ((0, 0), (0, store.n_theta), (4096, 8192), (store.n_theta, store.n_theta)):
            assert table.span(lo, hi) == (0, 0)
        assert table.records.numel() > 0                         # one zeroed record: never a NULL table
        table.at(0, 0, "empty")
        with pytest.raises(ValueError):
            table.at(0, 1, "empty")


@pytest.mark.parametrize("kind", sorted(TABLES))
def test_at_checks_the_rows_and_returns_the_record_address(store, kind):
    import ctypes
    table = TABLES[kind](store)
    n, size = len(table), ctypes.sizeof(table.record)
    base = table.records.data_ptr()
    assert table.at(0, n, "t").value == base and table.at(3, n - 3, "t").value == base + 3 * size
    assert table.at(n, 0, "t").value == base + n * size          # no rows at the end of the table: valid
    assert table.at(n - 1, 1, "t").value == base + (n - 1) * size
    for first, count in ((-1, 1), (-1, 0), (0, n + 1), (1, n), (n, 1), (n + 1, 0), (0, -1)):
        with pytest.raises(ValueError, match=r"who: rows \[-?\d+, -?\d+\) outside a table of %d" % n):
            table.at(first, count, "who")


def test_select_variables(store):
    sel = ops.select_variables
    assert sel(store, "cls.bias", "x") == sel(store, ["cls.bias"], "x") == ["cls.bias"]
    assert sel(store, "beta", "x") == sel(store, ("beta",), "x")
    assert sel(store, ["cls.bias", "up3.kernel", "cls.bias"], "x") == ["cls.bias", "up3.kernel"]     # named twice: once
    assert sel(store, (), "x") == []
    for kind in TRAINABLE_KINDS:                                 # a kind: its variables in the order of params.specs
        assert sel(store, [kind], "x") == [n for n, _, k in store.specs if k == kind] != []
    gammas = [n for n, _, k in store.specs if k == "gamma"]
    assert sel(store, ["up3.kernel", "gamma", gammas[2], "cls.bias"], "x") == ["up3.kernel"] + gammas + ["cls.bias"]
    assert sorted(sel(store, TRAINABLE_KINDS, "x")) == sorted(store.trainable_names())
    assert sel(store, iter(["cls.bias", "gamma"]), "x") == ["cls.bias"] + gammas                     # any iterable


CALLERS = {
    "decayed": lambda store, names: ops.decay_chunks(store, names),
    "excluded from an update": lambda store, names: ops.lamb_chunks(store, names),
    "excluded from an update (adaptation)": lambda store, names: ops.lamb_chunks(store, None, names),
}


@pytest.mark.parametrize("what", sorted(CALLERS))
def test_select_variables_refusals_reach_both_callers(store, what):
    call = CALLERS[what]
    words = what.split(" (")[0]
    with pytest.raises(KeyError):
        call(store, ["no.such.kernel"])
    with pytest.raises(KeyError):
        call(store, ["moving_mean"])                             # not a kind of trainable variable
    for moving in ("mid1.bn.moving_mean", "rpn1.bn0.moving_variance"):   # the moving statistics are not trained
        with pytest.raises(ValueError, match=f"{moving} is not a trainable variable: it cannot be {words}$"):
            call(store, ["kernel", moving])
        with pytest.raises(ValueError, match=f"it cannot be {words}$"):
            ops.select_variables(store, [moving], words)
    with pytest.raises(KeyError):
        ops.select_variables(store, ["kernel", "no.such.kernel"], words)


def test_the_cutter_is_what_every_table_is_made_of(store):
    for name in ("cls.bias", "rpn2.conv3.kernel", "vfe1.bn.beta", "up3.kernel"):
        _, off, shape = store.offsets[name]
        n = 1
        for s in shape:
            n *= s
        padded = (n + 3) // 4 * 4
        chunks = list(ops.variable_chunks(store, name))
        assert len(chunks) == -(-padded // _lib.REG_CHUNK) and chunks[0][0] == off
        assert sum(c for _, c in chunks) == padded and all(0 < c <= _lib.REG_CHUNK and c % 4 == 0 for _, c in chunks)
        assert all(a[0] + a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert chunks == ops.decay_chunks(store, name)
        assert chunks == [r[:2] for r in ops.reg_chunks(store, {name: (0.5, 0.25)})]
        assert chunks == [c[:2] for c in ops.lamb_chunks(store)[0] if off <= c[0] < off + padded]
