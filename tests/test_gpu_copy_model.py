"""Two live groups and the copies between them model-checked on the device: the sequences of tests/copy_model.py (inserts,
retires, set_bits, compactions, a finalize, copies A -> B and B -> A with random lists, planned refusals) replayed through
the Python objects and compared with the two host models after EVERY step -- what the call returns (or the error code,
with kwage_last_error set), and for BOTH groups the span, the column count, the row bytes, real_columns() and every row
through read_rows, all exact.  tests/test_copy_model.py checks the sequences themselves without a device."""
import numpy as np
import pytest

import copy_model as cm

pytestmark = pytest.mark.gpu

STAT_KEYS = ("span_before", "span_after", "columns", "runs", "first_unit", "units")


@pytest.fixture(scope="module")
def ka():
    import kwage_amd as ka
    from kwage_amd import native
    native.ensure_built()
    return ka


@pytest.fixture(scope="module")
def ctx(ka):
    c = ka.Context(0)
    yield c
    c.close()


def call(ka, groups, op):
    """The step on the device groups -> what the model returns for it (the error code where the call is refused)."""
    from kwage_amd.native import lib
    g = groups[op.on]
    try:
        if op.kind == "add_columns":
            return g.add_columns(op.image, op.nf)
        if op.kind == "insert":
            return g.insert_filters(op.filters)
        if op.kind == "copy":
            return g.copy_columns_from(groups[op.src], op.cols)[0]
        if op.kind == "retire":
            g.retire_columns(op.cols)
        elif op.kind == "set_bits":
            g.set_bits(op.rows, op.cols)
        elif op.kind == "compact":
            new, st = g.compact()
            return new, {key: int(st[key]) for key in STAT_KEYS}
        elif op.kind == "finalize":
            g.finalize()
        return 0
    except ka.KwageError as e:
        assert e.code < 0 and lib().kwage_last_error(), op
        return e.code


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_sequence(ka, ctx, seed):
    ops = cm.sequence(seed)
    models = cm.fresh_models()
    groups = {name: ka.Group(ctx, cm.K, cm.NH, cm.L, cm.CAPACITY) for name in "AB"}
    nrows = 1 << cm.L
    try:
        assert all(groups[name].row_stride == models[name].stride for name in "AB")
        for step, op in enumerate(ops):
            what = (seed, step, op)
            want = cm.apply(models, op)
            got = call(ka, groups, op)
            if op.kind == "compact":
                assert np.array_equal(got[0], want[0]) and got[1] == {key: want[1][key] for key in STAT_KEYS}, what
            else:
                assert got == want and op.refused() == (got < 0), (what, got, want)
            # the state of BOTH groups, all of it, exact (a refused call moved neither model, so it may move neither group)
            for name in "AB":
                g, m = groups[name], models[name]
                assert (g.column_span, g.num_columns, g.row_bytes) == (m.span, m.num_columns, m.span // 8), (what, name)
                assert np.array_equal(g.real_columns(), m.real), (what, name)
                if m.span:
                    rows = g.read_rows(np.arange(nrows))
                    assert np.array_equal(rows, m.packed()), (what, name, np.argwhere(rows != m.packed())[:5])
    finally:
        for g in groups.values():
            g.close()
