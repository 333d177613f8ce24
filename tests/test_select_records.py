"""Selection of records (DirectSort<N>::selectRanksMany / selectRecords,
EvalRotateFoldMany) on the C oracle.

select_many(rank, [c0, c1, ...], T): column c holds the residues of
select_ranked(rank, c, T) -- the indicator of a batch is evaluated once for
all columns, which changes no residue.  The oracle has no column-tiled
primitive, so rotate_fold_many is rotate_fold per column there and the
counters say so.

Shapes, inputs, target lists and the gate are tests/test_select.py's.  The
payload columns are cos / sin / index-derived vectors of the keys' indices in
[-1, 1], all distinct, so swapped columns are caught.
"""
import numpy as np
import pytest

import sfhe
from test_select import GATE, SHAPES, Ctx, Ranked, batches_of, make_input, target_lists
from test_gpu_select import FOLD_DEPTH, FOLD_KEYS, FOLD_SLOTS, FOLD_STEPS, FOLDS

MANY = [(8, 12, C, name) for C in (1, 2, 3, 5, 8) for name in ("min", "five", "all")] + \
       [(64, 12, 3, "seven"), (64, 12, 3, "forty")]


def columns(N, x, C):
    """C distinct columns in [-1, 1]: the keys, then functions of the index."""
    i = np.arange(N)
    gen = [x, np.cos(i), np.sin(i), 2.0 * i / N - 1.0, np.cos(2 * i + 1), np.sin(3 * i + 2), 1.0 - 2.0 * i / N,
           np.cos(5 * i + 3)]
    return [np.asarray(v, dtype=float) for v in gen[:C]]


def expected(col, keys, T, N, stable=False):
    want = np.zeros(N)
    want[: len(T)] = col[np.argsort(keys, kind="stable" if stable else None)][T]
    return want


@pytest.fixture(scope="module")
def ranked(oracle_lib):
    out = {(N, logn): Ranked(N, logn) for N, logn in SHAPES}
    for r in out.values():
        r.cols = columns(r.c.N, r.x, sfhe.MAX_COLUMNS)
        r.cts = [r.ct] + [r.c.e.encrypt(v.tolist()) for v in r.cols[1:]]
        r.memo = {}
    yield out
    for r in out.values():
        r.c.e.close()


def separate(r, c, name, T):
    """select_ranked of column c (computed once per column and target list)."""
    if (c, name) not in r.memo:
        r.memo[c, name] = r.c.s.select_ranked(r.rank, r.cts[c], T).download()
    return r.memo[c, name]


@pytest.mark.parametrize("N,logn,C,name", MANY)
def test_select_many_equals_the_separate_calls(ranked, N, logn, C, name):
    r = ranked[N, logn]
    T = target_lists(N)[name]
    refs = [separate(r, c, name, T) for c in range(C)]
    r.c.e.op_stats(reset=True)
    outs = r.c.s.select_many(r.rank, r.cts[:C], T)
    B = batches_of(N, logn, len(T))
    assert r.c.e.select_counts()[0] == B  # a batch is counted once, not once per column
    # the oracle composes: every column of every fold step of every batch
    assert r.c.e.select_cols_counts() == (C, 0, C * FOLD_STEPS[N] * B)
    assert len(outs) == C
    for c, out in enumerate(outs):
        assert np.array_equal(out.download(), refs[c]), f"column {c} differs from select_ranked"
        assert out.level == r.place_level and out.slots == N
        err = float(np.max(np.abs(np.array(r.c.e.decrypt(out))[:N] - expected(r.cols[c], r.x, T, N))))
        assert err < GATE, (c, err)


@pytest.mark.parametrize("N,logn", SHAPES)
def test_select_records_is_stable_on_duplicate_keys(ranked, N, logn):
    """Input (b): every key occurs twice; the index column shows that equal
    keys' rows come out in input order."""
    c = ranked[N, logn].c
    kw = dict(n=c.cfg[0], dg=c.cfg[1], df=c.cfg[2])
    x = make_input(N, "b")
    idx = np.arange(N) / N
    other = np.cos(np.arange(N))
    keys, p_idx, p_other = (c.e.encrypt(v.tolist()) for v in (x, idx, other))
    T = list(range(N)) if N == 8 else target_lists(N)["seven"]
    c.e.op_stats(reset=True)
    keys_out, outs = c.s.select_records(keys, [p_idx, p_other], T, stable=True, **kw)
    assert c.e.select_cols_counts()[0] == 3
    assert np.array_equal(keys_out.download(), c.s.select(keys, T, stable=True, **kw).download())
    for got, col in ((keys_out, x), (outs[0], idx), (outs[1], other)):
        err = float(np.max(np.abs(np.array(c.e.decrypt(got))[:N] - expected(col, x, T, N, stable=True))))
        assert err < GATE, err
    if N == 8:
        k = 3
        kout, (iout,) = c.s.top_k_records(keys, [p_idx], k, largest=True, **kw)
        order = np.argsort(x, kind="stable")[::-1][:k]
        for got, col in ((kout, x), (iout, idx)):
            want = np.r_[col[order], np.zeros(N - k)]
            assert float(np.max(np.abs(np.array(c.e.decrypt(got))[:N] - want))) < GATE
        # no payload columns: the keys alone
        kout0, none = c.s.select_records(keys, (), [0], stable=True, **kw)
        assert none == [] and abs(c.e.decrypt(kout0)[0] - np.sort(x)[0]) < GATE


@pytest.mark.parametrize("C", [1, 3])
def test_rotate_fold_many_equals_rotate_fold(oracle_lib, C):
    e = sfhe.Engine("oracle", mult_depth=FOLD_DEPTH, ring_dim=1 << 10, batch_size=FOLD_SLOTS, rotations=FOLD_KEYS,
                    seed=77 + 10)
    rng = np.random.default_rng(6)
    vs = [rng.uniform(-1, 1, FOLD_SLOTS) for _ in range(C)]
    cts = [e.encrypt(v.tolist(), level=FOLD_DEPTH + 1 - 3) for v in vs]
    assert cts[0].info()["limbs"] == 3
    for stride, count, rotating in FOLDS:
        e.op_stats(reset=True)
        outs = e.rotate_fold_many(cts, stride, count)
        assert e.select_cols_counts() == (0, 0, C)
        assert e.select_counts() == (0, 0, C if rotating else 0)
        for ct, v, out in zip(cts, vs, outs):
            assert np.array_equal(out.download(), e.rotate_fold(ct, stride, count).download()), (stride, count)
            want = sum(np.roll(v, -k * stride) for k in range(count))
            assert float(np.max(np.abs(np.array(e.decrypt(out))[:FOLD_SLOTS] - want))) < 1e-6
    with pytest.raises(sfhe.SfheError, match="one level"):
        e.rotate_fold_many([cts[0], e.encrypt(vs[0].tolist(), level=1)], 1, 4)
    for bad in ([], [cts[0], None]):
        with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
            e.rotate_fold_many(bad, 1, 4)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
        e.rotate_fold_many(cts, 1, 9)
    e.close()


def test_argument_errors(ranked):
    N, logn = 8, 12
    r = ranked[N, logn]
    s, T = r.c.s, [0, 1]
    kw = dict(n=r.c.cfg[0], dg=r.c.cfg[1], df=r.c.cfg[2])
    with pytest.raises(sfhe.SfheError, match="one level"):
        s.select_many(r.rank, [r.ct, r.c.e.encrypt(r.cols[1].tolist(), level=1)], T)
    for bad in ([], [r.ct] * (sfhe.MAX_COLUMNS + 1), [r.ct, None]):
        with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
            s.select_many(r.rank, bad, T)
    for bad in ([r.ct] * (sfhe.MAX_COLUMNS + 1), [None]):
        with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
            s.select_records(r.ct, bad, T, **kw)
    for bad in ([0, 0], [N], [], list(range(N)) + [0], [-1]):
        with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
            s.select_many(r.rank, r.cts[:2], bad)
        with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
            s.select_records(r.ct, r.cts[1:2], bad, **kw)
    # the engine still works
    out = s.select_many(r.rank, r.cts[:2], [0])
    assert np.array_equal(out[1].download(), separate(r, 1, "min", [0]))


def test_depth_too_small_names_the_depth(oracle_lib):
    N, logn = 8, 12
    depth = sfhe.select_params(N, "oracle")[0]
    short = Ctx("oracle", N, logn, depth=depth - 1)
    ct = short.e.encrypt(make_input(N).tolist())
    rank = short.s.rank(ct, *short.cfg)
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {depth}\b"):
        short.s.select_many(rank, [ct, ct], [0])
    short.e.close()


def test_abi_lists_the_record_selection_entry_points(oracle_lib):
    for name in ("sfhe_sorter_select_many", "sfhe_sorter_select_records", "sfhe_eval_rotate_fold_many",
                 "sfhe_select_cols_counts"):
        assert hasattr(oracle_lib, name), name
        assert name in sfhe.ABI_SYMBOLS
