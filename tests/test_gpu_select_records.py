"""Selection of records on the device against the C oracle, residue for
residue (`==` on Ct.download()): rotate_fold_many / select_many /
select_records.

The product runs the key inner products of a fold step of all columns as
tiles of columns (prims.h sfp_ks_inner_aut_sum_cols, kernels
k_ks_inner_aut_sum_cols<2> / <4>: each key word and source index once per
tile, a left-over column through k_ks_inner_aut_sum); the oracle -- and the
product under SFHE_SELECT_COLS=0 -- folds column by column.  Engines share a
seed, so equal residues in means equal residues out.

rotate_fold_many runs on test_gpu_select's fold engines (13 limbs: beta = 3,
the whole P; 3 limbs: a tier, beta = 1; rings 2^12 and 2^10; every entry of
FOLDS) with 1, 2, 3, 4, 5 and 9 columns: every tile, partial tile and the
left-over column, under both tile widths.
"""
import numpy as np
import pytest

import sfhe
from test_select import GATE, SHAPES, Ctx, batches_of, make_input, target_lists
from test_gpu_select import FOLD_DEPTH, FOLD_KEYS, FOLD_SLOTS, FOLD_STEPS, FOLDS, same
from test_select_records import columns, expected

pytestmark = pytest.mark.gpu

DEFAULT_TILE, OTHER_TILE = 2, 4  # prims_hip.hip kFoldTileDefault
COLUMN_COUNTS = [1, 2, 3, 4, 5, 9]
KNOBS = {"default": {}, "cols0": {"SFHE_SELECT_COLS": "0"}, "other_tile": {"SFHE_SELECT_TILE": str(OTHER_TILE)}}


def launches(C, tile):
    """Launches of one sfp_ks_inner_aut_sum_cols call over C columns."""
    n = 0
    while C:
        C -= tile if C >= tile else 2 if C >= 2 else 1
        n += 1
    return n


def set_knobs(monkeypatch, knob):
    for k in ("SFHE_SELECT_COLS", "SFHE_SELECT_TILE", "SFHE_SELECT_FOLD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def fold_engines(hip_lib, oracle_lib):
    out = {}
    for logn in (12, 10):
        out[logn] = ({b: sfhe.Engine(b, mult_depth=FOLD_DEPTH, ring_dim=1 << logn, batch_size=FOLD_SLOTS,
                                     rotations=FOLD_KEYS, seed=77 + logn) for b in ("hip", "oracle")}, {})
    yield out
    for eng, _ in out.values():
        for e in eng.values():
            e.close()


def fold_inputs(eng, memo, limbs):
    """Per limb count: the columns encrypted on both backends and, per fold, the
    oracle's and the product's rotate_fold of every column (computed once)."""
    if limbs not in memo:
        rng = np.random.default_rng(5)
        vs = [rng.uniform(-1, 1, FOLD_SLOTS) for _ in range(max(COLUMN_COUNTS))]
        level = FOLD_DEPTH + 1 - limbs
        cts = {b: [e.encrypt(v.tolist(), level=level) for v in vs] for b, e in eng.items()}
        for h, o in zip(cts["hip"], cts["oracle"]):
            same(h, o, "input")
        assert cts["hip"][0].info()["limbs"] == limbs
        refs = {}
        for stride, count, _ in FOLDS:
            o = [eng["oracle"].rotate_fold(ct, stride, count) for ct in cts["oracle"]]
            h = [eng["hip"].rotate_fold(ct, stride, count) for ct in cts["hip"]]
            for a, b in zip(h, o):
                same(a, b, f"rotate_fold({stride}, {count})")
            refs[stride, count] = [x.download() for x in o]
        memo[limbs] = (vs, cts, refs)
    return memo[limbs]


@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("limbs", [FOLD_DEPTH + 1, 3])
@pytest.mark.parametrize("logn", [12, 10])
def test_rotate_fold_many_bitexact(fold_engines, monkeypatch, logn, limbs, knob):
    eng, memo = fold_engines[logn]
    monkeypatch.delenv("SFHE_SELECT_FOLD", raising=False)
    vs, cts, refs = fold_inputs(eng, memo, limbs)
    set_knobs(monkeypatch, knob)
    e = eng["hip"]
    tile = OTHER_TILE if knob == "other_tile" else DEFAULT_TILE
    for stride, count, rotating in FOLDS:
        for C in COLUMN_COUNTS:
            e.op_stats(reset=True)
            outs = e.rotate_fold_many(cts["hip"][:C], stride, count)
            want = (0, 0, C) if knob == "cols0" or not rotating else (0, launches(C, tile), 0)
            assert e.select_cols_counts() == want, (stride, count, C)
            for c, out in enumerate(outs):
                # == the oracle's rotate_fold of the column == the product's (fold_inputs checked those equal)
                got = out.download()
                bad = int(np.count_nonzero(got != refs[stride, count][c]))
                assert bad == 0, f"rotate_fold_many({stride}, {count}) C={C} column {c}: {bad} residues differ"
        roll = [sum(np.roll(v, -k * stride) for k in range(count)) for v in vs]
        for c, out in enumerate(outs):  # (the widest call's outputs)
            err = float(np.max(np.abs(np.array(e.decrypt(out))[:FOLD_SLOTS] - roll[c])))
            assert err < 1e-6, (stride, count, c, err)


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per shape: both contexts, the columns encrypted on both, each backend's rank."""
    out = {}
    for N, logn in SHAPES:
        c = {b: Ctx(b, N, logn) for b in ("hip", "oracle")}
        x = make_input(N)
        cols = columns(N, x, 5)
        cts = {b: [c[b].e.encrypt(v.tolist()) for v in cols] for b in c}
        ranks = {b: c[b].s.rank(cts[b][0], *c[b].cfg) for b in c}
        same(ranks["hip"], ranks["oracle"], "rank")
        out[N] = (c, x, cols, cts, ranks, {})
    yield out
    for v in out.values():
        for c in v[0].values():
            c.e.close()


@pytest.mark.parametrize("knob", ["default", "cols0"])
@pytest.mark.parametrize("N,logn,C,name", [(8, 12, 2, "five"), (8, 12, 5, "five"), (64, 12, 3, "forty")])
def test_select_many_bitexact(pairs, monkeypatch, N, logn, C, name, knob):
    c, x, cols, cts, ranks, memo = pairs[N]
    T = target_lists(N)[name]
    if (C, name) not in memo:
        memo[C, name] = c["oracle"].s.select_many(ranks["oracle"], cts["oracle"][:C], T)
    set_knobs(monkeypatch, knob)
    e = c["hip"].e
    e.op_stats(reset=True)
    outs = c["hip"].s.select_many(ranks["hip"], cts["hip"][:C], T)
    B = batches_of(N, logn, len(T))
    steps = FOLD_STEPS[N] * B
    assert e.select_counts()[0] == B
    assert e.select_cols_counts() == ((C, steps * launches(C, DEFAULT_TILE), 0) if knob == "default"
                                      else (C, 0, steps * C))
    for k, (got, ref) in enumerate(zip(outs, memo[C, name])):
        same(got, ref, f"select_many {name} column {k}")
        err = float(np.max(np.abs(np.array(e.decrypt(got))[:N] - expected(cols[k], x, T, N))))
        assert err < GATE, (k, err)


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("N,logn", SHAPES)
def test_select_records_with_the_rank_on_the_device(pairs, monkeypatch, N, logn, stable):
    set_knobs(monkeypatch, "default")
    c, x, cols, cts, ranks, _ = pairs[N]
    T = target_lists(N)["seven"]
    kw = dict(stable=stable, n=c["hip"].cfg[0], dg=c["hip"].cfg[1], df=c["hip"].cfg[2])
    got = {b: c[b].s.select_records(cts[b][0], cts[b][1:3], T, **kw) for b in c}
    same(got["hip"][0], got["oracle"][0], f"select_records keys stable={stable}")
    for k in range(2):
        same(got["hip"][1][k], got["oracle"][1][k], f"select_records column {k} stable={stable}")
    for k, out in enumerate([got["hip"][0]] + got["hip"][1]):
        err = float(np.max(np.abs(np.array(c["hip"].e.decrypt(out))[:N] - expected(cols[k], x, T, N))))
        assert err < GATE, (k, err)


def test_select_ranked_reports_its_parent_counts(pairs, monkeypatch):
    """selectRanks is untouched by the refactoring: one fused fold per step and
    batch, and none of the multi-column counters moves."""
    set_knobs(monkeypatch, "default")
    N, logn = 8, 12
    c, x, cols, cts, ranks, _ = pairs[N]
    T = target_lists(N)["five"]
    e = c["hip"].e
    e.op_stats(reset=True)
    out = c["hip"].s.select_ranked(ranks["hip"], cts["hip"][0], T)
    B = batches_of(N, logn, len(T))
    assert e.select_counts() == (B, FOLD_STEPS[N] * B, 0)
    assert e.select_cols_counts() == (0, 0, 0)
    same(out, c["oracle"].s.select_ranked(ranks["oracle"], cts["oracle"][0], T), "select_ranked")
