"""Selection by rank on the device against the C oracle, residue for residue
(`==` on Ct.download()): select_ranked / select / rotate_fold.

Both backends run the same integer program.  The product sums the key inner
products of a fold's rotations in one launch (prims.h sfp_ks_inner_aut_sum,
kernel k_ks_inner_aut_sum: the shared digits read through every automorphism,
128-bit accumulators, one reduction); the oracle -- and the product under
SFHE_SELECT_FOLD=0 -- permutes the digits and accumulates per term.  Engines
share a seed, so equal residues in means equal residues out.

Shapes and target lists as tests/test_select.py.  rotate_fold alone runs where
the kernel's geometry differs: level 0 of a depth-12 context (13 limbs, above
the largest special-prime tier bound, beta = 3 digits, the whole P) and a
level with 3 limbs (a tier, beta = 1), counts 2, 4 and 8 (R = 1, 3, 7 rotating
terms), a stride that is a multiple of the slot count (identity terms only)
and one that mixes both kinds, at ring 2^12 and at ring 2^10 (the single-pass
NTT ring).
"""
import numpy as np
import pytest

import sfhe
from test_select import CASES, GATE, SHAPES, Ctx, batches_of, check, make_input, target_lists

pytestmark = pytest.mark.gpu

FOLD_STEPS = {8: 2, 64: 3}


def same(a, b, what):
    x, y = a.download(), b.download()
    assert x.shape == y.shape and a.level == b.level, (what, x.shape, y.shape, a.level, b.level)
    bad = int(np.count_nonzero(x != y))
    assert bad == 0, f"{what}: {bad} of {x.size} residues differ"


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per shape: both contexts, the input encrypted on both, each backend's
    rank, and a memo of the oracle's select_ranked per target list."""
    out = {}
    for N, logn in SHAPES:
        c = {b: Ctx(b, N, logn) for b in ("hip", "oracle")}
        x = make_input(N)
        cts = {b: c[b].e.encrypt(x.tolist()) for b in c}
        ranks = {b: c[b].s.rank(cts[b], *c[b].cfg) for b in c}
        same(ranks["hip"], ranks["oracle"], "rank")
        out[N] = (c, x, cts, ranks, {})
    yield out
    for v in out.values():
        for c in v[0].values():
            c.e.close()


def reference(pair, name, T):
    c, x, cts, ranks, memo = pair
    if name not in memo:
        memo[name] = c["oracle"].s.select_ranked(ranks["oracle"], cts["oracle"], T)
    return memo[name]


@pytest.mark.parametrize("knob", [None, "0"])
@pytest.mark.parametrize("N,logn,name", CASES)
def test_select_ranked_bitexact(pairs, monkeypatch, N, logn, name, knob):
    if knob is None:
        monkeypatch.delenv("SFHE_SELECT_FOLD", raising=False)
    else:
        monkeypatch.setenv("SFHE_SELECT_FOLD", knob)
    c, x, cts, ranks, _ = pairs[N]
    T = target_lists(N)[name]
    ref = reference(pairs[N], name, T)
    e, s = c["hip"].e, c["hip"].s
    e.op_stats(reset=True)
    out = s.select_ranked(ranks["hip"], cts["hip"], T)
    B = batches_of(N, logn, len(T))
    folds = FOLD_STEPS[N] * B
    assert e.select_counts() == ((B, folds, 0) if knob is None else (B, 0, folds))
    same(out, ref, f"select_ranked {name}")
    err = check(e.decrypt(out), np.sort(x), T, N)
    assert err < GATE, err


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("N,logn", SHAPES)
def test_select_with_the_rank_on_the_device(pairs, monkeypatch, N, logn, stable):
    monkeypatch.delenv("SFHE_SELECT_FOLD", raising=False)
    c, x, cts, ranks, _ = pairs[N]
    T = target_lists(N)["seven"]
    kw = dict(stable=stable, n=c["hip"].cfg[0], dg=c["hip"].cfg[1], df=c["hip"].cfg[2])
    got = c["hip"].s.select(cts["hip"], T, **kw)
    same(got, c["oracle"].s.select(cts["oracle"], T, **kw), f"select stable={stable}")
    assert check(c["hip"].e.decrypt(got), np.sort(x), T, N) < GATE


FOLD_SLOTS = 64
FOLD_DEPTH = 12
FOLD_KEYS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 32, 48]
# (stride, count, rotating terms): 64 = the slot count (identity terms only), 32 mixes both kinds
FOLDS = [(1, 2, 1), (1, 4, 3), (1, 8, 7), (4, 4, 3), (16, 4, 3), (64, 3, 0), (32, 4, 2)]


@pytest.fixture(scope="module")
def fold_engines(hip_lib, oracle_lib):
    out = {}
    for logn in (12, 10):
        eng = {b: sfhe.Engine(b, mult_depth=FOLD_DEPTH, ring_dim=1 << logn, batch_size=FOLD_SLOTS,
                              rotations=FOLD_KEYS, seed=77 + logn) for b in ("hip", "oracle")}
        out[logn] = eng
    yield out
    for eng in out.values():
        for e in eng.values():
            e.close()


@pytest.mark.parametrize("knob", [None, "0"])
@pytest.mark.parametrize("limbs", [FOLD_DEPTH + 1, 3])
@pytest.mark.parametrize("logn", [12, 10])
def test_rotate_fold_bitexact(fold_engines, monkeypatch, logn, limbs, knob):
    if knob is None:
        monkeypatch.delenv("SFHE_SELECT_FOLD", raising=False)
    else:
        monkeypatch.setenv("SFHE_SELECT_FOLD", knob)
    eng = fold_engines[logn]
    info = eng["hip"].info()
    assert info["num_q"] == FOLD_DEPTH + 1 and info["dnum"] == 3  # alpha = 5: beta = 3 at 13 limbs, 1 at 3
    v = np.random.default_rng(5).uniform(-1, 1, FOLD_SLOTS)
    level = FOLD_DEPTH + 1 - limbs
    cts = {b: e.encrypt(v.tolist(), level=level) for b, e in eng.items()}
    same(cts["hip"], cts["oracle"], "input")
    assert cts["hip"].info()["limbs"] == limbs
    for stride, count, rotating in FOLDS:
        eng["hip"].op_stats(reset=True)
        got = eng["hip"].rotate_fold(cts["hip"], stride, count)
        want_counts = (0, 0, 0) if not rotating else (0, 1, 0) if knob is None else (0, 0, 1)
        assert eng["hip"].select_counts() == want_counts, (stride, count)
        same(got, eng["oracle"].rotate_fold(cts["oracle"], stride, count), f"rotate_fold({stride}, {count})")
        want = sum(np.roll(v, -k * stride) for k in range(count))
        err = float(np.max(np.abs(np.array(eng["hip"].decrypt(got))[:FOLD_SLOTS] - want)))
        assert err < 1e-6, (stride, count, err)
