"""Records ordered by several keys (DirectSort<N>::constructRankLex /
sortRecordsLex / selectRecordsLex) on the C oracle.

rank_lex counts, for every row r, the rows j before it in (key_1, ..., key_m,
input index) order, key i descending where asked:
argsort(lexsort((index, ...keys with the descending ones negated))).

Shapes as tests/test_stable_sort.py: N = 8 at ring 2^12 (one batch) and N = 64
at ring 2^12 (P = 32, B = 2: the wrap crosses the batch boundary and both lanes
run); m = 2 keys at both, m = 3 at N = 8; mult_depth = lex_sort_depth(N, cfg,
m).  Inputs on the k/N grid, seeded as test_stable_sort.make_input:
  (g) primary with 4 groups (2 at N = 8) of equal values, secondary "every
      value twice": ties on both keys fall through to the index;
  (e) primary all equal;
  (f) both all equal: rank = index;
  (h) primary distinct: the rank ignores the secondary;
  (gd) (g) with the secondary descending;
  m = 3: two primaries with groups and a distinct third key.
The output gate is the reference's own (DirectSortTest: max error < 0.01).
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_stable_sort import GATE, make_input

SHAPES = [(8, 12, 1), (64, 12, 2)]  # N, log2 ring, batches B
KINDS = ["g", "e", "f", "h", "gd"]


def lex_input(N, kind):
    """(keys, descending) of a two-key case"""
    rng = np.random.default_rng(20251205 + N)
    groups = 2 if N == 8 else 4
    twice = make_input(N, "b")
    if kind in ("g", "gd"):
        return [rng.integers(0, groups, N) / N, twice], [False, kind == "gd"]
    if kind == "e":
        return [np.full(N, 0.5), twice], [False, False]
    if kind == "f":
        return [np.full(N, 0.5), np.full(N, 0.25)], [False, False]
    return [make_input(N, "a"), twice], [False, False]  # (h)


def lex_input3(N):
    rng = np.random.default_rng(20251205 + N)
    return [rng.integers(0, 2, N) / N, rng.integers(0, 2, N) / N, make_input(N, "a")], [False, True, False]


def lex_order(keys, desc):
    """row indices in (key_1, ..., key_m, index) order"""
    cols = [np.arange(len(keys[0]))] + [(-k if d else k) for k, d in reversed(list(zip(keys, desc)))]
    return np.lexsort(tuple(cols))


def lex_rank(keys, desc):
    return np.argsort(lex_order(keys, desc), kind="stable")


class Ctx:
    def __init__(self, backend, N, logn, m, short=0):
        self.N, self.m = N, m
        self.cfg = slotsim.default_sign_config(N)
        self.depth = sfhe.lex_sort_depth(N, self.cfg, m, backend) - short
        _, rots = sfhe.select_params(N, backend)
        self.e = sfhe.Engine(backend, mult_depth=self.depth, ring_dim=1 << logn, batch_size=N, rotations=rots,
                             seed=20251205 + N)
        self.e.set_quiet(True)
        self.s = self.e.sorter(N, rotations=rots)

    def enc(self, cols):
        return [self.e.encrypt(np.asarray(c, dtype=float).tolist()) for c in cols]

    def dec(self, ct):
        return np.array(self.e.decrypt(ct))[:self.N]


@pytest.fixture(scope="module")
def ctxs(oracle_lib):
    out = {(N, 2): Ctx("oracle", N, logn, 2) for N, logn, _ in SHAPES}
    out[8, 3] = Ctx("oracle", 8, 12, 3)
    yield out
    for c in out.values():
        c.e.close()


def test_depth_formula(oracle_lib):
    for N, _, _ in SHAPES:
        cfg = slotsim.default_sign_config(N)
        stable = sfhe.direct_sort_params(N, "oracle")[0] + 1
        assert [sfhe.lex_sort_depth(N, cfg, m, "oracle") for m in (1, 2, 3, 4)] == [stable + k for k in range(4)]
    with pytest.raises(sfhe.SfheError):
        sfhe.lex_sort_depth(8, (3, 2, 2), 5, "oracle")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_rank_lex(ctxs, N, logn, B, kind):
    c = ctxs[N, 2]
    keys, desc = lex_input(N, kind)
    cts = c.enc(keys)
    c.e.op_stats(reset=True)
    rank = c.s.rank_lex(cts, desc, *c.cfg)
    assert c.e.lex_counts() == (0, B)  # (m - 1) B steps, composed on the oracle
    got = c.dec(rank)
    want = lex_rank(keys, desc)
    err = float(np.max(np.abs(got - want)))
    print(f"N={N} ({kind}): lex rank err {err:.3g}, level {rank.level}")
    assert np.array_equal(np.rint(got), want), err
    assert rank.level == c.s.rank_stable(cts[0], *c.cfg).level + 1
    if kind == "f":
        assert np.array_equal(want, np.arange(N))
    if kind == "h":
        assert np.array_equal(want, lex_rank(keys[:1], desc[:1]))


def test_rank_lex_three_keys(ctxs):
    N = 8
    c = ctxs[N, 3]
    keys, desc = lex_input3(N)
    cts = c.enc(keys)
    c.e.op_stats(reset=True)
    rank = c.s.rank_lex(cts, desc, *c.cfg)
    assert c.e.lex_counts() == (0, 2)
    got = c.dec(rank)
    want = lex_rank(keys, desc)
    err = float(np.max(np.abs(got - want)))
    print(f"N={N} m=3: lex rank err {err:.3g}")
    assert np.array_equal(np.rint(got), want), err
    assert rank.level == c.s.rank_stable(cts[0], *c.cfg).level + 2
    # the three-key record sort ends at its depth
    ks, _ = c.s.sort_records_lex(cts, [], desc, *c.cfg)
    assert ks[0].level == c.depth == sfhe.lex_sort_depth(N, c.cfg, 3, "oracle")
    order = lex_order(keys, desc)
    for k, ct in zip(keys, ks):
        assert float(np.max(np.abs(c.dec(ct) - k[order]))) < GATE


@pytest.mark.parametrize("kind", ["g", "gd"])
@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_sort_and_select_records_lex(ctxs, N, logn, B, kind):
    c = ctxs[N, 2]
    keys, desc = lex_input(N, kind)
    rng = np.random.default_rng(7)
    cols = [rng.permutation(N) / N, 1.0 - 2.0 * rng.permutation(N) / N]
    order = lex_order(keys, desc)
    kcts, ccts = c.enc(keys), c.enc(cols)
    ks, outs = c.s.sort_records_lex(kcts, ccts, desc, *c.cfg)
    assert len(ks) == 2 and len(outs) == 2
    assert all(ct.level == c.depth for ct in ks + outs)
    worst = 0.0
    for src, ct in zip(keys + cols, ks + outs):
        worst = max(worst, float(np.max(np.abs(c.dec(ct) - src[order]))))
    print(f"N={N} ({kind}): sort_records_lex max err {worst:.3g}")
    assert worst < GATE, worst
    kcts, ccts = c.enc(keys), c.enc(cols)
    ks, outs = c.s.select_records_lex(kcts, ccts, range(4), desc, *c.cfg)
    worst = 0.0
    for src, ct in zip(keys + cols, ks + outs):
        worst = max(worst, float(np.max(np.abs(c.dec(ct)[:4] - src[order][:4]))))
    print(f"N={N} ({kind}): select_records_lex max err {worst:.3g}")
    assert worst < GATE, worst
    # top_k_records_lex is that call (the same ciphertexts in: the same residues out)
    ks2, outs2 = c.s.top_k_records_lex(kcts, ccts, 4, desc, **dict(zip(("n", "dg", "df"), c.cfg)))
    assert all(np.array_equal(a.download(), b.download()) for a, b in zip(ks + outs, ks2 + outs2))


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_one_ascending_key_is_rank_stable(ctxs, N, logn, B):
    c = ctxs[N, 2]
    ct = c.e.encrypt(make_input(N, "b").tolist())
    a, b = c.s.rank_lex([ct], None, *c.cfg), c.s.rank_stable(ct, *c.cfg)
    assert a.level == b.level
    assert np.array_equal(a.download(), b.download())
    # one descending key: the stable rank of the negated key
    x = make_input(N, "b")
    got = c.dec(c.s.rank_lex([ct], [True], *c.cfg))
    assert np.array_equal(np.rint(got), lex_rank([x], [True]))


def test_depth_one_short_is_an_error(oracle_lib):
    """A context one level short: SFHE_ESCHEME naming the depth, before anything is computed."""
    N, logn = 8, 12
    c = Ctx("oracle", N, logn, 2, short=1)
    keys, desc = lex_input(N, "g")
    cts = c.enc(keys)
    c.e.op_stats(reset=True)
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {c.depth + 1}\b"):
        c.s.sort_records_lex(cts, [], desc, *c.cfg)
    stats = c.e.op_stats()
    assert c.e.lex_counts() == (0, 0) and c.e.tie_counts() == (0, 0), stats
    # the rank alone fits this context; one more level short and it does not
    rank_depth = c.s.rank_lex(cts, desc, *c.cfg).level
    short = sfhe.Engine("oracle", mult_depth=rank_depth - 1, ring_dim=1 << logn, batch_size=N,
                        rotations=sfhe.direct_sort_params(N, "oracle")[1], seed=1)
    ss = short.sorter(N)
    scts = [short.encrypt(k.tolist()) for k in keys]
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {rank_depth}\b"):
        ss.rank_lex(scts, desc, *c.cfg)
    short.close()
    c.e.close()


def test_bad_arguments(ctxs):
    N = 8
    c = ctxs[N, 2]
    keys, desc = lex_input(N, "g")
    cts = c.enc(keys)
    low = c.e.mult_const(cts[1], 1.0)  # one level down
    assert low.level == cts[0].level + 1
    with pytest.raises(sfhe.SfheError, match="sfhe error -2: .*one level"):
        c.s.rank_lex([cts[0], low], desc, *c.cfg)
    five = c.enc([keys[0]] * 5)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*key count"):
        c.s.rank_lex(five, None, *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*key count"):
        c.s.rank_lex([], None, *c.cfg)
    with pytest.raises(sfhe.SfheError, match="descending flag"):
        c.s.rank_lex(cts, [True], *c.cfg)
    many = c.enc([keys[0]] * sfhe.MAX_COLUMNS)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*too many columns"):
        c.s.sort_records_lex(cts, many, desc, *c.cfg)


def test_lex_step_values(ctxs):
    """lex_step(v, q, u) = v + (1 - q) u, with v and q above u's level as the rank uses it."""
    N = 8
    c = ctxs[N, 2]
    rng = np.random.default_rng(11)
    v, q, u = (rng.uniform(-1, 1, N) for _ in range(3))
    cv, cq, cu = c.enc([v, q, u])
    cu2 = c.e.mult_const(c.e.mult_const(cu, 1.0), 1.0)
    cv1 = c.e.mult_const(cv, 1.0)
    c.e.op_stats(reset=True)
    for a, b, w in ((cv, cq, cu), (cv1, cq, cu2), (cv1, cv1, cu2)):
        out = c.e.lex_step(a, b, w)
        assert out.level == w.level + 1
        want = v + (1 - (v if b is cv1 else q)) * u
        err = float(np.max(np.abs(c.dec(out) - want)))
        assert err < 1e-6, err
    assert c.e.lex_counts() == (0, 3)
    with pytest.raises(sfhe.SfheError, match="sfhe error -2: .*limbs"):
        c.e.lex_step(cu2, cq, cu)


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_one_key_sort_leaves_the_secondary_unordered(ctxs, N, logn, B):
    """The gap this feature closes: sort_records by the primary alone keeps equal primaries in
    input order, so the secondary column comes out of lexicographic order: the secondary's
    values span half the unit interval inside each group, far more than 5 x the gate."""
    c = ctxs[N, 2]
    keys, desc = lex_input(N, "g")
    kcts = c.enc(keys)
    _, outs = c.s.sort_records(kcts[0], [kcts[1]], True, *c.cfg)
    want = keys[1][lex_order(keys, desc)]
    err = float(np.max(np.abs(c.dec(outs[0]) - want)))
    print(f"N={N}: one-key record sort, secondary column off by {err:.3g}")
    assert err > 5 * GATE, err


def test_abi_lists_the_lex_entry_points(oracle_lib):
    for name in ("sfhe_lex_sort_depth", "sfhe_sorter_rank_lex", "sfhe_sorter_sort_records_lex",
                 "sfhe_sorter_select_records_lex", "sfhe_eval_lex_step", "sfhe_lex_counts"):
        assert hasattr(oracle_lib, name), name
