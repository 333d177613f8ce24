"""Grouping rows by an encrypted key (DirectSort<N>::groupAggregate) on the C
oracle: for every row r, in input order,

    count_r = #{j : k_j = k_r},   index_r = #{j < r : k_j = k_r},   sum_cr = sum of col_c over that set.

Shapes as tests/test_stable_sort.py: N = 8 at ring 2^12 (one batch) and N = 64 at ring 2^12
(P = 32, B = 2: the wrap r + d >= N crosses the batch boundary and both lanes run);
mult_depth = group_params(N).  Keys on the k/N grid (equal, or at least the sign's resolution
1/N apart):
  (a) distinct;  (b) every value twice;  (g) 4 groups of uneven sizes (2 at N = 8);  (d) all equal.
Payload columns perm / N, 1 - 2 perm / N and perm / N - 1/2, seeded.
The gate is the reference's own (DirectSortTest: max error < 0.01); rint of count and index
must equal numpy exactly.
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_stable_sort import GATE, make_input

SHAPES = [(8, 12, 1), (64, 12, 2)]  # N, log2 ring, batches B
KINDS = ["a", "b", "g", "d"]
GROUP_SIZES = {8: [5, 3], 64: [29, 17, 11, 7]}


def group_keys(N, kind):
    if kind == "g":
        rng = np.random.default_rng(20251205 + N)
        ids = np.repeat(np.arange(len(GROUP_SIZES[N])), GROUP_SIZES[N])
        return rng.permutation(ids) / N
    return make_input(N, kind)


def payload(N, count=3):
    rng = np.random.default_rng(7)
    cols = [rng.permutation(N) / N, 1.0 - 2.0 * rng.permutation(N) / N, rng.permutation(N) / N - 0.5]
    return cols[:count]


def expected(keys, cols):
    """(count, index, [sums]) from numpy"""
    eq = keys[:, None] == keys[None, :]  # eq[r, j]
    before = np.tril(np.ones_like(eq), -1)  # j < r
    return eq.sum(1), (eq & before).sum(1), [eq.astype(float) @ c for c in cols]


class Ctx:
    def __init__(self, backend, N, logn, short=0):
        self.N = N
        self.cfg = slotsim.default_sign_config(N)
        self.depth, self.rots = sfhe.group_params(N, backend)
        self.depth -= short
        self.e = sfhe.Engine(backend, mult_depth=self.depth, ring_dim=1 << logn, batch_size=N, rotations=self.rots,
                             seed=20251205 + N)
        self.e.set_quiet(True)
        self.s = self.e.sorter(N, rotations=self.rots)

    def enc(self, cols):
        return [self.e.encrypt(np.asarray(c, dtype=float).tolist()) for c in cols]

    def dec(self, ct):
        return np.array(self.e.decrypt(ct))[:self.N]


def check_group(c, got, keys, cols, what):
    """the gate on every output, rint of count and index exact; returns the maxima"""
    count, index, sums = expected(keys, cols)
    errs = {"count": float(np.max(np.abs(c.dec(got["count"]) - count)))}
    assert np.array_equal(np.rint(c.dec(got["count"])), count), (what, errs)
    if got["index"] is not None:
        errs["index"] = float(np.max(np.abs(c.dec(got["index"]) - index)))
        assert np.array_equal(np.rint(c.dec(got["index"])), index), (what, errs)
    assert len(got["sums"]) == len(cols)
    errs["sums"] = max([float(np.max(np.abs(c.dec(ct) - s))) for ct, s in zip(got["sums"], sums)], default=0.0)
    print(f"{what}: " + ", ".join(f"{k} err {v:.3g}" for k, v in errs.items()))
    assert all(v < GATE for v in errs.values()), (what, errs)
    return errs


@pytest.fixture(scope="module")
def ctxs(oracle_lib):
    out = {N: Ctx("oracle", N, logn) for N, logn, _ in SHAPES}
    yield out
    for c in out.values():
        c.e.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_group(ctxs, N, logn, B, kind):
    c = ctxs[N]
    keys, cols = group_keys(N, kind), payload(N, 2)
    kct, ccts = c.enc([keys])[0], c.enc(cols)
    c.e.op_stats(reset=True)
    got = c.s.group(kct, ccts, True, *c.cfg)
    assert c.e.group_counts() == (0, 1)  # one gated sum, composed on the oracle
    check_group(c, got, keys, cols, f"N={N} ({kind})")
    # the count sits at the gates' level, the gated sums and the index one below: the context's depth
    assert got["count"].level == c.depth - 1
    assert got["index"].level == c.depth and all(s.level == c.depth for s in got["sums"])
    want = expected(keys, cols)
    if kind == "a":  # distinct keys: every row is its own group
        assert np.array_equal(want[0], np.ones(N)) and np.array_equal(want[1], np.zeros(N))
        assert all(np.array_equal(s, col) for s, col in zip(want[2], cols))
    if kind == "d":
        assert np.array_equal(want[0], np.full(N, N)) and np.array_equal(want[1], np.arange(N))
    if kind == "g":
        assert sorted(set(want[0])) == sorted(GROUP_SIZES[N])


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_depth_is_the_rank_s_not_the_sort_s(ctxs, N, logn, B):
    """group_params' depth is below direct_sort_params'; an engine built there groups (test_group)
    and refuses to sort."""
    c = ctxs[N]
    sort_depth = sfhe.direct_sort_params(N, "oracle")[0]
    assert c.depth < sort_depth
    ct = c.enc([make_input(N, "a")])[0]
    assert c.s.rank_stable(ct, *c.cfg).level == c.depth  # the stable rank's depth
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {sort_depth + 1}\b"):
        c.s.sort_stable(ct, *c.cfg)
    if N == 8:  # the plain sort runs out of levels on the way (an engine of its own: it fails midway)
        d = Ctx("oracle", N, logn)
        x = make_input(N, "a")
        with pytest.raises(sfhe.SfheError):
            d.s.sort(d.enc([x])[0], *d.cfg)
        d.e.close()


def test_depth_one_short_is_an_error(oracle_lib):
    """One level short: SFHE_ESCHEME naming the depth needed, before anything is computed."""
    N, logn = 8, 12
    c = Ctx("oracle", N, logn, short=1)
    kct = c.enc([group_keys(N, "g")])[0]
    ccts = c.enc(payload(N, 1))
    c.e.op_stats(reset=True)
    before = c.e.op_stats()
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {c.depth + 1}\b"):
        c.s.group(kct, ccts, True, *c.cfg)
    assert c.e.op_stats() == before
    assert c.e.group_counts() == (0, 0)
    c.e.close()


def test_no_columns_and_no_index(ctxs):
    N = 8
    c = ctxs[N]
    keys = group_keys(N, "g")
    kct = c.enc([keys])[0]
    c.e.op_stats(reset=True)
    got = c.s.group(kct, (), False, *c.cfg)
    assert c.e.group_counts() == (0, 0)  # no gated sum without columns
    assert got["index"] is None and got["sums"] == []
    check_group(c, got, keys, [], "N=8 (g), count alone")
    got = c.s.group(kct, c.enc(payload(N, 1)), False, *c.cfg)
    assert got["index"] is None and len(got["sums"]) == 1
    check_group(c, got, keys, payload(N, 1), "N=8 (g), one column, no index")


def test_gate_sum_many_values(ctxs):
    """gate_sum_many on B = 2, C = 1: sum_b (1 - q_b) u_b, with u above the gates' level."""
    N = 8
    c = ctxs[N]
    rng = np.random.default_rng(11)
    q = [rng.uniform(0, 1, N) for _ in range(2)]
    u = [rng.uniform(-1, 1, N) for _ in range(2)]
    qct = [c.e.mult_const(x, 1.0) for x in c.enc(q)]  # one level down
    uct = c.enc(u)  # level 0: more limbs than the gates
    c.e.op_stats(reset=True)
    out = c.e.gate_sum_many(qct, [uct])
    assert c.e.group_counts() == (0, 1)
    assert len(out) == 1 and out[0].level == qct[0].level + 1
    want = sum((1 - a) * b for a, b in zip(q, u))
    err = float(np.max(np.abs(c.dec(out[0]) - want)))
    print(f"gate_sum_many B=2 C=1: err {err:.3g}")
    assert err < 1e-6, err
    assert c.e.gate_sum_many(qct, []) == []


def test_gate_sum_many_one_batch_is_lex_step(ctxs):
    """B = 1, C = 1 has the residues of lex_step with an all-zero v: u - u is a ciphertext of
    all-zero residues at u's scale, built from the public ops, and its lifted rows add nothing
    to the tensor."""
    N = 8
    c = ctxs[N]
    rng = np.random.default_rng(12)
    q, u = rng.uniform(0, 1, N), rng.uniform(-1, 1, N)
    qct, uct = c.enc([q, u])
    zero = c.e.sub(uct, uct)
    assert not zero.download().any()
    a = c.e.gate_sum_many([qct], [[uct]])[0]
    b = c.e.lex_step(zero, qct, uct)
    assert a.level == b.level
    assert np.array_equal(a.download(), b.download())
    assert float(np.max(np.abs(c.dec(a) - (1 - q) * u))) < 1e-6


def test_bad_arguments(ctxs):
    N = 8
    c = ctxs[N]
    keys = group_keys(N, "g")
    kct = c.enc([keys])[0]
    col = c.enc(payload(N, 1))[0]
    low = c.e.mult_const(col, 1.0)
    assert low.level == kct.level + 1
    # gates at different levels; an operand with fewer limbs than the gates
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one level"):
        c.e.gate_sum_many([kct, low], [[col, col]])
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*limbs"):
        c.e.gate_sum_many([kct], [[low]])
    nine = [[col]] * (sfhe.MAX_COLUMNS + 1)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*column count"):
        c.e.gate_sum_many([kct], nine)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one operand per gate"):
        c.e.gate_sum_many([kct, kct], [[col]])
    c.e.op_stats(reset=True)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*column count"):
        c.s.group(kct, [col] * (sfhe.MAX_COLUMNS + 1), False, *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one level"):
        c.s.group(kct, [low], False, *c.cfg)
    assert c.e.group_counts() == (0, 0)


def test_abi_lists_the_group_entry_points(oracle_lib):
    for name in ("sfhe_group_params", "sfhe_sorter_group", "sfhe_eval_gate_sum_many", "sfhe_group_counts"):
        assert hasattr(oracle_lib, name), name
    assert "sfhe_sorter_group" in sfhe.ABI_SYMBOLS
