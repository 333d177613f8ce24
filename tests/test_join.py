"""Join of two encrypted tables on up to four keys (DirectSort<N>::joinAggregate)
on the C oracle: for every row r of table A, in A's input order,

    count_r = #{j : keyB_kj = keyA_kr for every k},   sum_cr = sum of colsB[c]_j over that set.

Shapes as tests/test_group.py: N = 8 at ring 2^12 (one batch) and N = 64 at ring 2^12 (P = 32,
B = 2: the wrap r + d >= N crosses the batch boundary and both lanes run); mult_depth =
join_params(N, m).  Keys on the k/N grid (equal, or at least the sign's resolution 1/N apart),
payloads from test_group.payload.  One key:
  (fk) B distinct, A drawn from B's values with repeats: count all ones, sums the looked-up value;
  (h)  B holds N/2 values twice, A all N grid values: counts 2 and 0;
  (n)  disjoint value sets: counts and sums all zero;
  (d)  everything equal: count N, sums the column totals.
Several keys: small value sets, so that rows agree on one key and differ on another.
Every output is compared against numpy's eq = all_k(keyA_k[:, None] == keyB_k[None, :]); the gate
is the reference's own (DirectSortTest: max error < 0.01) and rint(count) must equal numpy exactly.
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_group import SHAPES, payload
from test_stable_sort import GATE, make_input

KINDS = ["fk", "h", "n", "d"]


def layers(m):
    return (m - 1).bit_length()  # ceil(log2 m)


def join_keys(N, kind):
    """([keysA], [keysB]) of the one-key cases"""
    rng = np.random.default_rng(20251205 + N)
    if kind == "fk":
        b = make_input(N, "a")
        return [rng.choice(b, N)], [b]
    if kind == "h":
        return [make_input(N, "a")], [make_input(N, "b")]
    if kind == "n":
        return [2 * rng.integers(0, N // 2, N) / N], [(2 * rng.integers(0, N // 2, N) + 1) / N]
    return [np.full(N, 0.5)], [np.full(N, 0.5)]


def multi_keys(N, m, seed=0):
    """m keys per table from a few grid values each, so that every pattern of agreeing and
    differing keys occurs"""
    rng = np.random.default_rng(20251205 + N + 100 * m + seed)
    vals = 4 if m == 2 else 2
    return ([rng.integers(0, vals, N) / N for _ in range(m)], [rng.integers(0, vals, N) / N for _ in range(m)])


def expected(ka, kb, cols):
    """(count, [sums]) from numpy"""
    eq = np.ones((len(ka[0]), len(kb[0])), dtype=bool)  # eq[r, j]
    for a, b in zip(ka, kb):
        eq &= a[:, None] == b[None, :]
    return eq.sum(1), [eq.astype(float) @ c for c in cols]


class Ctx:
    def __init__(self, backend, N, logn, m=1, short=0):
        self.N, self.m = N, m
        self.cfg = slotsim.default_sign_config(N)
        self.depth, self.rots = sfhe.join_params(N, m, backend)
        self.depth -= short
        self.e = sfhe.Engine(backend, mult_depth=self.depth, ring_dim=1 << logn, batch_size=N, rotations=self.rots,
                             seed=20251205 + N)
        self.e.set_quiet(True)
        self.s = self.e.sorter(N, rotations=self.rots)

    def enc(self, cols):
        return [self.e.encrypt(np.asarray(c, dtype=float).tolist()) for c in cols]

    def dec(self, ct):
        return np.array(self.e.decrypt(ct))[:self.N]


def check_join(c, got, ka, kb, cols, what):
    """the gate on every output, rint of the count exact; returns the maxima"""
    count, sums = expected(ka, kb, cols)
    errs = {"count": float(np.max(np.abs(c.dec(got["count"]) - count)))}
    assert np.array_equal(np.rint(c.dec(got["count"])), count), (what, errs)
    assert len(got["sums"]) == len(cols)
    errs["sums"] = max([float(np.max(np.abs(c.dec(ct) - s))) for ct, s in zip(got["sums"], sums)], default=0.0)
    print(f"{what}: " + ", ".join(f"{k} err {v:.3g}" for k, v in errs.items()))
    assert all(v < GATE for v in errs.values()), (what, errs)
    return errs


@pytest.fixture(scope="module")
def ctxs(oracle_lib):
    """One context per (N, depth), made when first asked for: m = 3 and m = 4 share one."""
    made = {}

    def get(N, m):
        logn = {n: l for n, l, _ in SHAPES}[N]
        key = (N, layers(m))
        if key not in made:
            made[key] = Ctx("oracle", N, logn, m)
        return made[key]

    yield get
    for c in made.values():
        c.e.close()


def run(c, ka, kb, cols, m, B):
    """the join with its level and counter checks"""
    act, bct, ccts = c.enc(ka), c.enc(kb), c.enc(cols)
    c.e.op_stats(reset=True)
    got = c.s.join(act, bct, ccts, *c.cfg)
    depth = sfhe.join_params(c.N, m, "oracle")[0]
    assert depth == c.depth
    assert c.e.join_counts() == (0, B * (m - 1))  # composed on the oracle, one per tree node and batch
    assert c.e.group_counts() == (0, 1 if cols else 0)
    assert got["count"].level == depth - 1 and all(s.level == depth for s in got["sums"])
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_join_one_key(ctxs, N, logn, B, kind):
    c = ctxs(N, 1)
    (ka, kb), cols = join_keys(N, kind), payload(N, 2)
    got = run(c, ka, kb, cols, 1, B)
    check_join(c, got, ka, kb, cols, f"N={N} m=1 ({kind})")
    count, sums = expected(ka, kb, cols)
    if kind == "fk":  # a foreign-key lookup: one match each, the sum is the looked-up value
        look = {k: i for i, k in enumerate(kb[0])}
        assert np.array_equal(count, np.ones(N)) and len(set(ka[0])) < N
        assert all(np.array_equal(s, col[[look[k] for k in ka[0]]]) for s, col in zip(sums, cols))
    if kind == "h":  # half of A's rows are unmatched
        assert sorted(count) == [0] * (N // 2) + [2] * (N // 2)
    if kind == "n":
        assert not count.any() and not any(s.any() for s in sums)
    if kind == "d":
        assert np.array_equal(count, np.full(N, N))
        assert all(np.allclose(s, col.sum()) for s, col in zip(sums, cols))


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_join_two_keys(ctxs, N, logn, B):
    """A != B, with pairs that agree on key 1 and differ on key 2, and the reverse."""
    c = ctxs(N, 2)
    (ka, kb), cols = multi_keys(N, 2), payload(N, 2)
    e1, e2 = (a[:, None] == b[None, :] for a, b in zip(ka, kb))
    assert (e1 & ~e2).any() and (~e1 & e2).any() and (e1 & e2).any() and (~e1 & ~e2).any()
    got = run(c, ka, kb, cols, 2, B)
    check_join(c, got, ka, kb, cols, f"N={N} m=2 (cross)")


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_self_join_two_keys_is_group_by_pair(ctxs, N, logn, B):
    c = ctxs(N, 2)
    (ka, _), cols = multi_keys(N, 2, seed=1), payload(N, 2)
    got = run(c, ka, ka, cols, 2, B)
    check_join(c, got, ka, ka, cols, f"N={N} m=2 (self)")
    pairs = list(zip(*ka))
    want = np.array([pairs.count(p) for p in pairs])  # numpy's group-by-pair
    assert 1 < len(set(pairs)) < N and np.array_equal(np.rint(c.dec(got["count"])), want)


@pytest.mark.parametrize("m", [3, 4])
def test_join_three_and_four_keys(ctxs, m):
    """The uneven tree (q1 v q2) v q3, its operands at two levels, and the full one."""
    N, B = 8, 1
    c = ctxs(N, m)
    (ka, kb), cols = multi_keys(N, m), payload(N, 1)
    count, _ = expected(ka, kb, cols)
    assert count.any() and not count.all()
    got = run(c, ka, kb, cols, m, B)
    check_join(c, got, ka, kb, cols, f"N={N} m={m}")


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_self_join_on_one_key_has_group_s_residues(ctxs, N, logn, B):
    """join([k], [k], cols) runs groupAggregate's op sequence: equal residues on one engine."""
    c = ctxs(N, 1)
    keys, cols = make_input(N, "b"), payload(N, 2)
    kct, ccts = c.enc([keys])[0], c.enc(cols)
    j = c.s.join([kct], [kct], ccts, *c.cfg)
    g = c.s.group(kct, ccts, False, *c.cfg)
    for name, a, b in [("count", j["count"], g["count"])] + [(f"sum{i}", a, b) for i, (a, b) in
                                                              enumerate(zip(j["sums"], g["sums"]))]:
        assert a.level == b.level, name
        assert np.array_equal(a.download(), b.download()), name
    check_join(c, j, [keys], [keys], cols, f"N={N} m=1 (self)")


def test_depths():
    for N, _, _ in SHAPES:
        d, rots = sfhe.group_params(N, "oracle")
        assert sfhe.join_params(N, 1, "oracle") == (d, rots)
        for m in (2, 3, 4):
            assert sfhe.join_params(N, m, "oracle") == (d + layers(m), rots)
    assert [layers(m) for m in (1, 2, 3, 4)] == [0, 1, 2, 2]
    for m in (0, 5):
        with pytest.raises(sfhe.SfheError):
            sfhe.join_params(8, m, "oracle")


def test_depth_one_short_is_an_error(oracle_lib):
    """One level short: SFHE_ESCHEME naming the depth needed, before anything is computed."""
    N, logn, m = 8, 12, 2
    c = Ctx("oracle", N, logn, m, short=1)
    ka, kb = multi_keys(N, m)
    act, bct, ccts = c.enc(ka), c.enc(kb), c.enc(payload(N, 1))
    c.e.op_stats(reset=True)
    before = c.e.op_stats()
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {c.depth + 1}\b"):
        c.s.join(act, bct, ccts, *c.cfg)
    assert c.e.op_stats() == before
    assert c.e.join_counts() == (0, 0) and c.e.group_counts() == (0, 0)
    c.e.close()


def test_bad_arguments(ctxs):
    N = 8
    c = ctxs(N, 4)
    ka, kb = multi_keys(N, 4)
    act, bct = c.enc(ka), c.enc(kb)
    col = c.enc(payload(N, 1))[0]
    low = c.e.mult_const(col, 1.0)
    assert low.level == col.level + 1
    c.e.op_stats(reset=True)
    before = c.e.op_stats()
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*key count"):
        c.s.join([], [], [col], *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*key count"):
        c.s.join(act + act[:1], bct + bct[:1], [col], *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*column count"):
        c.s.join(act[:1], bct[:1], [col] * (sfhe.MAX_COLUMNS + 1), *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*2 keys of table A against 1"):
        c.s.join(act[:2], bct[:1], [col], *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one level"):
        c.s.join(act[:1], bct[:1], [low], *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one level"):
        c.s.join(act[:2], [bct[0], low], [col], *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*null"):
        c.s.join([None], bct[:1], [col], *c.cfg)
    assert c.e.op_stats() == before
    assert c.e.join_counts() == (0, 0) and c.e.group_counts() == (0, 0)


def test_gate_or_values(ctxs):
    """gate_or alone on chosen values in [0, 1], the 0/1 corners included, with the operands at
    one level and at two: a + b - ab one level below the lower operand."""
    N = 8
    c = ctxs(N, 1)
    a = np.array([0.0, 0.0, 1.0, 1.0, 0.25, 0.5, 1.0, 0.0])
    b = np.array([0.0, 1.0, 0.0, 1.0, 0.75, 0.5, 0.3, 0.6])
    want = a + b - a * b
    assert np.array_equal(want[:4], [0, 1, 1, 1])
    act, bct = c.enc([a, b])
    low = c.e.mult_const(bct, 1.0)  # one level down: fewer limbs than a
    lower = c.e.mult_const(low, 1.0)
    c.e.op_stats(reset=True)
    for x, y, what in [(act, bct, "one level"), (act, low, "a above b"), (low, act, "b above a"),
                       (act, lower, "two levels apart")]:
        out = c.e.gate_or(x, y)
        assert out.level == max(x.level, y.level) + 1, what
        err = float(np.max(np.abs(c.dec(out) - want)))
        print(f"gate_or ({what}): err {err:.3g}")
        assert err < 1e-6, (what, err)
    assert c.e.join_counts() == (0, 4)
    wide = c.e.encrypt(a.tolist(), slots=2 * N)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*slot count"):
        c.e.gate_or(act, wide)
    assert c.e.join_counts() == (0, 4)


def test_no_columns(ctxs):
    N = 8
    c = ctxs(N, 2)
    ka, kb = multi_keys(N, 2)
    got = run(c, ka, kb, [], 2, 1)  # (group_counts stays (0, 0): no gated sum without columns)
    assert got["sums"] == []
    check_join(c, got, ka, kb, [], "N=8 m=2, count alone")


def test_abi_lists_the_join_entry_points(oracle_lib):
    for name in ("sfhe_join_params", "sfhe_sorter_join", "sfhe_eval_gate_or", "sfhe_join_counts"):
        assert hasattr(oracle_lib, name), name
        assert name in sfhe.ABI_SYMBOLS
