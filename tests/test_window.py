"""Aggregates over an ordered frame (DirectSort<N>::windowSums) on the C oracle:
for every row r, in input order, the count and the column sums over row r's frame,

    rows:   {j : (k_j, j) <= (k_r, r)}     range:  {j : k_j <= k_r}     below:  {j : k_j < k_r}.

Shapes, keys and payload columns as tests/test_group.py: N = 8 at ring 2^12 (one batch) and
N = 64 at ring 2^12 (P = 32, B = 2: the wrap r + d >= N crosses the batch boundary and both lanes
run); mult_depth = window_params(N).  Keys (a) distinct, (b) every value twice, (g) uneven groups,
(d) all equal.  The gate is the reference's own (DirectSortTest: max error < 0.01); rint of the
count must equal numpy exactly.
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_group import GATE, SHAPES, KINDS, Ctx, expected as group_expected, group_keys, make_input, payload

FRAMES = {8: ["rows", "range", "below"], 64: ["rows", "range"]}
CASES = [(N, logn, B, frame) for N, logn, B in SHAPES for frame in FRAMES[N]]


def frame_sets(keys, frame):
    """member[r, j]: row j is in row r's frame"""
    k = np.asarray(keys)
    idx = np.arange(len(k))
    less, eq = k[None, :] < k[:, None], k[None, :] == k[:, None]
    if frame == "rows":
        return less | (eq & (idx[None, :] <= idx[:, None]))
    if frame == "range":
        return less | eq
    return less


def expected(keys, cols, frame):
    """(count, [sums]) from numpy"""
    member = frame_sets(keys, frame)
    return member.sum(1), [member.astype(float) @ c for c in cols]


class WCtx(Ctx):
    """test_group's context at window_params' depth"""

    def __init__(self, backend, N, logn, short=0):
        self.N = N
        self.cfg = slotsim.default_sign_config(N)
        self.depth, self.rots = sfhe.window_params(N, backend)
        self.depth -= short
        self.e = sfhe.Engine(backend, mult_depth=self.depth, ring_dim=1 << logn, batch_size=N, rotations=self.rots,
                             seed=20251205 + N)
        self.e.set_quiet(True)
        self.s = self.e.sorter(N, rotations=self.rots)


def check_window(c, got, keys, cols, frame, what):
    """the gate on every output, rint of the count exact; returns the maxima"""
    count, sums = expected(keys, cols, frame)
    errs = {}
    if got["count"] is not None:
        errs["count"] = float(np.max(np.abs(c.dec(got["count"]) - count)))
    assert len(got["sums"]) == len(cols)
    errs["sums"] = max([float(np.max(np.abs(c.dec(ct) - s))) for ct, s in zip(got["sums"], sums)], default=0.0)
    print(f"{what}: " + ", ".join(f"{k} err {v:.3g}" for k, v in errs.items()))
    if got["count"] is not None:
        assert np.array_equal(np.rint(c.dec(got["count"])), count), (what, errs)
    assert all(v < GATE for v in errs.values()), (what, errs)
    return errs


@pytest.fixture(scope="module")
def ctxs(oracle_lib):
    out = {N: WCtx("oracle", N, logn) for N, logn, _ in SHAPES}
    yield out
    for c in out.values():
        c.e.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn,B,frame", CASES)
def test_window(ctxs, N, logn, B, frame, kind):
    c = ctxs[N]
    keys, cols = group_keys(N, kind), payload(N, 2)
    kct, ccts = c.enc([keys])[0], c.enc(cols)
    c.e.op_stats(reset=True)
    got = c.s.window(kct, ccts, frame, True, *c.cfg)
    assert c.e.window_counts() == (0, 1)  # one weighted sum, composed on the oracle
    check_window(c, got, keys, cols, frame, f"N={N} {frame} ({kind})")
    # the count sits at the gates' level, the weighted sums one below: the context's depth
    assert got["count"].level == c.depth - 1
    assert all(s.level == c.depth for s in got["sums"])
    # the expectations themselves: the inputs exercise ties
    count, sums = expected(keys, cols, frame)
    if kind == "d" and frame == "rows":  # all equal: prefix sums in input order
        assert np.array_equal(count, np.arange(N) + 1)
        assert all(np.allclose(s, np.cumsum(col), atol=1e-12) for s, col in zip(sums, cols))
    if kind == "a" and frame == "range":  # distinct keys: no peers
        rows = expected(keys, cols, "rows")
        assert np.array_equal(count, rows[0]) and all(np.array_equal(s, t) for s, t in zip(sums, rows[1]))
    if kind != "a" and frame == "range":
        assert not np.array_equal(count, expected(keys, cols, "rows")[0])
    if frame == "range":  # range - below = the key's group
        below = expected(keys, cols, "below")
        gcount, _, gsums = group_expected(keys, cols)
        assert np.array_equal(count - below[0], gcount)
        assert all(np.allclose(s - t, g, atol=1e-12) for s, t, g in zip(sums, below[1], gsums))


@pytest.mark.parametrize("N,logn,B", SHAPES)
@pytest.mark.parametrize("kind", ["b", "g"])
def test_row_number_is_the_stable_rank_plus_one(ctxs, N, logn, B, kind):
    c = ctxs[N]
    kct = c.enc([group_keys(N, kind)])[0]
    c.e.op_stats(reset=True)
    got = c.s.window(kct, (), "rows", True, *c.cfg)
    assert c.e.window_counts() == (0, 0)  # no weighted sum without columns
    assert got["sums"] == []
    rank = c.s.rank_stable(kct, *c.cfg)
    err = float(np.max(np.abs(c.dec(got["count"]) - 1.0 - c.dec(rank))))
    print(f"N={N} ({kind}): count - 1 against rank_stable: {err:.3g}")
    assert err < GATE, err


def test_no_count(ctxs):
    N = 8
    c = ctxs[N]
    keys, cols = group_keys(N, "g"), payload(N, 1)
    got = c.s.window(c.enc([keys])[0], c.enc(cols), "range", False, *c.cfg)
    assert got["count"] is None and len(got["sums"]) == 1
    check_window(c, got, keys, cols, "range", "N=8 range (g), one column, no count")


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_params(oracle_lib, N, logn, B):
    depth, rots = sfhe.window_params(N, "oracle")
    gdepth, grots = sfhe.group_params(N, "oracle")
    assert depth == gdepth + 1 and rots == grots


def test_depth_one_short_is_an_error(oracle_lib):
    """One level short: SFHE_ESCHEME naming the depth needed, before anything is computed."""
    N, logn = 8, 12
    c = WCtx("oracle", N, logn, short=1)
    kct = c.enc([group_keys(N, "g")])[0]
    ccts = c.enc(payload(N, 1))
    c.e.op_stats(reset=True)
    before = c.e.op_stats()
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {c.depth + 1}\b"):
        c.s.window(kct, ccts, "rows", True, *c.cfg)
    assert c.e.op_stats() == before
    assert c.e.window_counts() == (0, 0)
    c.e.close()


def test_weight_sum_many_values(ctxs):
    """weight_sum_many on B = 2, C = 1: sum_b (p_b + v_b) u_b, with u above the gates' level."""
    N = 8
    c = ctxs[N]
    rng = np.random.default_rng(11)
    v = [rng.uniform(-0.5, 0.5, N) for _ in range(2)]
    p = [rng.integers(0, 2, N).astype(float) for _ in range(2)]
    u = [rng.uniform(-1, 1, N) for _ in range(2)]
    vct = [c.e.mult_const(x, 1.0) for x in c.enc(v)]  # one level down
    uct = c.enc(u)  # level 0: more limbs than the gates
    c.e.op_stats(reset=True)
    out = c.e.weight_sum_many(vct, p, [uct])
    assert c.e.window_counts() == (0, 1)
    assert len(out) == 1 and out[0].level == vct[0].level + 1
    want = sum((w + a) * b for w, a, b in zip(p, v, u))
    err = float(np.max(np.abs(c.dec(out[0]) - want)))
    print(f"weight_sum_many B=2 C=1: err {err:.3g}")
    assert err < 1e-6, err
    assert c.e.weight_sum_many(vct, p, []) == []


def test_bad_arguments(ctxs):
    N = 8
    c = ctxs[N]
    kct = c.enc([group_keys(N, "g")])[0]
    col = c.enc(payload(N, 1))[0]
    low = c.e.mult_const(col, 1.0)
    w = [0.5] * N
    assert low.level == kct.level + 1
    c.e.op_stats(reset=True)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*frame"):
        c.s.window(kct, [col], "groups", False, *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*frame"):  # past the binding's names
        c.e._chk(c.e.lib.sfhe_sorter_window(c.s.h, kct.h, None, 0, 3, 0, *c.cfg, None, None))
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*column count"):
        c.s.window(kct, [col] * (sfhe.MAX_COLUMNS + 1), "rows", False, *c.cfg)
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one level"):
        c.s.window(kct, [low], "rows", False, *c.cfg)
    # gates at different levels; a column with the wrong operand count; a weight count != nv
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one level"):
        c.e.weight_sum_many([kct, low], [w, w], [[col, col]])
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one operand per gate"):
        c.e.weight_sum_many([kct, kct], [w, w], [[col]])
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*one weight vector per gate"):
        c.e.weight_sum_many([kct, kct], [w], [[col, col]])
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*limbs"):
        c.e.weight_sum_many([low], [w], [[c.e.mult_const(low, 1.0)]])
    with pytest.raises(sfhe.SfheError, match="sfhe error -1: .*column count"):
        c.e.weight_sum_many([kct], [w], [[col]] * (sfhe.MAX_COLUMNS + 1))
    assert c.e.window_counts() == (0, 0)


def test_abi_lists_the_window_entry_points(oracle_lib):
    for name in ("sfhe_window_params", "sfhe_sorter_window", "sfhe_eval_weight_sum_many", "sfhe_window_counts"):
        assert hasattr(oracle_lib, name), name
    assert "sfhe_sorter_window" in sfhe.ABI_SYMBOLS
