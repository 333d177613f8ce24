"""The tie-aware stable rank sort (DirectSort<N>::sortStable /
constructRankStable) on the C oracle.

The plain rank sort is only correct on distinct inputs: a comparison of equal
values gives 1/2, two equal elements share the rank L + 1/2 and the placement
writes 0.64 x + 0.64 x into two slots.  The stable rank is
#{j : x_j < x_r} + #{j < r : x_j = x_r}, i.e. argsort(argsort(x, "stable")).

Shapes: the smallest that reach each path -- N = 8 at ring 2^12 (one batch,
P = 8, CompositeSign(3, 2, 2)) and N = 64 at ring 2^12 (P = 32, B = 2,
CompositeSign(3, 3, 2)): the wrap condition r + b P + p >= N crosses the batch
boundary and both lanes run.  Depth = direct_sort_params' depth + 1.  Inputs,
all on the k/N grid (equal, or at least the sign's resolution 1/N apart):
  (a) the bench permutation (distinct);
  (b) every value twice;
  (c) one value at every other index (N/2 copies: equal elements on both sides
      of the wrap for every r), distinct values between them;
  (d) all equal.
The output gate is the reference's own (DirectSortTest: max error < 0.01).
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim

SHAPES = [(8, 12), (64, 12)]
KINDS = ["a", "b", "c", "d"]
GATE = 0.01  # the reference's DirectSortTest gate


def make_input(N, kind):
    rng = np.random.default_rng(20251205 + N)
    perm = rng.permutation(N)
    if kind == "a":
        return (perm / N).astype(float)
    if kind == "b":
        return ((perm // 2) / N).astype(float)
    if kind == "c":
        x = np.empty(N)
        x[0::2] = (N // 4) / N
        others = np.array([k for k in range(N) if k != N // 4][: N // 2])
        x[1::2] = rng.permutation(others) / N
        return x
    return np.full(N, 0.5)


def stable_rank(x):
    return np.argsort(np.argsort(x, kind="stable"), kind="stable")


class Ctx:
    def __init__(self, backend, N, logn, extra=1):
        self.N = N
        self.depth, rots = sfhe.direct_sort_params(N, backend)
        self.depth += extra
        self.cfg = slotsim.default_sign_config(N)
        self.e = sfhe.Engine(backend, mult_depth=self.depth, ring_dim=1 << logn, batch_size=N, rotations=rots,
                             seed=20251205 + N)
        self.e.set_quiet(True)
        self.s = self.e.sorter(N)


@pytest.fixture(scope="module")
def ctxs(oracle_lib):
    out = {(N, logn): Ctx("oracle", N, logn) for N, logn in SHAPES}
    yield out
    for c in out.values():
        c.e.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn", SHAPES)
def test_stable_rank_and_sort(ctxs, N, logn, kind):
    c = ctxs[N, logn]
    x = make_input(N, kind)
    ct = c.e.encrypt(x.tolist())
    rank = c.s.rank_stable(ct, *c.cfg)
    got = np.array(c.e.decrypt(rank))[:N]
    want = stable_rank(x)
    rank_err = float(np.max(np.abs(got - want)))
    out = c.s.sort_stable(ct, *c.cfg)
    dec = np.array(c.e.decrypt(out))[:N]
    out_err = float(np.max(np.abs(dec - np.sort(x))))
    print(f"N={N} ({kind}): stable rank err {rank_err:.3g}, output err {out_err:.3g}, level {out.level}/{c.depth}")
    assert np.array_equal(np.rint(got), want), rank_err
    assert out_err < GATE, out_err
    assert out.level == c.depth
    # one level below the plain rank
    assert rank.level == c.s.rank(ct, *c.cfg).level + 1


@pytest.mark.parametrize("N,logn", SHAPES)
def test_plain_sort_misses_the_gate_on_duplicates(ctxs, N, logn):
    """The gap this feature closes: a pair of equal values x shares the rank
    L + 1/2, and the doubled sinc at offset 1/2 puts 2/pi x from each into
    slots L and L + 1: 1.27 x where x belongs, an error of 0.27 x -- 0.1 for
    the largest pair of (b).  The stable sort of the same ciphertext passes."""
    c = ctxs[N, logn]
    x = make_input(N, "b")
    ct = c.e.encrypt(x.tolist())
    plain = np.array(c.e.decrypt(c.s.sort(ct, *c.cfg)))[:N]
    err = float(np.max(np.abs(plain - np.sort(x))))
    print(f"N={N}: plain sort on duplicates, max err {err:.3g}")
    assert err > 5 * GATE, err


def test_payload_ordered_by_key(ctxs):
    """place(rank_stable(keys), payload): records ordered by key, equal keys
    in input order."""
    N, logn = 64, 12
    c = ctxs[N, logn]
    keys = make_input(N, "b")
    payload = np.random.default_rng(7).permutation(N) / N
    rank = c.s.rank_stable(c.e.encrypt(keys.tolist()), *c.cfg)
    out = c.s.place(rank, c.e.encrypt(payload.tolist()))
    got = np.array(c.e.decrypt(out))[:N]
    want = payload[np.argsort(keys, kind="stable")]
    err = float(np.max(np.abs(got - want)))
    print(f"payload by key: max err {err:.3g}")
    assert err < GATE, err


def test_depth_one_short_is_an_error(oracle_lib):
    """A context at the plain sort's depth: SFHE_ESCHEME with the depth needed
    in the message, from both entry points, before anything is computed."""
    N, logn = 8, 12
    c = Ctx("oracle", N, logn, extra=0)
    ct = c.e.encrypt(make_input(N, "b").tolist())
    c.s.sort(ct, *c.cfg)  # (the plain sort fits)
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {c.depth + 1}\b"):
        c.s.sort_stable(ct, *c.cfg)
    # the stable rank alone fits this context (the placement's levels are free)
    assert c.s.rank_stable(ct, *c.cfg).level == c.s.rank(ct, *c.cfg).level + 1
    rank_depth = c.s.rank_stable(ct, *c.cfg).level
    short = sfhe.Engine("oracle", mult_depth=rank_depth - 1, ring_dim=1 << logn, batch_size=N,
                        rotations=sfhe.direct_sort_params(N, "oracle")[1], seed=1)
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {rank_depth}\b"):
        short.sorter(N).rank_stable(short.encrypt(make_input(N, "b").tolist()), *c.cfg)
    short.close()
    c.e.close()


def test_plain_sort_unchanged_after_a_stable_sort(oracle_lib):
    """A sorter may alternate the two modes (each keeps its own masks and
    captured graph): after a stable sort, the plain sort's residues are those
    of a fresh engine's plain sort (same seed)."""
    N, logn = 8, 12
    x = make_input(N, "a")
    a, b = Ctx("oracle", N, logn), Ctx("oracle", N, logn)
    cta, ctb = a.e.encrypt(x.tolist()), b.e.encrypt(x.tolist())
    assert np.array_equal(cta.download(), ctb.download())
    a.s.sort_stable(cta, *a.cfg)
    for _ in range(2):
        assert np.array_equal(a.s.sort(cta, *a.cfg).download(), b.s.sort(ctb, *b.cfg).download())
        a.s.sort_stable(cta, *a.cfg)
    a.e.close()
    b.e.close()


def test_abi_lists_the_stable_entry_points(oracle_lib):
    for name in ("sfhe_sorter_sort_stable", "sfhe_sorter_rank_stable", "sfhe_tie_counts"):
        assert hasattr(oracle_lib, name), name
