"""Selection by rank (DirectSort<N>::selectRanks / select, EvalRotateFold;
DESIGN.md §4g) on the C oracle.

select_ranked(rank, x, T): slot i < K of the N-slot result holds the element
whose rank is T[i], the other slots hold 0.  The oracle runs the composed
fold (sfp_automorph + sfp_ks_inner / sfp_ks_inner_acc per term).

Shapes (tests/test_stable_sort.py's): N = 8 at ring 2^12 -- Psel <= 8, one
batch, fold steps (stride 1, count 4) and (stride 4, count 2) -- and N = 64 at
ring 2^12 -- P = 32, so K = 40 takes two batches, the second with 8 real
targets and 24 padded ones; three fold steps of count 4.  The rotation keys
are select_params': direct_sort_params' list lacks 3 at N = 8 and 12 at N = 64.
The gate is the reference's own (DirectSortTest: max error < 0.01).
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim

SHAPES = [(8, 12), (64, 12)]
GATE = 0.01  # the reference's DirectSortTest gate


def make_input(N, kind="a"):
    rng = np.random.default_rng(20251205 + N)
    perm = rng.permutation(N)
    return ((perm // 2 if kind == "b" else perm) / N).astype(float)


def target_lists(N):
    rng = np.random.default_rng(11 + N)
    out = {"min": [0], "max": [N - 1], "median": [N // 2], "five": list(range(5)),
           "seven": [int(t) for t in rng.permutation(N)[:7]], "all": list(range(N))}
    if N == 64:
        out["forty"] = [int(t) for t in rng.permutation(N)[:40]]
    return out


CASES = [(N, logn, name) for N, logn in SHAPES for name in target_lists(N)]


def batches_of(N, logn, K):
    P = min(N, (1 << logn) // 2 // N)
    psel = 1
    while psel < K and psel < P:
        psel *= 2
    return -(-K // psel)


class Ctx:
    def __init__(self, backend, N, logn, extra=1, rots=None, depth=None):
        self.N = N
        self.depth, sel = sfhe.select_params(N, backend)
        self.depth = depth if depth is not None else self.depth + extra
        self.rots = sel if rots is None else rots
        self.cfg = slotsim.default_sign_config(N)
        self.e = sfhe.Engine(backend, mult_depth=self.depth, ring_dim=1 << logn, batch_size=N, rotations=self.rots,
                             seed=20251205 + N)
        self.e.set_quiet(True)
        self.s = self.e.sorter(N, rotations=self.rots)


class Ranked:
    """One context per shape with the ranks every case shares (computed once)."""

    def __init__(self, N, logn):
        self.c = Ctx("oracle", N, logn)
        self.x = make_input(N)
        self.ct = self.c.e.encrypt(self.x.tolist())
        self.rank = self.c.s.rank(self.ct, *self.c.cfg)
        self.place_level = self.c.s.place(self.rank, self.ct.clone()).level


@pytest.fixture(scope="module")
def ranked(oracle_lib):
    out = {(N, logn): Ranked(N, logn) for N, logn in SHAPES}
    yield out
    for r in out.values():
        r.c.e.close()


def check(got, x_sorted_by_rank, T, N):
    want = np.zeros(N)
    want[: len(T)] = x_sorted_by_rank[T]
    return float(np.max(np.abs(np.asarray(got)[:N] - want)))


@pytest.mark.parametrize("N,logn,name", CASES)
def test_select_ranked(ranked, N, logn, name):
    r = ranked[N, logn]
    T = target_lists(N)[name]
    r.c.e.op_stats(reset=True)
    out = r.c.s.select_ranked(r.rank, r.ct, T)
    batches, fused, composed = r.c.e.select_counts()
    err = check(r.c.e.decrypt(out), np.sort(r.x), T, N)
    print(f"N={N} {name} (K={len(T)}): max err {err:.3g}, level {out.level}, batches {batches}, "
          f"folds fused {fused} composed {composed}")
    assert err < GATE, err
    assert out.level == r.place_level
    assert out.slots == N
    assert batches == batches_of(N, logn, len(T))
    # the oracle has no fused prim: every fold of every batch is composed
    steps = 2 if N == 8 else 3
    assert (fused, composed) == (0, steps * batches)


@pytest.mark.parametrize("N,logn", SHAPES)
def test_duplicates_need_the_stable_rank(ranked, N, logn):
    """Input (b), every value twice: the stable rank selects the right elements;
    the plain rank gives two elements the rank L + 1/2, which no integer target
    hits (as test_plain_sort_misses_the_gate_on_duplicates shows for the sort)."""
    c = ranked[N, logn].c
    x = make_input(N, "b")
    ct = c.e.encrypt(x.tolist())
    T = list(range(N))
    stable = c.s.select(ct, T, stable=True, n=c.cfg[0], dg=c.cfg[1], df=c.cfg[2])
    err = check(c.e.decrypt(stable), np.sort(x), T, N)
    plain = c.s.select(ct, T, stable=False, n=c.cfg[0], dg=c.cfg[1], df=c.cfg[2])
    perr = check(c.e.decrypt(plain), np.sort(x), T, N)
    print(f"N={N}: duplicates, stable max err {err:.3g}, plain max err {perr:.3g}")
    assert err < GATE, err
    assert perr > 5 * GATE, perr
    assert stable.level == c.depth


def test_payload_selected_by_the_keys_rank(ranked):
    N, logn = 64, 12
    r = ranked[N, logn]
    payload = np.random.default_rng(7).permutation(N) / N
    T = target_lists(N)["seven"]
    out = r.c.s.select_ranked(r.rank, r.c.e.encrypt(payload.tolist()), T)
    err = check(r.c.e.decrypt(out), payload[np.argsort(r.x)], T, N)
    print(f"payload by key rank: max err {err:.3g}")
    assert err < GATE, err


def test_top_k_and_kth(ranked):
    N, logn = 8, 12
    r = ranked[N, logn]
    kw = dict(n=r.c.cfg[0], dg=r.c.cfg[1], df=r.c.cfg[2])
    xs = np.sort(r.x)
    small = np.array(r.c.e.decrypt(r.c.s.top_k(r.ct, 3, **kw)))[:N]
    large = np.array(r.c.e.decrypt(r.c.s.top_k(r.ct, 3, largest=True, **kw)))[:N]
    kth = np.array(r.c.e.decrypt(r.c.s.kth(r.ct, N // 2, **kw)))[:N]
    assert np.max(np.abs(small - np.r_[xs[:3], np.zeros(N - 3)])) < GATE
    assert np.max(np.abs(large - np.r_[xs[::-1][:3], np.zeros(N - 3)])) < GATE
    assert np.max(np.abs(kth - np.r_[xs[N // 2], np.zeros(N - 1)])) < GATE


@pytest.mark.parametrize("stride,count", [(1, 4), (4, 2), (16, 4), (1, 8)])
def test_rotate_fold(ranked, stride, count):
    """rotate_fold = the sum of numpy rolls; 64 slots, keys of select_params(64)
    (k * stride for (1, 8) needs 1 .. 7: all in the sort's list)."""
    N, logn = 64, 12
    c = ranked[N, logn].c
    v = np.random.default_rng(3).uniform(-1, 1, N)
    ct = c.e.encrypt(v.tolist())
    c.e.op_stats(reset=True)
    out = c.e.rotate_fold(ct, stride, count)
    want = sum(np.roll(v, -k * stride) for k in range(count))
    err = float(np.max(np.abs(np.array(c.e.decrypt(out))[:N] - want)))
    print(f"rotate_fold({stride}, {count}): max err {err:.3g}")
    assert err < 1e-6, err
    assert out.level == ct.level
    assert c.e.select_counts() == (0, 0, 1)


def test_rotate_fold_identity_terms(ranked):
    """A term whose amount is a multiple of the slot count is added as it is:
    stride 32 at 64 slots, count 4 = 2 x + 2 rot(x, 32)."""
    N, logn = 64, 12
    c = ranked[N, logn].c
    v = np.random.default_rng(4).uniform(-1, 1, N)
    out = c.e.rotate_fold(c.e.encrypt(v.tolist()), 32, 4)
    want = 2 * v + 2 * np.roll(v, -32)
    assert float(np.max(np.abs(np.array(c.e.decrypt(out))[:N] - want))) < 1e-6
    # every term an identity: no key is needed
    out = c.e.rotate_fold(c.e.encrypt(v.tolist()), 64, 3)
    assert float(np.max(np.abs(np.array(c.e.decrypt(out))[:N] - 3 * v))) < 1e-6


def test_argument_errors(ranked):
    N, logn = 8, 12
    r = ranked[N, logn]
    for bad in ([0, 0], [N], [], list(range(N)) + [0]):
        with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
            r.c.s.select_ranked(r.rank, r.ct, bad)
        with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
            r.c.s.select(r.ct, bad, n=r.c.cfg[0], dg=r.c.cfg[1], df=r.c.cfg[2])
    for count in (0, 1, 9):
        with pytest.raises(sfhe.SfheError, match="sfhe error -1:"):
            r.c.e.rotate_fold(r.ct, 1, count)


def test_missing_fold_key_and_depth(oracle_lib):
    """The sort's own key list lacks the fold amount 3 at N = 8: SFHE_ESCHEME
    naming the amount.  A context one level short: SFHE_ESCHEME naming the depth."""
    N, logn = 8, 12
    depth, sort_rots = sfhe.direct_sort_params(N, "oracle")
    assert 3 not in sort_rots and 3 in sfhe.select_params(N, "oracle")[1]
    assert sfhe.select_params(N, "oracle")[0] == depth
    assert 12 not in sfhe.direct_sort_params(64, "oracle")[1] and 12 in sfhe.select_params(64, "oracle")[1]
    assert sfhe.select_params(256, "oracle")[1] == sorted(sfhe.direct_sort_params(256, "oracle")[1])
    c = Ctx("oracle", N, logn, rots=sort_rots)
    ct = c.e.encrypt(make_input(N).tolist())
    rank = c.s.rank(ct, *c.cfg)
    with pytest.raises(sfhe.SfheError, match=r"sfhe error -2: .*rotation 3\b"):
        c.s.select_ranked(rank, ct, [0])
    with pytest.raises(sfhe.SfheError, match=r"sfhe error -2: .*rotation 3\b"):
        c.e.rotate_fold(ct, 1, 4)
    c.e.close()
    short = Ctx("oracle", N, logn, depth=depth - 1)
    ct = short.e.encrypt(make_input(N).tolist())
    rank = short.s.rank(ct, *short.cfg)
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {depth}\b"):
        short.s.select_ranked(rank, ct, [0])
    short.e.close()


def test_abi_lists_the_selection_entry_points(oracle_lib):
    for name in ("sfhe_select_params", "sfhe_sorter_select_ranked", "sfhe_sorter_select", "sfhe_eval_rotate_fold",
                 "sfhe_select_counts"):
        assert hasattr(oracle_lib, name), name
        assert name in sfhe.ABI_SYMBOLS


def test_sort_unchanged_after_a_select(oracle_lib):
    """The selection's masks live under their own memo tags: after a select, the
    sort's residues are those of a fresh engine's sort (same seed)."""
    N, logn = 8, 12
    x = make_input(N)
    a, b = Ctx("oracle", N, logn), Ctx("oracle", N, logn)
    cta, ctb = a.e.encrypt(x.tolist()), b.e.encrypt(x.tolist())
    assert np.array_equal(cta.download(), ctb.download())
    a.s.select(cta, [0, 3], n=a.cfg[0], dg=a.cfg[1], df=a.cfg[2])
    for _ in range(2):
        assert np.array_equal(a.s.sort(cta, *a.cfg).download(), b.s.sort(ctb, *b.cfg).download())
        a.s.select(cta, [N - 1], n=a.cfg[0], dg=a.cfg[1], df=a.cfg[2])
    a.e.close()
    b.e.close()
