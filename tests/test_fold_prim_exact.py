"""sfp_ks_inner_aut_sum (kernel k_ks_inner_aut_sum) and sfp_ks_inner_aut_sum_cols
(k_ks_inner_aut_sum_cols<2|4>) on chosen residues against Python integers (prims.h):

    acc_p[t] = sum_k sum_j ext_j[t][perm_k] * key_{k,j,p}[kr(t)]  mod q_kr(t)
    perm_k = Ring.aut_perm(gals[k]),  kr(t) = t for t < ell, else Lq + t - ell

with the key layout of prims_cases.case_ks_inner (per digit: NP b rows, then NP a rows).

  generic   ell = 5 of Lq = 7, K = 2, beta = 3, an ext stride one row above the rows; R = 1, 3, 7
            Galois elements out of {5, 25, 125, 5^(n/2-1), 2n-1, 3, 5^3 (2n-1) mod 2n}; rows
            `uniform` and `qm1`; rings 2^12 and 2^11 (one tile).  Also against the composed
            prims: on the device sfp_ks_inner_aut for the first term and sfp_automorph +
            sfp_ks_inner_acc for the others, on the oracle sfp_automorph + sfp_ks_inner(_acc).
  bound     R = 7, beta = 36: 252 products on a prime just below 2^60 (one q prime, one P
            prime).  With every word q - 1 the integer sum is 252 (q - 1)^2, asserted to lie in
            [2^127, 2^128): within 2^-6 of the top of the 128-bit accumulator the kernel
            comment claims ("R * beta <= 2^8 products of 2^120").  The residue is 252.
  declines  every case of prims.h returns -1 with the outputs at their fill and an input intact.
  columns   nc = 1, 2, 3, 5 under both tile widths (SFHE_SELECT_TILE is read per call): the
            launch count of the tiling rule, every column exact and equal to the one-column
            prim's; nc = 4 all q - 1 at 252 products (the 4-tile's accumulators); its declines.

The unmarked tests check the reference against the oracle's composed prims; the device
comparisons are marked gpu.  The prims are weak and bound here by ctypes.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prims_harness as H  # noqa: E402
from prims_harness import Limbs, assert_eq, u64  # noqa: E402

FILL = 0xDEAD
FOLD_MAX, FOLD_COLS, MAX_PRODUCTS = 7, 16, 256  # prims.h SFP_FOLD_MAX, SFP_FOLD_COLS; R * beta
GENERIC = dict(ell=5, K=2, Lq=7, beta=3)
BOUND = dict(ell=1, K=1, Lq=1, beta=36)


def gal_pool(n):
    return [5, 25, 125, pow(5, n // 2 - 1, 2 * n), 2 * n - 1, 3, 125 * (2 * n - 1) % (2 * n)]


def gals_for(n, R):
    pool = gal_pool(n)
    return {1: [pool[6]], 3: [pool[4], pool[5], pool[3]], 7: pool}[R]


def bound_primes(logn):
    m = 2 << logn
    p0 = H.prime_below(1 << 60, m)
    return [p0, H.prime_below(p0, m)]


class Shape:
    def __init__(self, ring, R, ell, K, Lq, beta):
        self.R, self.ell, self.K, self.Lq, self.beta = R, ell, K, Lq, beta
        self.rows, self.NP = ell + K, Lq + K
        self.kr = list(range(ell)) + [Lq + i for i in range(K)]  # key row (= prime) of ext row t
        self.m = Limbs(self.rows, ell, Lq, 0, 0)
        self.q = np.array([ring.primes[p] for p in self.kr], dtype=object).reshape(-1, 1)
        self.qkey = np.array(ring.primes[:self.NP], dtype=object).reshape(-1, 1)
        self.stride = (self.rows + 1) * ring.n  # one row above the rows


def rand_rows(rng, qcol, n):
    return np.stack([H.obj(rng.integers(0, int(q), n, dtype=np.uint64)) for q in qcol.ravel()])


def digits(R, sh, kind, seed):
    """beta digit row sets [rows, n] (object arrays)"""
    if kind == "qm1":
        return [np.broadcast_to(sh.q - 1, (sh.rows, R.n)).copy() for _ in range(sh.beta)]
    rng = np.random.default_rng(seed)
    return [rand_rows(rng, sh.q, R.n) for _ in range(sh.beta)]


def key_rows(R, sh, kind, seed):
    """(kb, ka): beta row sets [NP, n] each"""
    if kind == "qm1":
        full = np.broadcast_to(sh.qkey - 1, (sh.NP, R.n)).copy()
        return [full] * sh.beta, [full] * sh.beta
    rng = np.random.default_rng(seed)
    return ([rand_rows(rng, sh.qkey, R.n) for _ in range(sh.beta)],
            [rand_rows(rng, sh.qkey, R.n) for _ in range(sh.beta)])


def ext_words(sh, ext):
    buf = np.zeros((sh.beta, sh.stride), dtype=np.uint64)
    for j in range(sh.beta):
        buf[j, :ext[j].size] = u64(ext[j]).ravel()
    return buf


def key_words(sh, kb, ka):
    return np.concatenate([np.concatenate([u64(kb[j]), u64(ka[j])]) for j in range(sh.beta)])


def exact_sums(R, sh, ext, keys, gals):
    """the two integer sums BEFORE reduction ([rows, n] object arrays)"""
    s0 = np.zeros((sh.rows, R.n), dtype=object)
    s1 = np.zeros((sh.rows, R.n), dtype=object)
    for (kb, ka), g in zip(keys, gals):
        perm = R.aut_perm(g)
        for j in range(sh.beta):
            e = ext[j][:, perm]
            s0 = s0 + e * kb[j][sh.kr]
            s1 = s1 + e * ka[j][sh.kr]
    return s0, s1


def fold(D, a0, a1, E, stride, keys, gals, R, sh, beta=None, ell=None):
    f = D.lib.sfp_ks_inner_aut_sum
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5
    kp = np.array([int(k or 0) for k in keys] + [0], dtype=np.uint64)
    gv = np.array(list(gals) + [0], dtype=np.uint32)
    r = f(D.d, a0, a1, E, stride, kp.ctypes.data_as(C.c_void_p), gv.ctypes.data_as(C.c_void_p), R,
          sh.beta if beta is None else beta, sh.ell if ell is None else ell, sh.K, sh.Lq)
    D.check()
    return r


def fold_cols(D, a0, a1, E, stride, keys, gals, R, sh):
    f = D.lib.sfp_ks_inner_aut_sum_cols
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_uint32] * 5
    ptr = lambda ps: np.array([int(p) for p in ps] + [0], dtype=np.uint64)
    p0, p1, pe, kp = ptr(a0), ptr(a1), ptr(E), ptr(keys)
    gv = np.array(list(gals) + [0], dtype=np.uint32)
    v = lambda a: a.ctypes.data_as(C.c_void_p)
    r = f(D.d, v(p0), v(p1), v(pe), stride, len(a0), v(kp), v(gv), R, sh.beta, sh.ell, sh.K, sh.Lq)
    D.check()
    return r


def composed(D, E, kd, gals, sh, n, first_aut):
    """term 0 by sfp_ks_inner_aut (first_aut) or sfp_automorph + sfp_ks_inner; the others by
    sfp_automorph of the digits + sfp_ks_inner_acc"""
    words = sh.rows * n
    a0, a1, tmp = D.alloc(words), D.alloc(words), D.alloc(sh.beta * sh.stride, fill=0)
    for k, g in enumerate(gals):
        if k == 0 and first_aut:
            D.call("sfp_ks_inner_aut", a0, a1, E, sh.stride, kd[0], sh.beta, sh.ell, sh.K, sh.Lq, g)
            continue
        for j in range(sh.beta):
            D.call("sfp_automorph", tmp + 8 * j * sh.stride, E + 8 * j * sh.stride, g, sh.m)
        D.call("sfp_ks_inner_acc" if k else "sfp_ks_inner", a0, a1, tmp, sh.stride, kd[k], sh.beta, sh.ell, sh.K,
               sh.Lq)
    return D.down(a0, (sh.rows, n)), D.down(a1, (sh.rows, n))


_cases = {}


def generic_case(logn, R_, kind):
    """(ring, shape, digits, keys, gals, exact acc0, exact acc1), built once per process"""
    key = (logn, R_, kind)
    if key not in _cases:
        R = H.ring(H.prime_set(logn), logn)
        sh = Shape(R, R_, **GENERIC)
        ext = digits(R, sh, kind, 100 + R_)
        keys = [key_rows(R, sh, kind, 200 + 10 * R_ + k) for k in range(R_)]
        gals = gals_for(R.n, R_)
        s0, s1 = exact_sums(R, sh, ext, keys, gals)
        _cases[key] = (R, sh, ext, keys, gals, s0 % sh.q, s1 % sh.q)
    return _cases[key]


def bound_case(kind, logn=12):
    key = ("bound", kind)
    if key not in _cases:
        R = H.ring(bound_primes(logn), logn)
        sh = Shape(R, FOLD_MAX, **BOUND)
        ext = digits(R, sh, kind, 7)
        kb, ka = key_rows(R, sh, kind, 8)
        gals = gal_pool(R.n)
        s0, s1 = exact_sums(R, sh, ext, [(kb, ka)] * FOLD_MAX, gals)  # one key buffer serves the seven terms
        _cases[key] = (R, sh, ext, (kb, ka), gals, s0, s1)
    return _cases[key]


def assert_at_the_bound(sh, s0, s1):
    """the qm1 sums sit at the accumulator's bound: 252 products, in [2^127, 2^128)"""
    assert sh.R * sh.beta == 252 and sh.R * sh.beta <= MAX_PRODUCTS
    for s in (s0, s1):
        assert (1 << 127) <= int(np.min(s)) and int(np.max(s)) < (1 << 128)
        assert np.all(s % sh.q == 252)


# ---- not marked gpu: the reference against the oracle's composed prims ----------------------


def test_galois_pool_is_odd_and_distinct():
    for logn in (11, 12):
        n = 1 << logn
        pool = gal_pool(n)
        assert len(set(pool)) == 7 and all(g & 1 and g < 2 * n for g in pool)
        assert 2 * n - 1 in pool and 3 in pool


@pytest.mark.parametrize("kind", ["uniform", "qm1"])
@pytest.mark.parametrize("R_", [1, 3, 7])
def test_reference_is_the_oracles_composed_form(oracle_lib, R_, kind):
    R, sh, ext, keys, gals, w0, w1 = generic_case(12, R_, kind)
    D = H.dev(oracle_lib, "oracle", R.primes, 12)
    E = D.up(ext_words(sh, ext))
    kd = [D.up(key_words(sh, kb, ka)) for kb, ka in keys]
    g0, g1 = composed(D, E, kd, gals, sh, R.n, first_aut=False)
    assert_eq(g0, w0, "oracle composed acc0")
    assert_eq(g1, w1, "oracle composed acc1")
    D.release()


def test_bound_case_sits_at_the_bound(oracle_lib):
    """252 (q - 1)^2 lies in [2^127, 2^128); the seeded uniform sum at the same shape does not
    reach it (which is why the qm1 input exists).  The oracle's composed form gives 252."""
    R, sh, ext, (kb, ka), gals, s0, s1 = bound_case("qm1")
    assert min(R.primes) > (1 << 60) - (1 << 40)
    assert_at_the_bound(sh, s0, s1)
    _, _, _, _, _, u0, _ = bound_case("uniform")
    assert int(np.max(u0)) < (1 << 127)
    D = H.dev(oracle_lib, "oracle", R.primes, 12)
    E, kd = D.up(ext_words(sh, ext)), D.up(key_words(sh, kb, ka))
    g0, g1 = composed(D, E, [kd] * FOLD_MAX, gals, sh, R.n, first_aut=False)
    assert_eq(g0, s0 % sh.q, "oracle composed acc0 at the bound")
    assert_eq(g1, s1 % sh.q, "oracle composed acc1 at the bound")
    D.release()


def tile_launches(nc, wide):
    """the tiling rule of sfp_ks_inner_aut_sum_cols, restated: tiles of `wide`, a remainder of
    2 or 3 as a 2-tile (+ 1), a remainder of 1 as the one-column prim"""
    c, out = 0, []
    while c < nc:
        left = nc - c
        ct = wide if left >= wide else 2 if left >= 2 else 1
        out.append(ct)
        c += ct
    return out


def test_tiling_rule_leaves_a_single_column_under_both_widths():
    assert [len(tile_launches(nc, 2)) for nc in (1, 2, 3, 5)] == [1, 1, 2, 3]
    assert [len(tile_launches(nc, 4)) for nc in (1, 2, 3, 5)] == [1, 1, 2, 2]
    for wide in (2, 4):
        assert tile_launches(1, wide) == [1] and tile_launches(3, wide) == [2, 1]
        assert tile_launches(5, wide)[-1] == 1
    assert tile_launches(4, 4) == [4] and tile_launches(4, 2) == [2, 2]


# ---- marked gpu -----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def hip(hip_lib):
    return lambda primes, logn: H.dev(hip_lib, "hip", primes, logn)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "qm1"])
@pytest.mark.parametrize("logn,R_", [(12, 1), (12, 3), (12, 7), (11, 7)])
def test_fold_exact_and_composed(hip, oracle_lib, logn, R_, kind):
    R, sh, ext, keys, gals, w0, w1 = generic_case(logn, R_, kind)
    D = hip(R.primes, logn)
    assert D.has("sfp_ks_inner_aut_sum")
    words = sh.rows * R.n
    E = D.up(ext_words(sh, ext))
    kd = [D.up(key_words(sh, kb, ka)) for kb, ka in keys]
    a0, a1 = D.alloc(words + 2, fill=FILL), D.alloc(words + 2, fill=FILL)
    assert fold(D, a0, a1, E, sh.stride, kd, gals, R_, sh) == 0
    g0, g1 = D.down(a0, (sh.rows, R.n)), D.down(a1, (sh.rows, R.n))
    assert_eq(g0, w0, "ks_inner_aut_sum acc0 R=%d %s" % (R_, kind))
    assert_eq(g1, w1, "ks_inner_aut_sum acc1 R=%d %s" % (R_, kind))
    assert (D.down(a0, (2,), words) == FILL).all() and (D.down(a1, (2,), words) == FILL).all()
    c0, c1 = composed(D, E, kd, gals, sh, R.n, first_aut=True)
    assert np.array_equal(c0, g0) and np.array_equal(c1, g1)
    D.release()
    if logn == 11:  # (the oracle's composed form at 2^12 is the unmarked test)
        O = H.dev(oracle_lib, "oracle", R.primes, logn)
        o0, o1 = composed(O, O.up(ext_words(sh, ext)), [O.up(key_words(sh, kb, ka)) for kb, ka in keys], gals, sh,
                          R.n, first_aut=False)
        assert np.array_equal(o0, g0) and np.array_equal(o1, g1)
        O.release()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["qm1", "uniform"])
def test_fold_at_the_accumulator_bound(hip, kind):
    R, sh, ext, (kb, ka), gals, s0, s1 = bound_case(kind)
    if kind == "qm1":
        assert_at_the_bound(sh, s0, s1)
    D = hip(R.primes, 12)
    words = sh.rows * R.n
    E, kd = D.up(ext_words(sh, ext)), D.up(key_words(sh, kb, ka))
    a0, a1 = D.alloc(words, fill=FILL), D.alloc(words, fill=FILL)
    assert fold(D, a0, a1, E, sh.stride, [kd] * FOLD_MAX, gals, FOLD_MAX, sh) == 0
    assert_eq(D.down(a0, (sh.rows, R.n)), s0 % sh.q, "252 products acc0 " + kind)
    assert_eq(D.down(a1, (sh.rows, R.n)), s1 % sh.q, "252 products acc1 " + kind)
    D.release()


@pytest.mark.gpu
def test_fold_declines(hip):
    """-1, the outputs at their fill, an input unchanged; then the plain call is exact."""
    R, sh, ext, keys, gals, w0, w1 = generic_case(12, 7, "uniform")
    D = hip(R.primes, 12)
    n, words = R.n, sh.rows * R.n
    ew, kw = ext_words(sh, ext), [key_words(sh, kb, ka) for kb, ka in keys]
    E = D.alloc(ew.size + 2, fill=0)
    D.put(E, ew)
    kd = []
    for w in kw:
        p = D.alloc(w.size + 2, fill=0)
        D.put(p, w)
        kd.append(p)
    a0, a1 = D.alloc(words + 2, fill=FILL), D.alloc(words + 2, fill=FILL)

    def untouched(what):
        for p in (a0, a1):
            assert (D.down(p, (words + 2,)) == FILL).all(), what + ": an output was written"
        assert np.array_equal(D.down(E, ew.shape), ew), what + ": the digits were written"
        assert np.array_equal(D.down(kd[0], kw[0].shape), kw[0]), what + ": a key was written"

    k1, g1 = kd[:1], gals[:1]
    cases = [
        ("R = 0", dict(keys=kd, gals=gals, R=0)),
        ("R = 8", dict(keys=kd + kd[:1], gals=gals + gals[:1], R=8)),
        ("beta = 0", dict(keys=kd, gals=gals, R=7, beta=0)),
        ("R * beta = 259", dict(keys=kd, gals=gals, R=7, beta=37)),
        ("R * beta = 257", dict(keys=k1, gals=g1, R=1, beta=257)),
        ("an even Galois element", dict(keys=kd, gals=gals[:3] + [4] + gals[4:], R=7)),
        ("a Galois element 2n + 1", dict(keys=kd, gals=gals[:6] + [2 * n + 1], R=7)),
        ("a Galois element 2n", dict(keys=k1, gals=[2 * n], R=1)),
        ("a null key", dict(keys=kd[:2] + [None] + kd[3:], gals=gals, R=7)),
        ("ell > Lq", dict(keys=kd, gals=gals, R=7, ell=sh.Lq + 1)),
        ("ext_stride below the rows", dict(keys=kd, gals=gals, R=7, stride=words - 2)),
        ("acc0 off alignment", dict(keys=kd, gals=gals, R=7, a0=a0 + 8)),
        ("acc1 off alignment", dict(keys=kd, gals=gals, R=7, a1=a1 + 8)),
        ("ext off alignment", dict(keys=kd, gals=gals, R=7, E=E + 8)),
        ("a key off alignment", dict(keys=kd[:6] + [kd[6] + 8], gals=gals, R=7)),
    ]
    for what, kw_ in cases:
        r = fold(D, kw_.get("a0", a0), kw_.get("a1", a1), kw_.get("E", E), kw_.get("stride", sh.stride), kw_["keys"],
                 kw_["gals"], kw_["R"], sh, beta=kw_.get("beta"), ell=kw_.get("ell"))
        assert r == -1, what
        untouched(what)
    assert fold(D, a0, a1, E, sh.stride, kd, gals, 7, sh) == 0
    assert_eq(D.down(a0, (sh.rows, n)), w0, "after the declines acc0")
    assert_eq(D.down(a1, (sh.rows, n)), w1, "after the declines acc1")
    D.release()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [None, "4"], ids=["tile2", "tile4"])
@pytest.mark.parametrize("nc", [1, 2, 3, 5])
def test_fold_cols_exact_launches_and_one_column(hip, monkeypatch, nc, tile):
    if tile is None:
        monkeypatch.delenv("SFHE_SELECT_TILE", raising=False)
    else:
        monkeypatch.setenv("SFHE_SELECT_TILE", tile)
    R, sh, _, keys, gals, _, _ = generic_case(12, 3, "uniform")
    D = hip(R.primes, 12)
    assert D.has("sfp_ks_inner_aut_sum_cols")
    words = sh.rows * R.n
    kd = [D.up(key_words(sh, kb, ka)) for kb, ka in keys]
    exts = [digits(R, sh, "uniform", 500 + c) for c in range(nc)]  # distinct digits per column
    E = [D.up(ext_words(sh, e)) for e in exts]
    a0 = [D.alloc(words + 2, fill=FILL) for _ in range(nc)]
    a1 = [D.alloc(words + 2, fill=FILL) for _ in range(nc)]
    assert fold_cols(D, a0, a1, E, sh.stride, kd, gals, 3, sh) == len(tile_launches(nc, int(tile or 2)))
    b0, b1 = D.alloc(words), D.alloc(words)
    for c in range(nc):
        s0, s1 = exact_sums(R, sh, exts[c], keys, gals)
        g0, g1 = D.down(a0[c], (sh.rows, R.n)), D.down(a1[c], (sh.rows, R.n))
        assert_eq(g0, s0 % sh.q, "cols nc=%d column %d acc0" % (nc, c))
        assert_eq(g1, s1 % sh.q, "cols nc=%d column %d acc1" % (nc, c))
        assert (D.down(a0[c], (2,), words) == FILL).all() and (D.down(a1[c], (2,), words) == FILL).all()
        assert fold(D, b0, b1, E[c], sh.stride, kd, gals, 3, sh) == 0
        assert np.array_equal(D.down(b0, (sh.rows, R.n)), g0) and np.array_equal(D.down(b1, (sh.rows, R.n)), g1)
    D.release()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [None, "4"], ids=["tile2", "tile4"])
def test_fold_cols_at_the_accumulator_bound(hip, monkeypatch, tile):
    """nc = 4, every word q - 1, 252 products per column: one 4-tile (or two 2-tiles)."""
    if tile is None:
        monkeypatch.delenv("SFHE_SELECT_TILE", raising=False)
    else:
        monkeypatch.setenv("SFHE_SELECT_TILE", tile)
    R, sh, ext, (kb, ka), gals, s0, s1 = bound_case("qm1")
    assert_at_the_bound(sh, s0, s1)
    D = hip(R.primes, 12)
    words = sh.rows * R.n
    kd = D.up(key_words(sh, kb, ka))
    E = [D.up(ext_words(sh, ext)) for _ in range(4)]
    a0 = [D.alloc(words, fill=FILL) for _ in range(4)]
    a1 = [D.alloc(words, fill=FILL) for _ in range(4)]
    assert fold_cols(D, a0, a1, E, sh.stride, [kd] * FOLD_MAX, gals, FOLD_MAX, sh) == (1 if tile else 2)
    for c in range(4):
        assert (D.down(a0[c], (sh.rows, R.n)) == 252).all(), c
        assert (D.down(a1[c], (sh.rows, R.n)) == 252).all(), c
    D.release()


@pytest.mark.gpu
def test_fold_cols_declines(hip, monkeypatch):
    monkeypatch.delenv("SFHE_SELECT_TILE", raising=False)
    R, sh, ext, keys, gals, w0, w1 = generic_case(12, 3, "uniform")
    D = hip(R.primes, 12)
    n, words = R.n, sh.rows * R.n
    kd = [D.up(key_words(sh, kb, ka)) for kb, ka in keys]
    kw0 = key_words(sh, *keys[0])
    lead = D.alloc(words + kw0.size, fill=FILL)  # key 0 once more, behind `words` words of fill:
    kd[0] = lead + 8 * words                     # an output may then END inside a key, in bounds
    D.put(kd[0], kw0)
    ew = ext_words(sh, ext)
    NC = FOLD_COLS + 1
    E = [D.up(ew) for _ in range(2)]
    a0 = [D.alloc(words + n, fill=FILL) for _ in range(NC)]  # (a row more: every span tried is in bounds)
    a1 = [D.alloc(words + n, fill=FILL) for _ in range(NC)]
    half = 8 * (n // 2)  # half a row, in bytes

    def untouched(what):
        for p in a0 + a1:
            assert (D.down(p, (words + n,)) == FILL).all(), what + ": an output was written"
        assert (D.down(lead, (words,)) == FILL).all(), what + ": an output was written"
        assert np.array_equal(D.down(kd[0], kw0.shape), kw0), what + ": a key was written"
        assert np.array_equal(D.down(E[0], ew.shape), ew), what + ": the digits were written"

    assert fold_cols(D, [], [], [], sh.stride, kd, gals, 3, sh) == -1
    untouched("nc = 0")
    assert fold_cols(D, a0, a1, [E[0]] * NC, sh.stride, kd, gals, 3, sh) == -1
    untouched("nc = 17")
    two = lambda x0, x1: fold_cols(D, x0, x1, E, sh.stride, kd, gals, 3, sh)
    assert two([E[1], a0[1]], a1[:2]) == -1
    assert two(a0[:2], [a1[0], E[0]]) == -1
    untouched("an output equal to an ext")
    assert two([E[0] + half, a0[1]], a1[:2]) == -1
    assert two(a0[:2], [a1[0], E[1] + 8 * sh.stride - half]) == -1  # ends half a row into digit 1
    untouched("an output reaching into an ext")
    assert two([kd[2] + half, a0[1]], a1[:2]) == -1
    assert two(a0[:2], [lead + half, a1[1]]) == -1  # ends half a row into key 0
    untouched("an output reaching into a key")
    assert two([a0[0], a0[0] + half], a1[:2]) == -1
    assert two(a0[:2], [a0[1] + half, a1[1]]) == -1
    assert two(a0[:2], [a1[0], a1[0]]) == -1
    untouched("an output reaching into another output")
    assert two(a0[:2], a1[:2]) == 1  # and the plain call runs
    for c in range(2):
        assert_eq(D.down(a0[c], (sh.rows, n)), w0, "after the declines column %d acc0" % c)
        assert_eq(D.down(a1[c], (sh.rows, n)), w1, "after the declines column %d acc1" % c)
    D.release()
