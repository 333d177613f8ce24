"""sfp_lex_tensor (kernel k_lex_tensor: the lexicographic rank's Horner step before its
relinearisation, prims.h) on chosen residues against Python integers, against the composed
generic primitives on the device and on the oracle, and its three decline cases.

    a0 = kr - q0, a1 = -q1
    d0 = lr v0 + a0 u0,  d1 = lr v1 + a0 u1 + a1 u0,  d2 = a1 u1        (mod each limb's prime)

Ring 2^12 with l = 3 (a 60-bit, a 30-bit and an FP64-range prime) and l = SFP_MAX_LIMBS = 96
(48 primes, each twice: the doubled map the engine uses for [c0 rows][c1 rows]).  Residues:
  qm1      every row and both constants q - 1;
  zero     everything 0;
  bound    kr = lr = q - 1, q0 = 0, q1 = 1, v and u all q - 1: a0 = a1 = q - 1 and d1 is three
           products (q - 1)^2 -- the stated 3 * 2^120 bound of the 128-bit accumulator on the
           primes just below 2^60;
  uniform  seeded random residues and constants.
The prim is weak and bound here by ctypes (the harness modules are imported, not edited).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prims_harness as H  # noqa: E402
from prims_harness import Limbs, assert_eq, u64  # noqa: E402

pytestmark = pytest.mark.gpu

LOGN = 12
MAX_LIMBS = 96  # prims.h SFP_MAX_LIMBS
FILL = 0xDEAD


def primes48():
    m = 2 << LOGN
    out = H.prime_set(LOGN)
    b60, b42 = min(p for p in out if p > 1 << 59), min(p for p in out if (1 << 41) < p < H.FP_BOUND)
    while len(out) < 48:
        if len(out) % 2:
            b60 = H.prime_below(b60, m)
            out.append(b60)
        else:
            b42 = H.prime_below(b42, m)
            out.append(b42)
    assert len(set(out)) == 48
    return out


@pytest.fixture(scope="module")
def devs(hip_lib, oracle_lib):
    pr = primes48()
    return H.ring(pr, LOGN), H.dev(hip_lib, "hip", pr, LOGN), H.dev(oracle_lib, "oracle", pr, LOGN)


def lex_tensor(D, d, v, q, u, kr, lr, m):
    f = D.lib.sfp_lex_tensor
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 12 + [Limbs]
    kr, lr = u64(kr), u64(lr)
    r = f(D.d, d[0], d[1], d[2], v[0], v[1], q[0], q[1], u[0], u[1], kr.ctypes.data_as(C.c_void_p),
          lr.ctypes.data_as(C.c_void_p), m)
    D.check()
    return r


def limb_maps():
    return {3: H.ident(3), MAX_LIMBS: Limbs(MAX_LIMBS, MAX_LIMBS // 2, 0, 0, 0)}


def rows(R, m, kind, seed):
    """six rows v0 v1 q0 q1 u0 u1 ([count, n] object arrays) and the constants kr, lr"""
    P = np.array([R.primes[p] for p in m.primes()], dtype=object)
    col = P.reshape(-1, 1)
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=object).reshape(-1, 1), (m.count, R.n)).copy()
    if kind == "qm1":
        return [full(P - 1) for _ in range(6)], P - 1, P - 1
    if kind == "zero":
        return [full(P * 0) for _ in range(6)], P * 0, P * 0
    if kind == "bound":
        x = full(P - 1)
        return [x, x, full(P * 0), full(P * 0 + 1), x, x], P - 1, P - 1
    rng = np.random.default_rng(seed)
    rand = lambda: np.stack([H.obj(rng.integers(0, int(p), R.n, dtype=np.uint64)) for p in P])
    out = [rand() for _ in range(6)]
    const = lambda: H.obj(rng.integers(0, 1 << 62, m.count, dtype=np.uint64)) % P
    return out, const(), const()


def exact(R, m, x, kr, lr):
    P = np.array([R.primes[p] for p in m.primes()], dtype=object).reshape(-1, 1)
    v0, v1, q0, q1, u0, u1 = x
    kr, lr = kr.reshape(-1, 1), lr.reshape(-1, 1)
    a0, a1 = (kr - q0) % P, (-q1) % P
    d1 = lr * v1 + a0 * u1 + a1 * u0
    assert int(np.max(d1)) < 3 << 120  # the stated bound of the one 128-bit reduction
    return (lr * v0 + a0 * u0) % P, d1 % P, a1 * u1 % P


def composed(D, dp, kr, lr, m, words):
    """the same integers from the generic prims (the engine's composed path)"""
    v0, v1, q0, q1, u0, u1 = dp
    a0, a1, l0, l1, d0, d1, d2 = (D.alloc(words) for _ in range(7))
    D.call("sfp_neg", a0, q0, m)
    D.call("sfp_neg", a1, q1, m)
    D.call("sfp_add_const", a0, a0, u64(kr), m)
    D.call("sfp_tensor", d0, d1, d2, a0, a1, u0, u1, m)
    D.call("sfp_mul_const", l0, v0, u64(lr), m)
    D.call("sfp_mul_const", l1, v1, u64(lr), m)
    D.call("sfp_add", d0, d0, l0, m)
    D.call("sfp_add", d1, d1, l1, m)
    return d0, d1, d2


@pytest.mark.parametrize("kind", ["qm1", "zero", "bound", "uniform"])
@pytest.mark.parametrize("ell", [3, MAX_LIMBS])
def test_lex_tensor_exact_and_composed(devs, ell, kind):
    R, hip, oracle = devs
    assert hip.has("sfp_lex_tensor") and not oracle.has("sfp_lex_tensor")
    m = limb_maps()[ell]
    x, kr, lr = rows(R, m, kind, 20251205 + ell)
    want = exact(R, m, x, kr, lr)
    if kind == "bound":  # three products (q - 1)^2 on a prime just below 2^60
        assert max(R.primes[p] for p in m.primes()) > (1 << 60) - (1 << 40)
    shape, words = (m.count, R.n), m.count * R.n
    for D in (hip, oracle):
        dp = [D.up(u64(r)) for r in x]
        c = composed(D, dp, kr, lr, m, words)
        got_c = [D.down(p, shape) for p in c]
        for i in range(3):
            assert_eq(got_c[i], want[i], "composed d%d %s l=%d %s" % (i, kind, ell, D is hip and "hip" or "oracle"))
        if D is hip:
            d = [D.alloc(words, fill=FILL) for _ in range(3)]
            assert lex_tensor(D, d, dp[0:2], dp[2:4], dp[4:6], kr, lr, m) == 0
            for i in range(3):
                got = D.down(d[i], shape)
                assert_eq(got, want[i], "lex_tensor d%d %s l=%d" % (i, kind, ell))
                assert np.array_equal(got, got_c[i])
        D.release()


def test_lex_tensor_declines(devs):
    """-1 with nothing written: more than SFP_MAX_LIMBS rows, a row off 16-byte alignment, an
    output overlapping an input."""
    R, hip, _ = devs
    D = hip
    big = Limbs(MAX_LIMBS + 1, 48, 0, 0, 0)  # 48 + 49 rows: one row too many
    m = H.ident(3)
    x, kr, lr = rows(R, m, "uniform", 5)
    words = (MAX_LIMBS + 1) * R.n
    ins = [D.alloc(words + 2, fill=1) for _ in range(6)]
    for p, r in zip(ins, x):
        D.put(p, u64(r))
    outs = [D.alloc(words + 2, fill=FILL) for _ in range(3)]
    kbig, lbig = np.ones(MAX_LIMBS + 1, dtype=object), np.ones(MAX_LIMBS + 1, dtype=object)

    def untouched(what):
        for p in outs:
            assert (D.down(p, (words + 2,)) == FILL).all(), what + ": an output was written"
        assert np.array_equal(D.down(ins[0], (3, R.n)), u64(x[0])), what + ": an input was written"

    assert lex_tensor(D, outs, ins[0:2], ins[2:4], ins[4:6], kbig, lbig, big) == -1
    untouched("too many rows")
    for k in range(6):  # an input row 8 bytes off
        off = list(ins)
        off[k] = ins[k] + 8
        assert lex_tensor(D, outs, off[0:2], off[2:4], off[4:6], kr, lr, m) == -1
    untouched("misaligned input")
    for k in range(3):  # an output row 8 bytes off
        off = list(outs)
        off[k] = outs[k] + 8
        assert lex_tensor(D, off, ins[0:2], ins[2:4], ins[4:6], kr, lr, m) == -1
    untouched("misaligned output")
    for k in range(3):  # an output that is, or reaches into, an input
        for j in range(6):
            ov = list(outs)
            ov[k] = ins[j]
            assert lex_tensor(D, ov, ins[0:2], ins[2:4], ins[4:6], kr, lr, m) == -1
            ov[k] = ins[j] + 16 * (R.n // 2)  # (half a row in)
            assert lex_tensor(D, ov, ins[0:2], ins[2:4], ins[4:6], kr, lr, m) == -1
    untouched("overlap")
    assert lex_tensor(D, outs, ins[0:2], ins[2:4], ins[4:6], kr, lr, m) == 0  # and the plain call runs
    want = exact(R, m, x, kr, lr)
    for i in range(3):
        assert_eq(D.down(outs[i], (3, R.n)), want[i], "after the declines d%d" % i)
    D.release()
