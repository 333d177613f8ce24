"""sfp_or_tensor (kernel k_or_tensor: the OR of two gates before its relinearisation, prims.h)
on chosen residues against Python integers, against the composed generic primitives on the device
and on the oracle, and its three decline cases.

    na0 = -a0, na1 = -a1
    d0 = kb a0 + ka b0 + na0 b0,  d1 = kb a1 + ka b1 + na0 b1 + na1 b0,  d2 = na1 b1    (mod each limb's prime)

Ring 2^12 with l = 3 (a 60-bit, a 30-bit and an FP64-range prime) and l = SFP_MAX_LIMBS = 96
(48 primes, each twice: the doubled map the engine uses for [c0 rows][c1 rows]).  Residues:
  qm1      every row and both constants q - 1;
  zero     everything 0;
  bound    ka = kb = q - 1, a0 = a1 = 1 (na = q - 1), b0 = b1 = q - 1: d1 is 3 (q - 1)^2 + (q - 1)
           -- against the stated 2^122 bound of the 128-bit accumulator on the primes just below
           2^60;
  uniform  seeded random residues and constants, ka != kb.
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
from test_gpu_lex_prim import FILL, LOGN, MAX_LIMBS, limb_maps, primes48  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devs(hip_lib, oracle_lib):
    pr = primes48()
    return H.ring(pr, LOGN), H.dev(hip_lib, "hip", pr, LOGN), H.dev(oracle_lib, "oracle", pr, LOGN)


def or_tensor(D, d, a, b, ka, kb, m):
    f = D.lib.sfp_or_tensor
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 10 + [Limbs]
    ka, kb = u64(ka), u64(kb)
    r = f(D.d, d[0], d[1], d[2], a[0], a[1], b[0], b[1], ka.ctypes.data_as(C.c_void_p),
          kb.ctypes.data_as(C.c_void_p), m)
    D.check()
    return r


def rows(R, m, kind, seed):
    """four rows a0 a1 b0 b1 ([count, n] object arrays) and the constants ka, kb"""
    P = np.array([R.primes[p] for p in m.primes()], dtype=object)
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=object).reshape(-1, 1), (m.count, R.n)).copy()
    if kind == "qm1":
        return [full(P - 1) for _ in range(4)], P - 1, P - 1
    if kind == "zero":
        return [full(P * 0) for _ in range(4)], P * 0, P * 0
    if kind == "bound":
        one, x = full(P * 0 + 1), full(P - 1)
        return [one, one, x, x], P - 1, P - 1
    rng = np.random.default_rng(seed)
    rand = lambda: np.stack([H.obj(rng.integers(0, int(p), R.n, dtype=np.uint64)) for p in P])
    out = [rand() for _ in range(4)]
    const = lambda: H.obj(rng.integers(0, 1 << 62, m.count, dtype=np.uint64)) % P
    return out, const(), const()


def exact(R, m, x, ka, kb):
    P = np.array([R.primes[p] for p in m.primes()], dtype=object).reshape(-1, 1)
    a0, a1, b0, b1 = x
    ka, kb = ka.reshape(-1, 1), kb.reshape(-1, 1)
    n0, n1 = (-a0) % P, (-a1) % P
    d1 = kb * a1 + ka * b1 + n0 * b1 + n1 * b0
    assert int(np.max(d1)) < 1 << 122  # the stated bound of the one 128-bit reduction
    return (kb * a0 + ka * b0 + n0 * b0) % P, d1 % P, n1 * b1 % P, d1


def composed(D, dp, ka, kb, m, words):
    """the same integers from the generic prims (the engine's composed path): 11 launches"""
    a0, a1, b0, b1 = dp
    n0, n1, l0, l1, d0, d1, d2 = (D.alloc(words) for _ in range(7))
    D.call("sfp_neg", n0, a0, m)
    D.call("sfp_neg", n1, a1, m)
    D.call("sfp_tensor", d0, d1, d2, n0, n1, b0, b1, m)
    D.call("sfp_mul_const", l0, a0, u64(kb), m)
    D.call("sfp_mul_const", l1, a1, u64(kb), m)
    D.call("sfp_add", d0, d0, l0, m)
    D.call("sfp_add", d1, d1, l1, m)
    D.call("sfp_mul_const", l0, b0, u64(ka), m)
    D.call("sfp_mul_const", l1, b1, u64(ka), m)
    D.call("sfp_add", d0, d0, l0, m)
    D.call("sfp_add", d1, d1, l1, m)
    return d0, d1, d2


@pytest.mark.parametrize("kind", ["qm1", "zero", "bound", "uniform"])
@pytest.mark.parametrize("ell", [3, MAX_LIMBS])
def test_or_tensor_exact_and_composed(devs, ell, kind):
    R, hip, oracle = devs
    assert hip.has("sfp_or_tensor") and not oracle.has("sfp_or_tensor")
    m = limb_maps()[ell]
    x, ka, kb = rows(R, m, kind, 20251205 + ell)
    *want, d1 = exact(R, m, x, ka, kb)
    if kind == "bound":  # 3 (q - 1)^2 + (q - 1) on a prime just below 2^60
        qmax = max(R.primes[p] for p in m.primes())
        assert qmax > (1 << 60) - (1 << 40) and int(np.max(d1)) == 3 * (qmax - 1) ** 2 + (qmax - 1)
    if kind == "uniform":
        assert all(int(s) != int(t) for s, t in zip(ka, kb))  # distinct ka != kb
    shape, words = (m.count, R.n), m.count * R.n
    for D in (hip, oracle):
        dp = [D.up(u64(r)) for r in x]
        c = composed(D, dp, ka, kb, m, words)
        got_c = [D.down(p, shape) for p in c]
        for i in range(3):
            assert_eq(got_c[i], want[i], "composed d%d %s l=%d %s" % (i, kind, ell, D is hip and "hip" or "oracle"))
        if D is hip:
            d = [D.alloc(words, fill=FILL) for _ in range(3)]
            assert or_tensor(D, d, dp[0:2], dp[2:4], ka, kb, m) == 0
            for i in range(3):
                got = D.down(d[i], shape)
                assert_eq(got, want[i], "or_tensor d%d %s l=%d" % (i, kind, ell))
                assert np.array_equal(got, got_c[i])
        D.release()


def test_or_tensor_swapped_constants_differ(devs):
    """ka multiplies b and kb multiplies a: swapping them changes d0 and d1, not d2."""
    R, hip, _ = devs
    m = H.ident(3)
    x, ka, kb = rows(R, m, "uniform", 7)
    shape, words = (m.count, R.n), m.count * R.n
    dp = [hip.up(u64(r)) for r in x]
    d = [hip.alloc(words, fill=FILL) for _ in range(3)]
    assert or_tensor(hip, d, dp[0:2], dp[2:4], kb, ka, m) == 0
    *want, _ = exact(R, m, x, kb, ka)
    *other, _ = exact(R, m, x, ka, kb)
    for i in range(3):
        assert_eq(hip.down(d[i], shape), want[i], "swapped constants d%d" % i)
    assert not np.array_equal(want[0], other[0]) and not np.array_equal(want[1], other[1])
    assert np.array_equal(want[2], other[2])
    hip.release()


def test_or_tensor_declines(devs):
    """-1 with nothing written: more than SFP_MAX_LIMBS rows, a row off 16-byte alignment, an
    output overlapping an input or another output."""
    R, hip, _ = devs
    D = hip
    big = Limbs(MAX_LIMBS + 1, 48, 0, 0, 0)  # 48 + 49 rows: one row too many
    m = H.ident(3)
    x, ka, kb = rows(R, m, "uniform", 5)
    words = (MAX_LIMBS + 1) * R.n
    ins = [D.alloc(words + 2, fill=1) for _ in range(4)]
    for p, r in zip(ins, x):
        D.put(p, u64(r))
    outs = [D.alloc(words + 2, fill=FILL) for _ in range(3)]
    kbig = np.ones(MAX_LIMBS + 1, dtype=object)

    def untouched(what):
        for p in outs:
            assert (D.down(p, (words + 2,)) == FILL).all(), what + ": an output was written"
        for p, r in zip(ins, x):
            assert np.array_equal(D.down(p, (3, R.n)), u64(r)), what + ": an input was written"

    assert or_tensor(D, outs, ins[0:2], ins[2:4], kbig, kbig, big) == -1
    untouched("too many rows")
    for k in range(4):  # an input row 8 bytes off
        off = list(ins)
        off[k] = ins[k] + 8
        assert or_tensor(D, outs, off[0:2], off[2:4], ka, kb, m) == -1
    untouched("misaligned input")
    for k in range(3):  # an output row 8 bytes off
        off = list(outs)
        off[k] = outs[k] + 8
        assert or_tensor(D, off, ins[0:2], ins[2:4], ka, kb, m) == -1
    untouched("misaligned output")
    for k in range(3):  # an output that is, or reaches into, an input
        for j in range(4):
            ov = list(outs)
            ov[k] = ins[j]
            assert or_tensor(D, ov, ins[0:2], ins[2:4], ka, kb, m) == -1
            ov[k] = ins[j] + 16 * (R.n // 2)  # (half a row in)
            assert or_tensor(D, ov, ins[0:2], ins[2:4], ka, kb, m) == -1
    untouched("output over input")
    for k in range(3):  # an output that is, or reaches into, another output
        for j in range(3):
            if j == k:
                continue
            ov = list(outs)
            ov[k] = outs[j]
            assert or_tensor(D, ov, ins[0:2], ins[2:4], ka, kb, m) == -1
            ov[k] = outs[j] + 16 * (R.n // 2)
            assert or_tensor(D, ov, ins[0:2], ins[2:4], ka, kb, m) == -1
    untouched("output over output")
    assert or_tensor(D, outs, ins[0:2], ins[2:4], ka, kb, m) == 0  # and the plain call runs
    *want, _ = exact(R, m, x, ka, kb)
    for i in range(3):
        assert_eq(D.down(outs[i], (3, R.n)), want[i], "after the declines d%d" % i)
    D.release()
