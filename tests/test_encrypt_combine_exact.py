"""sfp_encrypt_combine (kernel k_encrypt_combine) on chosen residues against Python integers
(prims.h), against the composed sfp_mul_add / sfp_mul_const / sfp_add sequence on the device
and on the oracle, out of place and in place.

    ext = 0:  out0 = v pkb + e0 + msg,              out1 = v pka + e1      (ell rows)
    ext = 1:  out0 = v pkb + e0 + k_i msg on the ell rows, v pkb + e0 on the ext row;
              out1 = v pka + e1                                            (ell + 1 rows)

Ring 2^12, ell = 3 (a 60-bit prime, one below 2^42, a 50-bit one), count = 2, a stride one row
above the rows.  The ext row is the 30-bit prime (prime index 4) and the public key keeps its
row at pk_ext_row = 4, not ell: key row 3 is never read and holds words >= q.  Rows and the
constants k are `uniform` (seeded) and `qm1` (everything q - 1: v pkb + e0 + k msg is two
products (q - 1)^2 and a q - 1 before its reductions).  In place, out0[b] / out1[b] are b's own
e0 / e1 rows.  The unmarked tests check the reference against the oracle's composed prims.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prims_harness as H  # noqa: E402
from prims_harness import Limbs, assert_eq, u64  # noqa: E402

LOGN, ELL, COUNT, EXT_PRIME, PK_ROWS = 12, 3, 2, 4, 5
FILL = 0xDEAD
JUNK = (1 << 64) - 1  # >= every prime: a word nothing may read


def primes5():
    ps = H.prime_set(LOGN)
    return [ps[0], ps[2], ps[5], ps[3], ps[1]]  # 60 | below 2^42 | 50 | above 2^42 | 30 bits


def limbs(ext):
    return Limbs(ELL + 1, ELL, EXT_PRIME, 0, 0) if ext else H.ident(ELL)


def make(R, kind, ext, seed):
    """rows as object arrays: t[b] = (v, e0, e1) and msg[b] per ciphertext, pkb / pka as
    [PK_ROWS, n] (row 3 junk), k"""
    m = limbs(ext)
    q = H.qcol(R, m)
    qm = H.qcol(R, H.ident(ELL))
    rows = m.count
    rng = np.random.default_rng(seed)

    def block(qc):
        if kind == "qm1":
            return np.broadcast_to(qc - 1, (len(qc), R.n)).copy()
        return np.stack([H.obj(rng.integers(0, int(x), R.n, dtype=np.uint64)) for x in qc.ravel()])

    t = [[block(q) for _ in range(3)] for _ in range(COUNT)]
    msg = [block(qm) for _ in range(COUNT)]
    pk = []
    for _ in range(2):
        full = np.full((PK_ROWS, R.n), JUNK, dtype=object)
        full[:ELL] = block(qm)
        full[EXT_PRIME] = block(np.array([[R.primes[EXT_PRIME]]], dtype=object))[0]
        pk.append(full)
    k = (qm - 1).ravel() if kind == "qm1" else H.obj(rng.integers(0, 1 << 62, ELL, dtype=np.uint64)) % qm.ravel()
    return m, q, rows, t, msg, pk[0], pk[1], k


def pk_rows(pk, ext):
    """the key's rows in the order of the limb map (contiguous, for the composed prims)"""
    return pk[list(range(ELL)) + ([EXT_PRIME] if ext else [])]


def exact(q, t, msg, pkb, pka, k, ext):
    out = []
    for (v, e0, e1), w in zip(t, msg):
        o0 = v * pk_rows(pkb, ext) + e0
        o0[:ELL] = o0[:ELL] + (k.reshape(-1, 1) * w if ext else w)
        out.append((o0 % q, (v * pk_rows(pka, ext) + e1) % q))
    return out


def composed(D, m, rows, n, t, msg, pkb, pka, k, ext):
    """sfp_mul_add, and for the message sfp_mul_const + sfp_add on the ell rows"""
    mi = H.ident(ELL)
    B, A = D.up(u64(pk_rows(pkb, ext))), D.up(u64(pk_rows(pka, ext)))
    out = []
    for (v, e0, e1), w in zip(t, msg):
        dv, d0, d1, dw = (D.up(u64(x)) for x in (v, e0, e1, w))
        o0, o1 = D.alloc(rows * n), D.alloc(rows * n)
        D.call("sfp_mul_add", o0, dv, B, d0, m)
        D.call("sfp_mul_add", o1, dv, A, d1, m)
        if ext:
            D.call("sfp_mul_const", dw, dw, u64(k), mi)
        D.call("sfp_add", o0, o0, dw, mi)
        out.append((D.down(o0, (rows, n)), D.down(o1, (rows, n))))
    return out


_cases = {}


def case(kind, ext):
    if (kind, ext) not in _cases:
        R = H.ring(primes5(), LOGN)
        made = make(R, kind, ext, 31 + ext)
        m, q, rows, t, msg, pkb, pka, k = made
        _cases[kind, ext] = (R,) + made + (exact(q, t, msg, pkb, pka, k, ext),)
    return _cases[kind, ext]


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("kind", ["uniform", "qm1"])
def test_reference_is_the_oracles_composed_form(oracle_lib, kind, ext):
    R, m, q, rows, t, msg, pkb, pka, k, want = case(kind, ext)
    assert [R.primes[p] for p in m.primes()] == primes5()[:ELL] + ([primes5()[EXT_PRIME]] if ext else [])
    assert R.primes[EXT_PRIME] < 1 << 30 and EXT_PRIME != ELL
    D = H.dev(oracle_lib, "oracle", R.primes, LOGN)
    for b, (g0, g1) in enumerate(composed(D, m, rows, R.n, t, msg, pkb, pka, k, ext)):
        assert_eq(g0, want[b][0], "oracle composed out0[%d] %s ext=%d" % (b, kind, ext))
        assert_eq(g1, want[b][1], "oracle composed out1[%d] %s ext=%d" % (b, kind, ext))
    D.release()


def combine(D, T, stride, msg, out0, out1, pkb, pka, ext, k):
    f = D.lib.sfp_encrypt_combine
    f.restype = C.c_int
    f.argtypes = ([C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32] + [C.c_void_p] * 5
                  + [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p])
    pm, p0, p1 = D.ptrs(msg), D.ptrs(out0), D.ptrs(out1)
    kk = u64(k)
    v = lambda a: a.ctypes.data_as(C.c_void_p)
    r = f(D.d, T, stride, COUNT, v(pm), v(p0), v(p1), pkb, pka, EXT_PRIME, ELL, ext, EXT_PRIME, v(kk) if ext else None)
    D.check()
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True], ids=["outofplace", "inplace"])
@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("kind", ["uniform", "qm1"])
def test_encrypt_combine_exact_and_composed(hip_lib, kind, ext, inplace):
    R, m, q, rows, t, msg, pkb, pka, k, want = case(kind, ext)
    D = H.dev(hip_lib, "hip", R.primes, LOGN)
    assert D.has("sfp_encrypt_combine")
    n = R.n
    stride = (rows + 1) * n  # one row above the rows
    tw = np.full((3 * COUNT, stride), FILL, dtype=np.uint64)
    for b in range(COUNT):
        for i in range(3):
            tw[3 * b + i, :rows * n] = u64(t[b][i]).ravel()
    T = D.up(tw)
    dm = [D.up(u64(w)) for w in msg]
    B, A = D.up(u64(pkb)), D.up(u64(pka))
    if inplace:
        out0 = [T + 8 * (3 * b + 1) * stride for b in range(COUNT)]
        out1 = [T + 8 * (3 * b + 2) * stride for b in range(COUNT)]
    else:
        out0 = [D.alloc(stride, fill=FILL) for _ in range(COUNT)]
        out1 = [D.alloc(stride, fill=FILL) for _ in range(COUNT)]
    assert combine(D, T, stride, dm, out0, out1, B, A, ext, k) == 0
    comp = composed(D, m, rows, n, t, msg, pkb, pka, k, ext)
    for b in range(COUNT):
        for i, p in enumerate((out0[b], out1[b])):
            got = D.down(p, (stride,))
            tag = "out%d[%d] %s ext=%d" % (i, b, kind, ext)
            assert_eq(got[:rows * n].reshape(rows, n), want[b][i], "encrypt_combine " + tag)
            assert (got[rows * n:] == FILL).all(), tag + ": wrote past its rows"
            assert np.array_equal(got[:rows * n].reshape(rows, n), comp[b][i]), tag + ": differs from the composed prims"
    after = D.down(T, (3 * COUNT, stride))
    keep = [3 * b for b in range(COUNT)] + ([] if inplace else [3 * b + i for b in range(COUNT) for i in (1, 2)])
    assert np.array_equal(after[keep], tw[keep]), "an input row set was written"
    assert np.array_equal(D.down(B, (PK_ROWS, n)), u64(pkb)) and np.array_equal(D.down(dm[0], (ELL, n)), u64(msg[0]))
    D.release()
