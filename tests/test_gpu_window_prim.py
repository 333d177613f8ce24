"""sfp_weight_tensor_cols (kernels k_weight_tensor_cols<1> and <2>: the window sums' weighted
column sums before their relinearisation, prims.h) on chosen residues against Python integers,
against the composed generic primitives on the device and on the oracle, and its decline cases.

    a_b0 = p_b + v_b0 (mod q, canonical), a_b1 = v_b1
    d0_c = sum_b a_b0 u_bc0,  d1_c = sum_b (a_b0 u_bc1 + a_b1 u_bc0),  d2_c = sum_b a_b1 u_bc1   (mod each prime)

Ring 2^12 with l = 3 (a 60-bit, a 30-bit and an FP64-range prime) and l = SFP_MAX_LIMBS = 96
(48 primes, each twice, as tests/test_gpu_lex_prim.py).  Batches and columns: B in {1, 2, 16}
with one column (kernel <1>), and (B, C) = (1, 2) and (16, 2) (kernel <2>).  Residues:
  qm1      every row q - 1;
  zero     everything 0;
  uniform  seeded random residues;
  wrap     p = q - 1 and v0 = q - 1, the rest seeded: a0 = q - 2 takes the modular add's
           conditional subtraction;
  bound    B = 16, p = q - 1, v0 = 0, v1 = q - 1, every u word q - 1: a0 = a1 = q - 1 and d1 is 32
           products (q - 1)^2 -- the stated 2^125 bound of the 128-bit accumulator on the primes
           just below 2^60.
The fused outputs are compared word for word with the composed prims' on both backends, and all
of them with Python integers on 256 columns of every limb (both ends and seeded random ones; the
constant kinds' rows are constant along a limb, so those columns are every distinct value).
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
from test_gpu_group_prim import FILL, sample_columns  # noqa: E402
from test_gpu_lex_prim import LOGN, MAX_LIMBS, limb_maps, primes48  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_B = 16  # prims.h SFP_WEIGHT_MAX_B
MAX_C = 8  # prims.h SFP_WEIGHT_MAX_C
SHAPES = [(1, 1), (2, 1), (16, 1), (1, 2), (16, 2)]  # (B, C)


@pytest.fixture(scope="module")
def devs(hip_lib, oracle_lib):
    pr = primes48()
    return H.ring(pr, LOGN), H.dev(hip_lib, "hip", pr, LOGN), H.dev(oracle_lib, "oracle", pr, LOGN)


def weight_tensor(D, d, v, p, u, nb, nc, m):
    """d = (d0[nc], d1[nc], d2[nc]), v = (v0[nb], v1[nb]), p[nb], u = (u0[nc * nb], u1[nc * nb]), column major"""
    f = D.lib.sfp_weight_tensor_cols
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 9 + [C.c_uint32, C.c_uint32, Limbs]
    arrays = [D.ptrs(x) for x in (*d, *v, p, *u)]  # host arrays of device pointers
    r = f(D.d, *[a.ctypes.data_as(C.c_void_p) for a in arrays], nb, nc, m)
    D.check()
    return r


def rows(R, m, kind, nb, nc, seed):
    """v0[nb], v1[nb], p[nb], u0[nc][nb], u1[nc][nb] ([count, n] uint64 arrays)"""
    P = np.array([R.primes[p] for p in m.primes()], dtype=object)
    full = lambda v: np.broadcast_to(u64(v).reshape(-1, 1), (m.count, R.n)).copy()
    grid = lambda f: [[f() for _ in range(nb)] for _ in range(nc)]
    if kind == "qm1":
        x = full(P - 1)
        return [x] * nb, [x] * nb, [x] * nb, grid(lambda: x), grid(lambda: x)
    if kind == "zero":
        x = full(P * 0)
        return [x] * nb, [x] * nb, [x] * nb, grid(lambda: x), grid(lambda: x)
    if kind == "bound":
        x = full(P - 1)
        return [full(P * 0)] * nb, [x] * nb, [x] * nb, grid(lambda: x), grid(lambda: x)
    rng = np.random.default_rng(seed)
    col = u64(P).reshape(-1, 1)
    rand = lambda: rng.integers(0, 1 << 63, (m.count, R.n), dtype=np.uint64) % col
    if kind == "wrap":
        x = full(P - 1)
        return [x] * nb, [rand() for _ in range(nb)], [x] * nb, grid(rand), grid(rand)
    return [rand() for _ in range(nb)], [rand() for _ in range(nb)], [rand() for _ in range(nb)], grid(rand), grid(rand)


def exact(R, m, v0, v1, p, u0, u1, cols, kind=None):
    """[(d0, d1, d2) per column] on the sampled columns, in Python integers"""
    P = np.array([R.primes[q] for q in m.primes()], dtype=object).reshape(-1, 1)
    o = lambda x: H.obj(x[:, cols])
    a0 = [(o(x) + o(w)) % P for x, w in zip(v0, p)]
    a1 = [o(x) for x in v1]
    if kind == "wrap":
        assert all(np.array_equal(a, np.broadcast_to(P - 2, a.shape)) for a in a0)
    out = []
    for c in range(len(u0)):
        y0, y1 = [o(x) for x in u0[c]], [o(x) for x in u1[c]]
        d0 = sum(a * y for a, y in zip(a0, y0))
        d1 = sum(a * y for a, y in zip(a0, y1)) + sum(a * y for a, y in zip(a1, y0))
        d2 = sum(a * y for a, y in zip(a1, y1))
        assert int(np.max(d1)) < 1 << 125  # the stated bound of the one 128-bit reduction
        out.append((d0 % P, d1 % P, d2 % P))
    return out


def composed(D, v0, v1, p, u0, u1, m, words):
    """the same integers from the generic prims (the engine's composed path); [(d0, d1, d2)]"""
    nb, nc = len(v0), len(u0)
    a0, t0, t1, t2 = (D.alloc(words) for _ in range(4))
    d = [tuple(D.alloc(words) for _ in range(3)) for _ in range(nc)]
    for b in range(nb):
        D.call("sfp_add", a0, v0[b], p[b], m)
        for c in range(nc):
            if b == 0:
                D.call("sfp_tensor", d[c][0], d[c][1], d[c][2], a0, v1[0], u0[c][0], u1[c][0], m)
                continue
            D.call("sfp_tensor", t0, t1, t2, a0, v1[b], u0[c][b], u1[c][b], m)
            for k, t in enumerate((t0, t1, t2)):
                D.call("sfp_add", d[c][k], d[c][k], t, m)
    return d


def run_case(devs, ell, kind, nb, nc):
    R, hip, oracle = devs
    assert hip.has("sfp_weight_tensor_cols") and not oracle.has("sfp_weight_tensor_cols")
    m = limb_maps()[ell]
    v0, v1, p, u0, u1 = rows(R, m, kind, nb, nc, 20251205 + ell + 100 * nb + nc)
    cols = sample_columns(R.n)
    want = exact(R, m, v0, v1, p, u0, u1, cols, kind)
    if kind == "bound":  # 32 products (q - 1)^2 on a prime just below 2^60
        assert nb == MAX_B and max(R.primes[q] for q in m.primes()) > (1 << 60) - (1 << 40)
    shape, words = (m.count, R.n), m.count * R.n
    got_c = {}
    for D in (hip, oracle):
        tag = "hip" if D is hip else "oracle"
        up = {}  # (rows the kinds share are uploaded once)
        dev = lambda x: up.setdefault(id(x), D.up(x))
        dv0, dv1, dp = [dev(x) for x in v0], [dev(x) for x in v1], [dev(x) for x in p]
        du0, du1 = [[dev(x) for x in col] for col in u0], [[dev(x) for x in col] for col in u1]
        got_c[tag] = [[D.down(x, shape) for x in dc] for dc in composed(D, dv0, dv1, dp, du0, du1, m, words)]
        for c in range(nc):
            for i in range(3):
                assert_eq(got_c[tag][c][i][:, cols], want[c][i], f"composed d{i}[{c}] {kind} l={ell} B={nb} {tag}")
        if D is hip:
            d = [[D.alloc(words, fill=FILL) for _ in range(nc)] for _ in range(3)]
            flat = lambda g: [x for col in g for x in col]
            assert weight_tensor(D, d, (dv0, dv1), dp, (flat(du0), flat(du1)), nb, nc, m) == 0
            for c in range(nc):
                for i in range(3):
                    got = D.down(d[i][c], shape)
                    assert_eq(got[:, cols], want[c][i], f"weight_tensor d{i}[{c}] {kind} l={ell} B={nb}")
                    assert np.array_equal(got, got_c[tag][c][i]), f"fused != composed d{i}[{c}] {kind} l={ell} B={nb}"
        D.release()
    for c in range(nc):
        for i in range(3):
            assert np.array_equal(got_c["hip"][c][i], got_c["oracle"][c][i])


@pytest.mark.parametrize("kind", ["qm1", "zero", "uniform", "wrap"])
@pytest.mark.parametrize("nb,nc", SHAPES)
@pytest.mark.parametrize("ell", [3, MAX_LIMBS])
def test_weight_tensor_exact_and_composed(devs, ell, nb, nc, kind):
    run_case(devs, ell, kind, nb, nc)


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("ell", [3, MAX_LIMBS])
def test_weight_tensor_bound(devs, ell, nc):
    run_case(devs, ell, "bound", MAX_B, nc)


def test_weight_tensor_three_columns(devs):
    """C = 3 in one call: a tile of two and a remainder of one"""
    run_case(devs, 3, "uniform", 2, 3)


def test_weight_tensor_declines(devs):
    """-1 with nothing written: B = 0 and B = 17, C = 0 and C = 9, more than SFP_MAX_LIMBS rows, a
    row off 16-byte alignment, an output overlapping an input or another output."""
    R, hip, _ = devs
    D = hip
    big = Limbs(MAX_LIMBS + 1, 48, 0, 0, 0)  # 48 + 49 rows: one row too many
    m = H.ident(3)
    nb, nc = 2, 2
    v0, v1, p, u0, u1 = rows(R, m, "uniform", nb, nc, 5)
    words = (MAX_LIMBS + 1) * R.n

    def buf(x):
        b = D.alloc(words + 2, fill=1)
        D.put(b, x)
        return b

    dv = ([buf(x) for x in v0], [buf(x) for x in v1])
    dp = [buf(x) for x in p]
    du = ([buf(x) for col in u0 for x in col], [buf(x) for col in u1 for x in col])
    ins = dv[0] + dv[1] + dp + du[0] + du[1]
    outs = [[D.alloc(words + 2, fill=FILL) for _ in range(nc)] for _ in range(3)]

    def untouched(what):
        for g in outs:
            for x in g:
                assert (D.down(x, (words + 2,)) == FILL).all(), what + ": an output was written"
        assert np.array_equal(D.down(ins[0], (3, R.n)), v0[0]), what + ": an input was written"

    def call(d=outs, v=dv, w=dp, u=du, b=nb, c=nc, mm=m):
        return weight_tensor(D, d, v, w, u, b, c, mm)

    assert call(mm=big) == -1
    untouched("too many rows")
    v17 = ([dv[0][0]] * (MAX_B + 1), [dv[1][0]] * (MAX_B + 1))
    u17 = ([du[0][0]] * (MAX_B + 1) * nc, [du[1][0]] * (MAX_B + 1) * nc)
    assert call(v=v17, w=[dp[0]] * (MAX_B + 1), u=u17, b=MAX_B + 1) == -1
    assert call(b=0) == -1
    untouched("batch count")
    d9 = [[g[0]] * (MAX_C + 1) for g in outs]
    u9 = ([du[0][0]] * nb * (MAX_C + 1), [du[1][0]] * nb * (MAX_C + 1))
    assert call(d=d9, u=u9, c=MAX_C + 1) == -1
    assert call(c=0) == -1
    untouched("column count")

    def shifted(groups, g, k, by):
        out = [list(x) for x in groups]
        out[g][k] = by
        return out

    for g in range(2):  # an input row 8 bytes off
        for k in range(nb):
            assert call(v=shifted(dv, g, k, dv[g][k] + 8)) == -1
        for k in range(nb * nc):
            assert call(u=shifted(du, g, k, du[g][k] + 8)) == -1
    for k in range(nb):
        assert call(w=shifted([dp], 0, k, dp[k] + 8)[0]) == -1
    untouched("misaligned input")
    for g in range(3):  # an output row 8 bytes off
        for k in range(nc):
            assert call(d=shifted(outs, g, k, outs[g][k] + 8)) == -1
    untouched("misaligned output")
    for g in range(3):  # an output that is, or reaches into, an input or another output
        for k in range(nc):
            for x in ins:
                assert call(d=shifted(outs, g, k, x)) == -1
                assert call(d=shifted(outs, g, k, x + 16 * (R.n // 2))) == -1  # (half a row in)
            other = outs[(g + 1) % 3][k]
            assert call(d=shifted(outs, g, k, other)) == -1
    untouched("overlap")
    assert call() == 0  # and the plain call runs
    cols = sample_columns(R.n)
    want = exact(R, m, v0, v1, p, u0, u1, cols)
    for c in range(nc):
        for i in range(3):
            assert_eq(D.down(outs[i][c], (3, R.n))[:, cols], want[c][i], "after the declines d%d[%d]" % (i, c))
    D.release()
