"""The case table of the primitive-level differential tests (prims_harness.py).

Every case takes `devs`: a function (primes, logn) -> [Dev, ...] of the libraries
under test (the oracle alone on the CPU; HIP and the oracle on the GPU), runs the
primitive on each on chosen residues and asserts integer equality with the exact
reference -- so two libraries that pass agree with each other as well.  Prims
only the HIP library has (weak symbols) are checked where present.
"""
import random

import numpy as np

import prims_harness as H
from prims_harness import Limbs, assert_eq, ident, obj, u64

LOGN = 12  # the smallest ring with two-pass NTT kernels (n = 2^11 is one k_ntt_small tile)


def maps9():
    """Identity | stride 2 from prime 1 (1, 3, 5, 7) | split/pbase (0, 1, then 6, 7, 8)."""
    return {"ident": ident(9), "stride": Limbs(4, 4, 0, 1, 2), "split": Limbs(5, 2, 6, 0, 0)}


def setup(devs, logn=LOGN, primes=None):
    primes = primes or H.prime_set(logn)
    return H.ring(primes, logn), devs(primes, logn)


# ---- 8. loading and sampling ---------------------------------------------------

def load_values(R):
    v = [0, 1, -1, 1 << 62, -(1 << 62), (1 << 63) - 1, -(1 << 63)]
    for q in R.primes:
        v += [q - 1, -(q - 1), q, -q]
    rng = random.Random(5)
    v += [rng.randrange(-(1 << 63), 1 << 63) for _ in range(R.n - len(v))]
    return v


def case_load_i64(devs, logn=11):
    R, Ds = setup(devs, logn)
    vals = load_values(R)
    c = np.array(vals, dtype=np.int64)
    for name, m in maps9().items():
        want = np.array([[v % R.primes[p] for v in vals] for p in m.primes()], dtype=object)
        for D in Ds:
            p = D.alloc(m.count * R.n)
            D.call("sfp_load_i64", p, c, m)
            assert_eq(D.down(p, (m.count, R.n)), want, "load_i64 %s" % name)
            D.release()


def case_sample_uniform(devs, logn=11):
    R, Ds = setup(devs, logn)
    for name, m in maps9().items():
        for seed in (0, 0xFFFFFFFFFFFFFFFF, 20251205):
            want = H.exact_uniform(R, m, seed)
            for D in Ds:
                p = D.alloc(m.count * R.n)
                D.call("sfp_sample_uniform", p, m, seed)
                assert_eq(D.down(p, (m.count, R.n)), want, "sample_uniform %s seed %d" % (name, seed))
                D.release()


def case_sample_small(devs, logn=11):
    """Weak: the libraries that have it (HIP)."""
    R, Ds = setup(devs, logn)
    ran = 0
    for name, m in maps9().items():
        seeds, kinds = [3, (1 << 64) - 5, 77], [0, 1, 1]
        stride = m.count * R.n + 2 * R.n  # larger than the rows
        for D in Ds:
            if not D.has("sfp_sample_small"):
                continue
            p = D.alloc(3 * stride, fill=0xDEAD)
            assert D.call("sfp_sample_small", p, stride, 3, u64(seeds), np.array(kinds, dtype=np.uint32), m) == 0
            got = D.down(p, (3, stride))
            for j in range(3):
                assert_eq(got[j, :m.count * R.n].reshape(m.count, R.n), H.exact_small(R, m, seeds[j], kinds[j]),
                          "sample_small %s poly %d" % (name, j))
                assert (got[j, m.count * R.n:] == 0xDEAD).all(), "sample_small wrote past its rows"
            D.release()
            ran += 1
    return ran


# ---- 2. element-wise and tensor -----------------------------------------------

def case_elementwise(devs, mapname, logn=LOGN):
    R, Ds = setup(devs, logn)
    m = maps9()[mapname]
    q = H.qcol(R, m)
    P = H.pattern_polys(R, m)
    names = list(P)
    rng = random.Random(11)
    kc = np.array([[R.primes[p] - 1, rng.randrange(R.primes[p])][i % 2] for i, p in enumerate(m.primes())],
                  dtype=object)
    shape = (m.count, R.n)
    for D in Ds:
        dp = {k: D.up(u64(P[k])) for k in names}
        o = [D.alloc(m.count * R.n) for _ in range(3)]
        for i, an in enumerate(names):
            # every pattern against itself, against the next one and against all-(q-1)
            for bn in (an, names[(i + 1) % len(names)], "qm1"):
                a, b, c = P[an], P[bn], P[names[(i + 2) % len(names)]]
                A, B, Cc = dp[an], dp[bn], dp[names[(i + 2) % len(names)]]
                tag = "%s (%s, %s)" % (mapname, an, bn)
                D.call("sfp_add", o[0], A, B, m)
                assert_eq(D.down(o[0], shape), (a + b) % q, "add " + tag)
                D.call("sfp_sub", o[0], A, B, m)
                assert_eq(D.down(o[0], shape), (a - b) % q, "sub " + tag)
                D.call("sfp_mul", o[0], A, B, m)
                assert_eq(D.down(o[0], shape), a * b % q, "mul " + tag)
                D.call("sfp_mul_add", o[0], A, B, Cc, m)
                assert_eq(D.down(o[0], shape), (a * b + c) % q, "mul_add " + tag)
                D.call("sfp_tensor", o[0], o[1], o[2], A, B, Cc, A, m)  # (a0, a1) = (a, b), (b0, b1) = (c, a)
                assert_eq(D.down(o[0], shape), a * c % q, "tensor d0 " + tag)
                assert_eq(D.down(o[1], shape), (a * a + b * c) % q, "tensor d1 " + tag)
                assert_eq(D.down(o[2], shape), b * a % q, "tensor d2 " + tag)
                if D.has("sfp_tie_tensor"):  # s = (a, b), w = c: u = (c a + k, c b)
                    assert D.call("sfp_tie_tensor", o[0], o[1], o[2], A, B, Cc, u64(kc), m) == 0
                    u0, u1 = (a * c + kc.reshape(-1, 1)) % q, b * c % q
                    assert_eq(D.down(o[0], shape), a * u0 % q, "tie_tensor d0 " + tag)
                    assert_eq(D.down(o[1], shape), (a * u1 + b * u0) % q, "tie_tensor d1 " + tag)
                    assert_eq(D.down(o[2], shape), b * u1 % q, "tie_tensor d2 " + tag)
            a, A = P[an], dp[an]
            D.call("sfp_neg", o[0], A, m)
            assert_eq(D.down(o[0], shape), (-a) % q, "neg %s %s" % (mapname, an))
            D.call("sfp_mul_const", o[0], A, u64(kc), m)
            assert_eq(D.down(o[0], shape), a * kc.reshape(-1, 1) % q, "mul_const %s %s" % (mapname, an))
            D.call("sfp_add_const", o[0], A, u64(kc), m)
            assert_eq(D.down(o[0], shape), (a + kc.reshape(-1, 1)) % q, "add_const %s %s" % (mapname, an))
        D.release()


# ---- 1. NTT -----------------------------------------------------------------------

_ntt_ref = {}


def forward_rows(R, m):
    """fwd1 / fwd2: per limb, the coefficient row that drives FP64 forward pass 1 / 2 hardest
    in the lazy model (Ring.fwd_aligned)."""
    if R.fwd_split() == 0:
        return {}
    return {"fwd%d" % w: np.stack([R.fwd_aligned(p, w) for p in m.primes()]) for w in (1, 2)}


def case_forward_pass_model(logn, p=2):
    """The model of the forward FP64 passes (Ring.fwd_pass_model) on the prime just below
    2^42.  Modelled max |v| / q inside (pass 1, pass 2), kernel's stated bound 19 q:

        row       n = 2^12 (4 + 8 stages)   n = 2^16 (8 + 8)    n = 2^17 (9 + 8)
        uniform   2.358  3.432              3.773  3.842        4.252  4.182
        qm1       2.211  3.212              3.346  3.903        3.751  3.817
        alt1      2.211  3.212              3.346  3.903        3.751  3.817
        alt0      2.211  2.865              3.346  3.770        3.751  3.500
        half      1.518  3.113              2.343  3.728        2.529  4.033
        fwd1      2.984  3.553              4.969  3.825        5.465  3.869
        fwd2      2.085  4.969              3.599  4.969        3.449  4.969

    fwd1 / fwd2 reach q - 1 + d h, h = 0.496 q, in their pass of d stages: the ceiling of a
    butterfly whose product is a centred residue is (1 + d / 2) q, 5.5 q for the longest pass,
    so the stated 19 q (2 q a stage) cannot be approached by any input; the rows push each
    pass as far as the arithmetic goes.  The figures record that; the one condition is that
    each aligned row exceeds the uniform row in its pass.  Returns the table's column."""
    R = H.ring(H.prime_set(logn) if logn == LOGN else H.small_prime_set(logn), logn)
    q = R.primes[p]
    assert q < H.FP_BOUND
    pat = H.patterns(R, q, 7)
    rows = {k: pat[k] for k in ("uniform", "qm1", "alt1", "alt0", "half")}
    rows["fwd1"], rows["fwd2"] = R.fwd_aligned(p, 1), R.fwd_aligned(p, 2)
    got = {k: R.fwd_pass_model(a, p) for k, a in rows.items()}
    d = (R.fwd_split(), logn - R.fwd_split())
    for w in (0, 1):
        assert got["fwd%d" % (w + 1)][w] > got["uniform"][w], (logn, w, got)
        assert got["fwd%d" % (w + 1)][w] == max(g[w] for g in got.values())
        assert got["fwd%d" % (w + 1)][w] > 1 + 0.49 * d[w]
    return got


def ntt_reference(R, m, seed=7):
    """name -> (coefficient poly, its exact forward NTT, its exact inverse NTT), shared by the NTT cases."""
    key = (id(R), tuple(m.primes()), seed)
    if key not in _ntt_ref:
        P = dict(H.pattern_polys(R, m, seed), **forward_rows(R, m))
        _ntt_ref[key] = {k: (a, H.exact_rows(R, m, a, R.ntt), H.exact_rows(R, m, a, R.intt)) for k, a in P.items()}
    return _ntt_ref[key]


def case_reference_ntt_definition(logn=LOGN):
    """The fast exact NTT against the definition, evaluated directly at the border indices."""
    R = H.ring(H.prime_set(logn), logn)
    ref = ntt_reference(R, ident(9))
    for name in ("uniform", "alt1", "qm1"):
        a, f, inv = ref[name]
        for p in (0, 1, 2, 3):
            for k in R.border_indices():
                assert int(f[p][k]) == R.ntt_at(a[p], p, k), ("ntt", name, p, k)
                assert int(inv[p][k]) == R.intt_at(a[p], p, k), ("intt", name, p, k)


def case_ntt(devs, mapname, logn=LOGN):
    """sfp_ntt of one polynomial per pattern: forward, inverse, round trip (at most 9 rows a launch)."""
    R, Ds = setup(devs, logn)
    m = maps9()[mapname]
    ref = ntt_reference(R, m)
    shape = (m.count, R.n)
    for D in Ds:
        for name, (a, f, inv) in ref.items():
            p = D.up(u64(a))
            D.call("sfp_ntt", p, m, 0)
            assert_eq(D.down(p, shape), f, "ntt forward %s %s" % (mapname, name))
            D.call("sfp_ntt", p, m, 1)
            assert_eq(D.down(p, shape), a, "ntt round trip %s %s" % (mapname, name))
            D.call("sfp_ntt", p, m, 1)
            assert_eq(D.down(p, shape), inv, "ntt inverse %s %s" % (mapname, name))
            D.release()


def case_ntt_batch(devs, count, limbs, logn=LOGN):
    """sfp_ntt_batch of `count` polynomials (pattern b mod #patterns in polynomial b) with a
    stride above the rows; count * limbs rows in one launch."""
    R, Ds = setup(devs, logn)
    m = ident(limbs)
    ref = ntt_reference(R, m)
    names = list(ref)
    pad = 0 if count > 64 else R.n  # (the 128 MiB launch is packed)
    stride = limbs * R.n + pad
    src = np.stack([u64(ref[k][0]) for k in names])
    fwd = np.stack([u64(ref[k][1]) for k in names])
    inv = np.stack([u64(ref[k][2]) for k in names])
    sel = np.arange(count) % len(names)

    def lay(x):
        buf = np.full((count, stride), 0xABCD, dtype=np.uint64)
        buf[:, :limbs * R.n] = x[sel].reshape(count, -1)
        return buf

    for D in Ds:
        for inverse, want in ((0, fwd), (1, inv)):
            p = D.up(lay(src))
            D.call("sfp_ntt_batch", p, stride, count, m, inverse)
            got = D.down(p, (count, stride))
            assert np.array_equal(got, lay(want)), "ntt_batch inverse=%d: %d rows differ" % (
                inverse, int((got != lay(want)).any(axis=1).sum()))
            D.call("sfp_ntt_batch", p, stride, count, m, 1 - inverse)
            assert np.array_equal(D.down(p, (count, stride)), lay(src)), "ntt_batch round trip"
            D.release()


def case_ntt_large(devs, logn, names=("uniform", "qm1", "alt0")):
    """Rings 2^16 / 2^17: four rows (60 bits, 30 bits, either side of 2^42).  The full exact
    transform of several rows is slow at these sizes: every library is checked against the
    definition, evaluated directly, at the border indices (all of them on the uniform row),
    its round trip against the input on every output, and the libraries against each other
    on every output."""
    R, Ds = setup(devs, logn, H.small_prime_set(logn))
    m = ident(4)
    P = dict(H.pattern_polys(R, m), **forward_rows(R, m))
    for name in names:
        a = P[name]
        idx = R.border_indices()[:: 1 if name == "uniform" else 4]
        want = {(d, p, k): (R.intt_at if d else R.ntt_at)(a[p], p, k) for d in (0, 1) for p in range(4) for k in idx}
        outs = []
        for D in Ds:
            p = D.up(u64(a))
            D.call("sfp_ntt", p, m, 0)
            f = D.down(p, (4, R.n))
            D.call("sfp_ntt", p, m, 1)
            assert_eq(D.down(p, (4, R.n)), a, "ntt round trip 2^%d %s" % (logn, name))
            D.call("sfp_ntt", p, m, 1)
            inv = D.down(p, (4, R.n))
            D.release()
            for (d, r, k), w in want.items():
                assert int((inv if d else f)[r][k]) == w, ("ntt 2^%d" % logn, name, "inverse" if d else "forward", r, k)
            outs.append((f, inv))
        for f, inv in outs[1:]:
            assert np.array_equal(f, outs[0][0]) and np.array_equal(inv, outs[0][1]), "ntt 2^%d: the libraries differ" % logn


# ---- 3. sums at their widest ----------------------------------------------------------

WIDE = Limbs(2, 2, 0, 0, 2)  # primes 0 (just below 2^60, integer row) and 2 (just below 2^42, FP64 row)


def sum_inputs(R, m, nin, kind, seed):
    """nin polynomials and nin weights per limb: all q - 1, or seeded uniform."""
    rng = random.Random(seed)
    qs = [R.primes[p] for p in m.primes()]
    if kind == "qm1":
        ins = [np.array([[q - 1] * R.n for q in qs], dtype=object)] * nin
        k = np.array([[q - 1 for q in qs]] * nin, dtype=object)
    elif kind == "half":
        # (q - 1) (q + 1)/2 = (q - 1)/2 mod q: every term's lazy residue has magnitude q/2 and
        # the same sign, so nin = 80 terms sum to 40 q in magnitude -- all-(q - 1) terms are
        # (q - 1)^2 = 1 mod q and sum to 80
        ins = [np.array([[q - 1] * R.n for q in qs], dtype=object)] * nin
        k = np.array([[(q + 1) // 2 for q in qs]] * nin, dtype=object)
    else:
        ins = [np.array([[rng.randrange(q) for _ in range(R.n)] for q in qs], dtype=object) for _ in range(nin)]
        k = np.array([[rng.randrange(q) for q in qs] for _ in range(nin)], dtype=object)
    return ins, k


def case_lin_wsum(devs, nin, kind, logn=LOGN):
    R, Ds = setup(devs, logn)
    m, q = WIDE, H.qcol(R, WIDE)
    ins, k = sum_inputs(R, m, nin, kind, nin)
    want = sum(a * k[j].reshape(-1, 1) for j, a in enumerate(ins)) % q
    for D in Ds:
        dp = [D.up(u64(ins[0]))] * nin if kind != "uniform" else [D.up(u64(a)) for a in ins]
        out = D.alloc(m.count * R.n)
        D.call("sfp_lin_wsum", out, D.ptrs(dp), u64(k), nin, m)
        assert_eq(D.down(out, (m.count, R.n)), want, "lin_wsum nin=%d %s" % (nin, kind))
        D.release()


def case_lin_wsum_multi(devs, nin, nout, kind, logn=LOGN):
    R, Ds = setup(devs, logn)
    m, q = WIDE, H.qcol(R, WIDE)
    in0, k0 = sum_inputs(R, m, nin, kind, 100 + nin)
    in1, _ = sum_inputs(R, m, nin, kind, 200 + nin)
    rng = random.Random(nout)
    ks = [k0 if kind != "uniform" else np.array([[rng.randrange(int(qq)) for qq in q.ravel()] for _ in range(nin)],
                                            dtype=object) for _ in range(nout)]
    rows = m.count * R.n
    poly_stride, out_stride = rows + R.n, 2 * (rows + R.n) + R.n  # strides above the rows
    for D in Ds:
        d0 = [D.up(u64(in0[0]))] * nin if kind != "uniform" else [D.up(u64(a)) for a in in0]
        d1 = [D.up(u64(in1[0]))] * nin if kind != "uniform" else [D.up(u64(a)) for a in in1]
        out = D.alloc(nout * out_stride, fill=0xFEED)
        D.call("sfp_lin_wsum_multi", out, out_stride, poly_stride, D.ptrs(d0), D.ptrs(d1), nin,
               u64(np.stack(ks)), nout, m)
        got = D.down(out, (nout, out_stride))
        for o in range(nout):
            for p, ins in enumerate((in0, in1)):
                want = sum(a * ks[o][j].reshape(-1, 1) for j, a in enumerate(ins)) % q
                assert_eq(got[o, p * poly_stride:p * poly_stride + rows].reshape(m.count, R.n), want,
                          "lin_wsum_multi nin=%d nout=%d %s out %d poly %d" % (nin, nout, kind, o, p))
            assert (got[o, rows:poly_stride] == 0xFEED).all() and (got[o, poly_stride + rows:] == 0xFEED).all(), \
                "lin_wsum_multi wrote between its rows"
        D.release()


def case_mac(devs, nin, kind, logn=LOGN):
    """sfp_mac_plain and sfp_mac_plain2."""
    R, Ds = setup(devs, logn)
    m, q = WIDE, H.qcol(R, WIDE)
    a0, _ = sum_inputs(R, m, nin, kind, 300)
    a1, _ = sum_inputs(R, m, nin, kind, 301)
    b, kw = sum_inputs(R, m, nin, kind, 302)
    if kind == "half":
        b = [np.repeat(kw[0].reshape(-1, 1), R.n, axis=1)] * nin
    w0, w1 = sum(x * y for x, y in zip(a0, b)) % q, sum(x * y for x, y in zip(a1, b)) % q
    shape = (m.count, R.n)
    for D in Ds:
        up = (lambda xs: [D.up(u64(xs[0]))] * nin) if kind != "uniform" else (lambda xs: [D.up(u64(x)) for x in xs])
        A0, A1, B = D.ptrs(up(a0)), D.ptrs(up(a1)), D.ptrs(up(b))
        o0, o1 = D.alloc(m.count * R.n), D.alloc(m.count * R.n)
        D.call("sfp_mac_plain", o0, A0, B, nin, m)
        assert_eq(D.down(o0, shape), w0, "mac_plain nin=%d %s" % (nin, kind))
        D.call("sfp_mac_plain2", o1, o0, A1, A0, B, nin, m)
        assert_eq(D.down(o1, shape), w1, "mac_plain2 out0 nin=%d %s" % (nin, kind))
        assert_eq(D.down(o0, shape), w0, "mac_plain2 out1 nin=%d %s" % (nin, kind))
        D.release()


def case_mac_multi(devs, ng, nin, kind, logn=LOGN):
    R, Ds = setup(devs, logn)
    m, q = WIDE, H.qcol(R, WIDE)
    a0, _ = sum_inputs(R, m, nin, kind, 400)
    a1, _ = sum_inputs(R, m, nin, kind, 401)
    b, kw = sum_inputs(R, m, ng * nin, kind, 402)
    if kind == "half":
        b = [np.repeat(kw[0].reshape(-1, 1), R.n, axis=1)] * (ng * nin)
    shape = (m.count, R.n)
    for D in Ds:
        up = (lambda xs: [D.up(u64(xs[0]))] * len(xs)) if kind != "uniform" else (lambda xs: [D.up(u64(x)) for x in xs])
        A0, A1, B = D.ptrs(up(a0)), D.ptrs(up(a1)), D.ptrs(up(b))
        o0 = [D.alloc(m.count * R.n) for _ in range(ng)]
        o1 = [D.alloc(m.count * R.n) for _ in range(ng)]
        assert D.call("sfp_mac_plain2_multi", D.ptrs(o0), D.ptrs(o1), A0, A1, B, nin, ng, m) == 0
        for g in range(ng):
            bg = b[g * nin:(g + 1) * nin]
            assert_eq(D.down(o0[g], shape), sum(x * y for x, y in zip(a0, bg)) % q, "mac_plain2_multi out0 %d" % g)
            assert_eq(D.down(o1[g], shape), sum(x * y for x, y in zip(a1, bg)) % q, "mac_plain2_multi out1 %d" % g)
        D.release()


def case_mac_multi_refused(devs, logn=LOGN):
    """Past SFP_MAC_MULTI_G / _N: -1 and nothing written."""
    R, Ds = setup(devs, logn)
    m = WIDE
    for D in Ds:
        a = D.alloc(m.count * R.n, fill=1)
        outs = [D.alloc(m.count * R.n, fill=0x5A5A) for _ in range(9)]
        for ng, nin in ((9, 32), (8, 33), (0, 1), (1, 0)):
            A = D.ptrs([a] * max(nin, 1))
            B = D.ptrs([a] * max(ng * nin, 1))
            O = D.ptrs(outs[:max(ng, 1)])
            assert D.call("sfp_mac_plain2_multi", O, O, A, A, B, nin, ng, m) == -1, (ng, nin)
        for o in outs:
            assert (D.down(o, (m.count * R.n,)) == 0x5A5A).all(), "a refused mac_plain2_multi wrote"
        D.release()


def case_mac_cols(devs, logn=LOGN, kind="uniform", nin=3):
    """Weak (HIP): tile borders -- ng no multiple of 4, nc odd -- and the refused shapes; kind
    "half" at nin = 32 drives every sum to 16 q."""
    R, Ds = setup(devs, logn)
    m, q = WIDE, H.qcol(R, WIDE)
    ng, nc = 5, 3
    a0, _ = sum_inputs(R, m, nc * nin, kind, 500)
    a1, _ = sum_inputs(R, m, nc * nin, kind, 501)
    b, kw = sum_inputs(R, m, ng * nin, kind, 502)
    if kind == "half":
        b = [np.repeat(kw[0].reshape(-1, 1), R.n, axis=1)] * (ng * nin)
    else:
        a0[0][:] = a1[0][:] = b[0][:] = q - 1
    shape = (m.count, R.n)
    ran = 0
    for D in Ds:
        if not D.has("sfp_mac_plain2_cols"):
            continue
        up = (lambda xs: [D.up(u64(xs[0]))] * len(xs)) if kind != "uniform" else (lambda xs: [D.up(u64(x)) for x in xs])
        A0, A1, B = (D.ptrs(up(xs)) for xs in (a0, a1, b))
        o0 = [D.alloc(m.count * R.n, fill=0x77) for _ in range(nc * ng)]
        o1 = [D.alloc(m.count * R.n, fill=0x77) for _ in range(nc * ng)]
        big = D.ptrs([o0[0]] * (65 * 17))
        for bad in ((33, ng, nc), (nin, 65, nc), (nin, ng, 17), (0, ng, nc)):
            assert D.call("sfp_mac_plain2_cols", big, big, big, big, big, bad[0], bad[1], bad[2], m) == -1, bad
        assert (D.down(o0[0], (m.count * R.n,)) == 0x77).all(), "a refused mac_plain2_cols wrote"
        assert D.call("sfp_mac_plain2_cols", D.ptrs(o0), D.ptrs(o1), A0, A1, B, nin, ng, nc, m) == 0
        for c in range(nc):
            for g in range(ng):
                bg = b[g * nin:(g + 1) * nin]
                for o, a in ((o0, a0), (o1, a1)):
                    want = sum(x * y for x, y in zip(a[c * nin:(c + 1) * nin], bg)) % q
                    assert_eq(D.down(o[c * ng + g], shape), want, "mac_plain2_cols col %d giant %d" % (c, g))
        D.release()
        ran += 1
    return ran


# ---- 4. automorphism ----------------------------------------------------------------

def galois_elements(n):
    return [5, pow(5, n // 2 - 1, 2 * n), 2 * n - 1, 3]


def case_reference_automorph(logn=11):
    """The evaluation-domain index map against the NTT of the coefficient-domain substitution."""
    R = H.ring(H.prime_set(logn), logn)
    a = H.patterns(R, R.primes[1], 3)["uniform"]
    A = R.ntt(a, 1)
    for g in galois_elements(R.n):
        assert np.array_equal(A[R.aut_perm(g)], R.ntt(R.aut_coeff(a, g, R.primes[1]), 1)), g


def case_automorph(devs, mapname, logn=LOGN):
    R, Ds = setup(devs, logn)
    m = maps9()[mapname]
    P = H.pattern_polys(R, m)
    shape = (m.count, R.n)
    for D in Ds:
        out = D.alloc(m.count * R.n)
        for name in ("uniform", "alt1", "delta255", "delta%d" % (R.n - 1)):
            src = D.up(u64(P[name]))
            for g in galois_elements(R.n):
                D.call("sfp_automorph", out, src, g, m)
                assert_eq(D.down(out, shape), P[name][:, R.aut_perm(g)], "automorph g=%d %s %s" % (g, mapname, name))
        D.release()


# ---- 5. rescale family ------------------------------------------------------------------

def dropped_coeffs(R, ql, seed):
    """Coefficients of the dropped row: the rounding boundary floor(q_last / 2) and its
    neighbours, 0, q_last - 1, and seeded values."""
    h = ql >> 1
    edge = [0, ql - 1, h, h + 1, h - 1, 1, h + 2, h - 2]
    rng = random.Random(seed)
    return np.array([edge[i % 8] if i % 16 < 8 else rng.randrange(ql) for i in range(R.n)], dtype=object)


def exact_rescale(R, rows, primes, last_coeffs, ql):
    """out_i = (in_i - NTT_i([last]_{q_i})) ql^-1 mod q_i, last centred in (-ql/2, ql/2]."""
    centred = np.where(last_coeffs > (ql >> 1), last_coeffs - ql, last_coeffs)
    out = []
    for row, p in zip(rows, primes):
        q = R.primes[p]
        out.append((row - R.ntt(centred % q, p)) * pow(ql, -1, q) % q)
    return np.stack(out)


def rescale_inputs(R, ell, drop_prime, seed):
    """Two polynomials of ell rows (evaluation domain): uniform and all-(q-1) kept rows; the
    dropped row is the NTT of dropped_coeffs."""
    ql = R.primes[drop_prime]
    polys, lasts = [], []
    for p in range(2):
        pat = H.pattern_polys(R, ident(ell - 1), seed + p)["uniform" if p == 0 else "qm1"]
        c = dropped_coeffs(R, ql, seed + p)
        polys.append(np.concatenate([pat, R.ntt(c, drop_prime).reshape(1, -1)]))
        lasts.append(c)
    return polys, lasts


def case_rescale(devs, ell, logn=LOGN):
    """sfp_rescale, sfp_mul_const_rescale, sfp_mul_rescale and, where present, the weak *_add
    forms, with npoly = 2 and strides above the rows."""
    R, Ds = setup(devs, logn)
    n, ql = R.n, R.primes[ell - 1]
    polys, lasts = rescale_inputs(R, ell, ell - 1, 40 + ell)
    kept = list(range(ell - 1))
    q = H.qcol(R, ident(ell - 1))
    qlinv = u64([pow(ql, -1, R.primes[i]) for i in kept])
    in_stride, out_stride = (ell + 1) * n, ell * n
    rng = random.Random(ell)
    k = np.array([R.primes[i] - 1 if i % 2 else rng.randrange(R.primes[i]) for i in range(ell)], dtype=object)
    pt = H.pattern_polys(R, ident(ell), 90)["uniform"]
    cst = np.array([[rng.randrange(R.primes[i]) for i in kept], [0] * (ell - 1)], dtype=object)
    want = [exact_rescale(R, polys[p][:-1], kept, lasts[p], ql) for p in range(2)]

    def prod_want(f):  # Rescale(in * f): the dropped row's coefficients are those of the product's last row
        out = []
        for p in range(2):
            pr = polys[p] * f % H.qcol(R, ident(ell))
            out.append(exact_rescale(R, pr[:-1], kept, R.intt(pr[-1], ell - 1), ql))
        return out

    wk, wm = prod_want(k.reshape(-1, 1)), prod_want(pt)
    src = np.full((2, in_stride), 0x1111, dtype=np.uint64)
    for p in range(2):
        src[p, :ell * n] = u64(polys[p]).ravel()

    def check(D, out, w, what, add=None):
        got = D.down(out, (2, out_stride))
        for p in range(2):
            e = w[p] if add is None else (w[p] + add[p].reshape(-1, 1)) % q
            assert_eq(got[p, :(ell - 1) * n].reshape(ell - 1, n), e, "%s ell=%d poly %d" % (what, ell, p))
            assert (got[p, (ell - 1) * n:] == 0x2222).all(), what + " wrote past its rows"

    for D in Ds:
        s = D.up(src)
        mk = lambda: D.alloc(2 * out_stride, fill=0x2222)
        out = mk()
        D.call("sfp_rescale", out, s, ell, qlinv, 2, in_stride, out_stride)
        check(D, out, want, "rescale")
        out = mk()
        D.call("sfp_mul_const_rescale", out, s, u64(k), ell, qlinv, 2, in_stride, out_stride)
        check(D, out, wk, "mul_const_rescale")
        out = mk()
        D.call("sfp_mul_rescale", out, s, D.up(u64(pt)), ell, qlinv, 2, in_stride, out_stride)
        check(D, out, wm, "mul_rescale")
        if D.has("sfp_rescale_add"):
            out = mk()  # (a library that has the form takes these shapes: -1 would leave nothing compared)
            assert D.call("sfp_rescale_add", out, s, ell, qlinv, 2, in_stride, out_stride, u64(cst)) == 0
            check(D, out, want, "rescale_add", cst)
            out = mk()
            assert D.call("sfp_mul_const_rescale_add", out, s, u64(k), ell, qlinv, 2, in_stride, out_stride,
                          u64(cst)) == 0
            check(D, out, wk, "mul_const_rescale_add", cst)
        D.release()


def case_rescale_ext(devs, logn=LOGN):
    """The dropped (last) row modulo prime 8 (60 bits), 7 (below 2^42) and 4 (32 bits)."""
    R, Ds = setup(devs, logn)
    n, ell = R.n, 4
    for drop in (8, 7, 4):
        ql = R.primes[drop]
        polys, lasts = rescale_inputs(R, ell, drop, 60 + drop)
        kept = list(range(ell - 1))
        qlinv = u64([pow(ql, -1, R.primes[i]) for i in kept])
        for D in Ds:
            for p in range(2):
                out = D.alloc((ell - 1) * n)
                D.call("sfp_rescale_ext", out, D.up(u64(polys[p])), ell, drop, qlinv, 1, 0, 0)
                assert_eq(D.down(out, (ell - 1, n)), exact_rescale(R, polys[p][:-1], kept, lasts[p], ql),
                          "rescale_ext drop %d poly %d" % (drop, p))
            D.release()


def case_rescale_rows(devs, mapname, logn=LOGN):
    """The dropped row supplied in coefficient form, kept rows on a limb map."""
    R, Ds = setup(devs, logn)
    n, m = R.n, maps9()[mapname]
    drop = 2 if mapname == "stride" else 5
    ql = R.primes[drop]
    prs = m.primes()
    qlinv = u64([pow(ql, -1, R.primes[i]) for i in prs])
    rows = m.count * n
    in_stride, out_stride, last_stride = rows + n, rows + 2 * n, 2 * n
    ins = [H.pattern_polys(R, m, 70 + p)["uniform" if p == 0 else "qm1"] for p in range(2)]
    lasts = [dropped_coeffs(R, ql, 80 + p) for p in range(2)]
    src = np.zeros((2, in_stride), dtype=np.uint64)
    lst = np.zeros((2, last_stride), dtype=np.uint64)
    for p in range(2):
        src[p, :rows], lst[p, :n] = u64(ins[p]).ravel(), u64(lasts[p])
    for D in Ds:
        out = D.alloc(2 * out_stride, fill=0x3333)
        D.call("sfp_rescale_rows", out, D.up(src), D.up(lst), drop, m, qlinv, 2, in_stride, out_stride, last_stride)
        got = D.down(out, (2, out_stride))
        for p in range(2):
            assert_eq(got[p, :rows].reshape(m.count, n), exact_rescale(R, ins[p], prs, lasts[p], ql),
                      "rescale_rows %s poly %d" % (mapname, p))
            assert (got[p, rows:] == 0x3333).all()
        D.release()


# ---- 6. base conversion ------------------------------------------------------------------

CONV_T = [16, 17, 18, 19, 20]  # 30 bits (FP64), below 2^42 (FP64), above 2^42, 50 bits, 60 bits
CONV_ROWS = [5, 0, 3, 1, 6]    # target t -> output row (a 7-row buffer; rows 2 and 4 stay untouched)


def conv_sources(ns, nbig):
    """ns source prime indices, nbig of them of 60 bits (first, as q_0 is)."""
    return list(range(nbig)) + list(range(3, 3 + ns - nbig))


def conv_shapes():
    return [(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (12, 0), (12, 1), (12, 2), (13, 0), (13, 1), (13, 2), (13, 3)]


def generic_y(R, cr, seed):
    """Seeded uniform y rows with no coefficient within 2^-30 of a tie (the seed is advanced
    until there is none: the chance per coefficient is about 2^-29)."""
    for s in range(seed, seed + 50):
        rng = random.Random(s)
        y = [np.array([rng.randrange(q) for _ in range(R.n)], dtype=object) for q in cr.s]
        x = cr.sources_for(y)
        if cr.centred(x)[1].all():
            return x
    raise AssertionError("no generic seed")


TIE_OFFSETS = [0, 1, -1, 2, -2, 3, -3, 5] + [sg << k for k in (5, 6, 7, 8, 9, 11) for sg in (1, -1)]


def tie_y(R, cr):
    """Near-tie inputs: all (s-1)/2, all (s+1)/2, and mixtures: an odd number of halves
    (s_i -+ 1)/2, whose distance -+sum 1/(2 s_i) from k + 1/2 the LARGEST source c cancels
    (y_c = round(s_c sum 1/(2 s_i))), plus an offset d per coefficient: the sum is
    k + 1/2 + (d + e)/s_c with |e| <= 1/2.  With s_c near 2^60 one ulp of the FP64 sum
    (2^-53 or 2^-52) is 2^7..2^8 units of 1/s_c, so d = 0, +-1..5 sits inside the ulp and
    +-2^5..2^11 brackets it from 1/4 ulp to 16; with s_c near 2^42 a unit is 2^10 ulps and
    only e is closer."""
    from fractions import Fraction
    ns, n = len(cr.s), R.n
    out = [[np.array([(s - 1) // 2] * n, dtype=object) for s in cr.s],
           [np.array([(s + 1) // 2] * n, dtype=object) for s in cr.s]]
    if ns >= 2:
        c = max(range(ns), key=lambda i: cr.s[i])
        halves = [i for i in range(ns) if i != c][:3 if ns >= 4 else 1]
        delta = sum(Fraction(1, 2 * cr.s[i]) for i in halves)
        for sign in (1, -1):
            y = []
            for i, s in enumerate(cr.s):
                if i == c:
                    base = sign * round(delta * s)
                    y.append(np.array([(base + TIE_OFFSETS[x % len(TIE_OFFSETS)]) % s for x in range(n)],
                                      dtype=object))
                elif i in halves:
                    y.append(np.array([((s - 1) // 2 if sign > 0 else (s + 1) // 2)] * n, dtype=object))
                else:
                    y.append(np.array([0] * n, dtype=object))
            out.append(y)
    return [cr.sources_for(y) for y in out]


def case_conv(devs, ns, nbig, logn=LOGN):
    primes = H.conv_prime_set(logn)
    R, Ds = setup(devs, logn, primes)
    n = R.n
    cr = H.ConvRef(R, conv_sources(ns, nbig), CONV_T, CONV_ROWS)
    xg = generic_y(R, cr, 1000 * ns + nbig)
    consts = [np.stack([np.array(f(s) * (n // 2), dtype=object) for s in cr.s])
              for f in (lambda s: [0, 0], lambda s: [1, 1], lambda s: [s - 1, s - 1], lambda s: [s >> 1, (s >> 1) + 1],
                        lambda s: [s - 1, 1])]
    ties = tie_y(R, cr)
    nt_use = 3
    results = []
    for D in Ds:
        c = cr.upload(D)
        res = []
        for x in [xg] + consts + ties:
            src = D.up(u64(x))
            dst = D.alloc(7 * n, fill=0x4444)
            D.call("sfp_conv_apply", dst, src, c)
            plain = D.down(dst, (7, n))
            dst2 = D.alloc(7 * n, fill=0x4444)
            D.call("sfp_conv_apply_centered", dst2, src, c, nt_use)
            res.append((plain, D.down(dst2, (7, n))))
        D.call("sfp_free_conv", c)
        D.release()
        results.append(res)
    for res in results:
        for j, x in enumerate([xg] + consts + ties):
            plain, cen = res[j]
            want = cr.plain(x)
            wc, generic = cr.centred(x)
            for t, r in enumerate(CONV_ROWS):
                assert_eq(plain[r], want[t], "conv_apply ns=%d big=%d input %d target %d" % (ns, nbig, j, t))
            assert (plain[[2, 4]] == 0x4444).all() and (cen[[2, 4]] == 0x4444).all()
            for r in CONV_ROWS[nt_use:]:
                assert (cen[r] == 0x4444).all(), "conv_apply_centered wrote a target past nt_use"
            if j == 0:
                assert generic.all()
            # generic coefficients: the exact centred value.  Near ties: exact or exact +- prod(S),
            # the same choice on every target.
            choice = None
            for t in range(nt_use):
                got, tq = obj(cen[CONV_ROWS[t]]), cr.t[t]
                d = (got - wc[t]) % tq
                pm = cr.prod % tq
                ch = np.where(d == 0, 0, np.where(d == pm, 1, np.where(d == (-pm) % tq, -1, 9)))
                assert not (ch[generic] != 0).any(), "conv_apply_centered ns=%d big=%d input %d target %d: " \
                    "a generic coefficient is not the exact centred value" % (ns, nbig, j, t)
                assert not (ch == 9).any(), "conv_apply_centered: neither exact nor exact +- prod(S)"
                assert choice is None or np.array_equal(choice, ch), "targets disagree on the overflow"
                choice = ch
    for res in results[1:]:  # the libraries agree everywhere, near ties included
        for (p0, c0), (p1, c1) in zip(results[0], res):
            assert np.array_equal(p0, p1) and np.array_equal(c0, c1), "conv: the libraries differ"


# ---- 7 (part). the key inner products on uploaded rows ------------------------------------

def case_ks_inner(devs, logn=LOGN):
    """sfp_ks_inner / _acc / _fold / _mul / _aut / _mul_aut: ell = 5 of Lq = 7, K = 2 (primes 7, 8),
    beta = 3 digits; keys and digits are arbitrary rows: uniform, and all q - 1."""
    R, Ds = setup(devs, logn)
    n, ell, K, Lq, beta = R.n, 5, 2, 7, 3
    rows = ell + K
    m = Limbs(rows, ell, Lq, 0, 0)
    q = H.qcol(R, m)
    kr = list(range(ell)) + [Lq, Lq + 1]  # key row of ext row t
    NP = Lq + K
    km = ident(NP)
    for kind in ("uniform", "qm1"):
        ext = [H.pattern_polys(R, m, 20 + j)[kind] for j in range(beta)]
        kb = [H.pattern_polys(R, km, 30 + j)[kind] for j in range(beta)]
        ka = [H.pattern_polys(R, km, 40 + j)[kind] for j in range(beta)]
        pm = H.pattern_polys(R, m, 50)[kind]
        f0, f1 = H.pattern_polys(R, ident(ell), 51)[kind], H.pattern_polys(R, ident(ell), 52)[kind]
        s0 = sum(e * b[kr] for e, b in zip(ext, kb)) % q
        s1 = sum(e * a[kr] for e, a in zip(ext, ka)) % q
        stride = rows * n + n
        ebuf = np.zeros((beta, stride), dtype=np.uint64)
        for j in range(beta):
            ebuf[j, :rows * n] = u64(ext[j]).ravel()
        key = np.concatenate([np.concatenate([u64(kb[j]), u64(ka[j])]) for j in range(beta)])
        fold_k = R.primes[ell - 1] - 2
        shape = (rows, n)
        g = 5
        perm = R.aut_perm(g)
        sp0 = sum(e[:, perm] * b[kr] for e, b in zip(ext, kb)) % q
        sp1 = sum(e[:, perm] * a[kr] for e, a in zip(ext, ka)) % q
        for D in Ds:
            E, Kd, PM = D.up(ebuf), D.up(key), D.up(u64(pm))
            a0, a1 = D.alloc(rows * n), D.alloc(rows * n)
            D.call("sfp_ks_inner", a0, a1, E, stride, Kd, beta, ell, K, Lq)
            assert_eq(D.down(a0, shape), s0, "ks_inner acc0 " + kind)
            assert_eq(D.down(a1, shape), s1, "ks_inner acc1 " + kind)
            D.call("sfp_ks_inner_acc", a0, a1, E, stride, Kd, beta, ell, K, Lq)
            assert_eq(D.down(a0, shape), 2 * s0 % q, "ks_inner_acc acc0 " + kind)
            assert_eq(D.down(a1, shape), 2 * s1 % q, "ks_inner_acc acc1 " + kind)
            D.call("sfp_ks_inner_fold", a0, a1, E, stride, Kd, beta, ell, K, Lq, D.up(u64(f0)), D.up(u64(f1)), fold_k)
            w0, w1 = s0.copy(), s1.copy()
            w0[ell - 1] = (w0[ell - 1] + f0[ell - 1] * fold_k) % R.primes[ell - 1]
            w1[ell - 1] = (w1[ell - 1] + f1[ell - 1] * fold_k) % R.primes[ell - 1]
            assert_eq(D.down(a0, shape), w0, "ks_inner_fold acc0 " + kind)
            assert_eq(D.down(a1, shape), w1, "ks_inner_fold acc1 " + kind)
            D.call("sfp_ks_inner_mul", a0, a1, E, stride, Kd, beta, ell, K, Lq, PM, 0)
            assert_eq(D.down(a0, shape), s0 * pm % q, "ks_inner_mul acc0 " + kind)
            D.call("sfp_ks_inner_mul", a0, a1, E, stride, Kd, beta, ell, K, Lq, PM, 1)
            assert_eq(D.down(a0, shape), 2 * s0 * pm % q, "ks_inner_mul accum acc0 " + kind)
            assert_eq(D.down(a1, shape), 2 * s1 * pm % q, "ks_inner_mul accum acc1 " + kind)
            D.call("sfp_ks_inner_aut", a0, a1, E, stride, Kd, beta, ell, K, Lq, g)
            assert_eq(D.down(a0, shape), sp0, "ks_inner_aut acc0 " + kind)
            assert_eq(D.down(a1, shape), sp1, "ks_inner_aut acc1 " + kind)
            D.call("sfp_ks_inner_mul_aut", a0, a1, E, stride, Kd, beta, ell, K, Lq, PM, 1, g)
            assert_eq(D.down(a0, shape), (sp0 + sp0 * pm) % q, "ks_inner_mul_aut acc0 " + kind)
            assert_eq(D.down(a1, shape), (sp1 + sp1 * pm) % q, "ks_inner_mul_aut acc1 " + kind)
            D.release()


# ---- 7. the key-switch chain on uploaded rows ---------------------------------------------

KS = dict(ell=5, K=2, Lq=7, alpha=2)  # digits (0, 1), (2, 3) and the ragged (4); P = primes 7, 8
NONE32 = 0xFFFFFFFF


def ks_primes(pset, logn):
    return H.prime_set(logn) if pset == "mixed" else H.fp_prime_set(logn)


def ks_convs(R, ell, K, Lq, alpha):
    """The ModUp table of every digit (targets: the other q rows at their index, P row k at
    ell + k) and the ModDown table P -> q rows, as prims.h lays them out."""
    beta = (ell + alpha - 1) // alpha
    up = []
    for j in range(beta):
        lo, hi = j * alpha, min(j * alpha + alpha, ell)
        dst = [i for i in range(ell) if not lo <= i < hi] + [Lq + k for k in range(K)]
        up.append(H.ConvRef(R, range(lo, hi), dst, [p if p < Lq else ell + p - Lq for p in dst]))
    return up, H.ConvRef(R, range(Lq, Lq + K), range(Lq))


def exact_modup(R, inp, up, ell, K):
    """Per digit: own rows copied, the others NTT(Conv_j(INTT(in[digit j])))."""
    coef = [R.intt(inp[i], i) for i in range(ell)]
    out = []
    for cr in up:
        e = np.zeros((ell + K, R.n), dtype=object)
        conv = cr.plain(np.stack([coef[i] for i in cr.S]))
        for t, (p, r) in enumerate(zip(cr.T, cr.dst_row)):
            e[r] = R.ntt(conv[t], p)
        for i in cr.S:
            e[i] = inp[i]
        out.append(e)
    return out


def exact_moddown(R, acc, down, ell, K, Lq):
    """(acc_i - NTT(Conv_{P->Q}(INTT(acc_P)))_i) P^-1 with the conversion of the true centred
    value; and per coefficient whether the conversion's input is generic."""
    pc = np.stack([R.intt(acc[ell + k], Lq + k) for k in range(K)])
    cen, generic = down.centred(pc)
    out = [(acc[i] - R.ntt(cen[i], i)) * pow(down.prod, -1, R.primes[i]) % R.primes[i] for i in range(ell)]
    return np.stack(out), generic


def exact_md_rescale(R, acc, dd, down, ell, K, Lq, fold_k):
    """Fold row l, ModDown, add d on rows < l, Rescale (prims.h, sfp_moddown_rescale)."""
    l = ell - 1
    a = acc.copy()
    a[l] = (a[l] + dd[l] * fold_k) % R.primes[l]
    s, generic = exact_moddown(R, a, down, ell, K, Lq)
    assert generic.all()
    for i in range(l):
        s[i] = (s[i] + dd[i]) % R.primes[i]
    return exact_rescale(R, s[:-1], list(range(l)), R.intt(s[l], l), R.primes[l])


def near_tie_check(R, got, want, generic, ell, what):
    """A ModDown output on near-tie P rows: in the coefficient domain every coefficient is the
    exact one or differs by the conversion's +-prod(P) (here +-1 after P^-1), the same choice
    on every row, and a generic coefficient is exact."""
    choice = None
    for i in range(ell):
        q = R.primes[i]
        e = R.intt((obj(want[i]) - obj(got[i])) % q, i)
        ch = np.where(e == 0, 0, np.where(e == 1, 1, np.where(e == q - 1, -1, 9)))
        assert not (ch == 9).any(), what + ": neither exact nor exact +- prod(P)"
        assert not (ch[generic] != 0).any(), what + ": a generic coefficient is not exact"
        assert choice is None or np.array_equal(choice, ch), what + ": rows disagree on the overflow"
        choice = ch


def ks_inputs(R, kind, ell, K, Lq, beta, down):
    """in (ell rows), d0 / d1 (ell rows), the key (beta digits of b rows then a rows), and the
    accumulators' P rows for the ModDown cases: of the kind's pattern, or, kind 'tie', the NTT
    of coefficient rows whose centred conversion sits next to a tie."""
    rows = ell + K
    m = Limbs(rows, ell, Lq, 0, 0)
    pat = "uniform" if kind == "tie" else kind
    inp = H.pattern_polys(R, ident(ell), 61)[pat]
    d0, d1 = H.pattern_polys(R, ident(ell), 62)[pat], H.pattern_polys(R, ident(ell), 63)[pat]
    kb = [H.pattern_polys(R, ident(Lq + K), 30 + j)[pat] for j in range(beta)]
    ka = [H.pattern_polys(R, ident(Lq + K), 40 + j)[pat] for j in range(beta)]
    acc = [H.pattern_polys(R, m, 64 + p)[pat] for p in range(2)]
    if kind == "tie":
        ties = tie_y(R, down)
        for p in range(2):
            x = ties[2 + p] if len(ties) > 2 else ties[p]
            for k in range(K):
                acc[p][ell + k] = R.ntt(x[k], Lq + k)
    return inp, d0, d1, kb, ka, acc


def case_ks_chain(devs, pset, kind, logn=LOGN):
    """sfp_modup, sfp_ks_inner(_fold), sfp_moddown2 (add0 / add1 both ways) and
    sfp_moddown_rescale against the exact reference, then every fused form a library has
    (sfp_modup_inner, its phases, sfp_mult_relin_rescale, the *_add forms) against the
    unfused definition prims.h names -- which is that same exact value.  Returns the number
    of libraries whose fused forms ran."""
    R, Ds = setup(devs, logn, ks_primes(pset, logn))
    n, ell, K, Lq, alpha = R.n, KS["ell"], KS["K"], KS["Lq"], KS["alpha"]
    rows, l, beta = ell + K, ell - 1, (ell + alpha - 1) // alpha
    up, down = ks_convs(R, ell, K, Lq, alpha)
    inp, d0, d1, kb, ka, accP = ks_inputs(R, kind, ell, K, Lq, beta, down)
    m = Limbs(rows, ell, Lq, 0, 0)
    q, ql = H.qcol(R, m), H.qcol(R, ident(ell))
    kr = list(range(ell)) + [Lq + k for k in range(K)]
    P = down.prod
    pinv = u64([pow(P, -1, R.primes[i]) for i in range(ell)])
    pmod = u64([P % R.primes[i] for i in range(ell)])
    qlinv = u64([pow(R.primes[l], -1, R.primes[i]) for i in range(l)])
    fold_k = P % R.primes[l]
    key = np.concatenate([np.concatenate([u64(kb[j]), u64(ka[j])]) for j in range(beta)])

    # the exact chain
    ext = exact_modup(R, inp, up, ell, K)
    s = [sum(e * k[kr] for e, k in zip(ext, kk)) % q for kk in (kb, ka)]
    md = [exact_moddown(R, accP[p], down, ell, K, Lq) for p in range(2)]
    generic = md[0][1] & md[1][1]
    assert generic.all() == (kind != "tie")
    prev = H.pattern_polys(R, ident(ell), 65)["uniform"]
    if kind != "tie":
        mdr = [exact_md_rescale(R, s[p], (d0, d1)[p], down, ell, K, Lq, fold_k) for p in range(2)]
        mds = [exact_moddown(R, s[p], down, ell, K, Lq)[0] for p in range(2)]
        # EvalMult end to end: operands (a, b) = (inp, d0), (d1, inp) -> tensor (t0, t1, t2)
        a0, a1, b0, b1 = d0, inp, d1, inp
        t0, t1, t2 = a0 * b0 % ql, (a0 * b1 + a1 * b0) % ql, a1 * b1 % ql
        ext2 = exact_modup(R, t2, up, ell, K)
        s2 = [sum(e * k[kr] for e, k in zip(ext2, kk)) % q for kk in (kb, ka)]
        mrr = [exact_md_rescale(R, s2[p], (t0, t1)[p], down, ell, K, Lq, fold_k) for p in range(2)]
        rng = random.Random(9)
        cst = np.array([rng.randrange(R.primes[i]) for i in range(l)], dtype=object)
        r0, r1 = H.pattern_polys(R, ident(l), 66)["uniform"], H.pattern_polys(R, ident(l), 67)["qm1"]
    qk = H.qcol(R, ident(l))
    fused = 0
    tie_out = []
    for D in Ds:
        cj = [c.upload(D) for c in up]
        assert all(cj)
        cv = D.ptrs(cj)
        cP = down.upload(D)
        IN, D0, D1, KEY = D.up(u64(inp)), D.up(u64(d0)), D.up(u64(d1)), D.up(key)
        E = D.alloc(beta * rows * n)
        scr = D.alloc(2 * ell * n)
        acc = D.alloc(2 * rows * n)
        acc1 = acc + rows * n * 8
        o0, o1 = D.alloc(ell * n), D.alloc(ell * n)

        def put_acc(a):
            D.put(acc, np.concatenate([u64(a[0]).ravel(), u64(a[1]).ravel()]))

        def down2(what, w, add0=0, add1=0, row_done=0):
            D.put(o0, u64(prev))
            D.put(o1, u64(prev))
            D.call("sfp_moddown2", o0, o1, acc, rows * n, ell, K, Lq, cP, pinv, add0, add1, scr, row_done)
            got = [D.down(o0, (ell, n)), D.down(o1, (ell, n))]
            for p, add in enumerate((add0, add1)):
                if add:
                    got[p] = u64((obj(got[p]) - prev) % ql)
            if kind == "tie":
                for p in range(2):
                    near_tie_check(R, got[p], w[p], md[p][1], ell, what)
                tie_out.append(got)
            else:
                for p in range(2):
                    assert_eq(got[p], w[p], "%s poly %d (%s, %s)" % (what, p, pset, kind))

        if kind == "tie":
            put_acc(accP)
            down2("moddown2 near a tie", [md[0][0], md[1][0]])
        else:
            D.call("sfp_modup", E, IN, ell, K, Lq, alpha, cv, scr)
            got = D.down(E, (beta, rows, n))
            for j in range(beta):
                assert_eq(got[j], ext[j], "modup digit %d (%s, %s)" % (j, pset, kind))
            D.call("sfp_ks_inner", acc, acc1, E, rows * n, KEY, beta, ell, K, Lq)
            assert_eq(D.down(acc, (rows, n)), s[0], "ks_inner of the modup acc0")
            assert_eq(D.down(acc1, (rows, n)), s[1], "ks_inner of the modup acc1")
            down2("moddown2", mds)
            for add in ((1, 0), (0, 1), (1, 1)):
                put_acc(s)
                down2("moddown2 add=%d%d" % add, mds, *add)
            put_acc(accP)
            down2("moddown2 of pattern accumulators", [md[0][0], md[1][0]])
            D.call("sfp_ks_inner_fold", acc, acc1, E, rows * n, KEY, beta, ell, K, Lq, D0, D1, fold_k)
            D.call("sfp_moddown_rescale", o0, o1, D0, D1, acc, rows * n, ell, K, Lq, cP, pinv, pmod, qlinv, scr, 0)
            assert_eq(D.down(o0, (l, n)), mdr[0], "moddown_rescale out0 (%s, %s)" % (pset, kind))
            assert_eq(D.down(o1, (l, n)), mdr[1], "moddown_rescale out1 (%s, %s)" % (pset, kind))
            R0, R1 = D.up(u64(r0)), D.up(u64(r1))
            if D.has("sfp_moddown_rescale_add"):
                for sign in (1, -1):
                    D.call("sfp_ks_inner_fold", acc, acc1, E, rows * n, KEY, beta, ell, K, Lq, D0, D1, fold_k)
                    assert D.call("sfp_moddown_rescale_add", o0, o1, D0, D1, acc, rows * n, ell, K, Lq, cP, pinv,
                                  pmod, qlinv, scr, 0, R0, R1, sign, u64(cst)) == 0
                    assert_eq(D.down(o0, (l, n)), (mdr[0] + sign * r0 + cst.reshape(-1, 1)) % qk,
                              "moddown_rescale_add out0 sign %d" % sign)
                    assert_eq(D.down(o1, (l, n)), (mdr[1] + sign * r1) % qk, "moddown_rescale_add out1 sign %d" % sign)
            # ---- the fused forms (return -1 where a library has none: the oracle) ----
            E2 = D.alloc(beta * rows * n)
            if D.call("sfp_modup_inner_phase", acc, acc1, IN, ell, K, Lq, alpha, cv, KEY, None, None, 0, 0, NONE32,
                      E2, scr, 0) == 0:
                fused += 1
                mi = lambda *a: D.call("sfp_modup_inner", acc, acc1, IN, ell, K, Lq, alpha, cv, KEY, *a)
                assert mi(None, None, 0, 0, NONE32, E2, scr) == 0
                assert_eq(D.down(acc, (rows, n)), s[0], "modup_inner acc0")
                assert_eq(D.down(acc1, (rows, n)), s[1], "modup_inner acc1")
                assert mi(None, None, 0, 1, NONE32, E2, scr) == 0
                assert_eq(D.down(acc, (rows, n)), 2 * s[0] % q, "modup_inner accumulating acc0")
                assert_eq(D.down(acc1, (rows, n)), 2 * s[1] % q, "modup_inner accumulating acc1")
                assert mi(None, None, 0, 0, ell, E2, scr) == 0  # the P rows leave after their ROW pass
                whole = D.down(acc, (2 * rows, n))
                down2("modup_inner + moddown2 row_done", mds, 1, 0, 1)
                D.put(acc, np.full(2 * rows * n, 7, dtype=np.uint64))
                ph = lambda k: D.call("sfp_modup_inner_phase", acc, acc1, IN, ell, K, Lq, alpha, cv, KEY, None, None,
                                      0, 0, ell, E2, scr, k)
                assert ph(1) == 0 and ph(2) == 0
                assert np.array_equal(D.down(acc, (2 * rows, n)), whole), "modup_inner phases 1 + 2 differ from 3"
                assert mi(D0, D1, fold_k, 0, l, E2, scr) == 0
                D.call("sfp_moddown_rescale", o0, o1, D0, D1, acc, rows * n, ell, K, Lq, cP, pinv, pmod, qlinv, scr, 1)
                assert_eq(D.down(o0, (l, n)), mdr[0], "modup_inner fold + moddown_rescale out0")
                assert_eq(D.down(o1, (l, n)), mdr[1], "modup_inner fold + moddown_rescale out1")
                mr = (o0, o1, D0, IN, D1, IN, ell, K, Lq, alpha, cv, KEY, cP, pinv, pmod, qlinv, acc, E2, scr)
                assert D.call("sfp_mult_relin_rescale", *mr) == 0
                assert_eq(D.down(o0, (l, n)), mrr[0], "mult_relin_rescale out0 (%s, %s)" % (pset, kind))
                assert_eq(D.down(o1, (l, n)), mrr[1], "mult_relin_rescale out1 (%s, %s)" % (pset, kind))
                for sign in (1, -1):
                    assert D.call("sfp_mult_relin_rescale_add", *mr, R0, R1, sign, u64(cst)) == 0
                    assert_eq(D.down(o0, (l, n)), (mrr[0] + sign * r0 + cst.reshape(-1, 1)) % qk,
                              "mult_relin_rescale_add out0 sign %d" % sign)
                    assert_eq(D.down(o1, (l, n)), (mrr[1] + sign * r1) % qk,
                              "mult_relin_rescale_add out1 sign %d" % sign)
        D.call("sfp_sync")
        for c in cj + [cP]:
            D.call("sfp_free_conv", c)
        D.release()
    for got in tie_out[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got, tie_out[0])), "moddown2 near a tie: the libraries differ"
    return fused


def case_const_terms(devs, logn=LOGN, merged=1):
    """Weak (HIP): sfp_const_terms_rescale of three terms at ell = 4, 3, 2 (one with constants)
    against Rescale(in * k_j) + cst_j, each from the exact reference; the return value says
    whether the terms went out merged (1) or one by one (0: a one-tile ring)."""
    R, Ds = setup(devs, logn)
    n, L = R.n, 4
    in_stride = (L + 1) * n
    polys = [H.pattern_polys(R, ident(L), 71 + p)["uniform" if p == 0 else "qm1"] for p in range(2)]
    src = np.full((2, in_stride), 0x1111, dtype=np.uint64)
    for p in range(2):
        src[p, :L * n] = u64(polys[p]).ravel()
    rng = random.Random(12)
    terms = []
    for ell in (4, 3, 2):
        k = np.array([R.primes[i] - 1 if i % 2 else rng.randrange(R.primes[i]) for i in range(ell)], dtype=object)
        cst = np.array([[rng.randrange(R.primes[i]) for i in range(ell - 1)], [0] * (ell - 1)],
                       dtype=object) if ell != 3 else None
        ql, kept = R.primes[ell - 1], list(range(ell - 1))
        want = []
        for p in range(2):
            pr = polys[p][:ell] * k.reshape(-1, 1) % H.qcol(R, ident(ell))
            w = exact_rescale(R, pr[:-1], kept, R.intt(pr[-1], ell - 1), ql)
            want.append(w if cst is None else (w + cst[p].reshape(-1, 1)) % H.qcol(R, ident(ell - 1)))
        terms.append((ell, u64(k), u64([pow(ql, -1, R.primes[i]) for i in kept]), None if cst is None else u64(cst),
                      want))
    ran = 0
    for D in Ds:
        if not D.has("sfp_const_terms_rescale"):
            continue
        s = D.up(src)
        out_stride = L * n
        outs = [D.alloc(2 * out_stride, fill=0x2222) for _ in terms]
        arr = (H.ConstTerm * len(terms))()
        for j, (ell, k, qlinv, cst, _) in enumerate(terms):
            arr[j] = H.ConstTerm(ell, H._host(k).value, H._host(qlinv).value, outs[j], out_stride,
                                 None if cst is None else H._host(cst).value)
        import ctypes
        r = D.call("sfp_const_terms_rescale", s, in_stride, 2, ctypes.addressof(arr), len(terms))
        assert r == merged, "const_terms_rescale returned %d" % r
        for j, (ell, _, _, _, want) in enumerate(terms):
            got = D.down(outs[j], (2, out_stride))
            for p in range(2):
                assert_eq(got[p, :(ell - 1) * n].reshape(ell - 1, n), want[p], "const_terms term %d poly %d" % (j, p))
                assert (got[p, (ell - 1) * n:] == 0x2222).all(), "const_terms wrote past its rows"
        D.release()
        ran += 1
    return ran


def case_ks_chain_large(devs, logn=16):
    """The n = 2^16 key switch (the ModUp / ModDown COL kernels and the fused inner product
    exist only there), ell = 5: every library against the exact reference where a full Python
    transform is not needed -- the ragged digit's ModUp (one source row: its conversion is the
    identity on [0, s)), at the border indices -- and every output of every step, fused forms
    included, against the first library's unfused sequence (the oracle's on the GPU half)."""
    R, Ds = setup(devs, logn, ks_primes("fp", logn))
    n, ell, K, Lq, alpha = R.n, KS["ell"], KS["K"], KS["Lq"], KS["alpha"]
    rows, l, beta = ell + K, ell - 1, (ell + alpha - 1) // alpha
    up, down = ks_convs(R, ell, K, Lq, alpha)
    inp, d0, d1, kb, ka, _ = ks_inputs(R, "uniform", ell, K, Lq, beta, down)
    P = down.prod
    pinv = u64([pow(P, -1, R.primes[i]) for i in range(ell)])
    pmod = u64([P % R.primes[i] for i in range(ell)])
    qlinv = u64([pow(R.primes[l], -1, R.primes[i]) for i in range(l)])
    fold_k = P % R.primes[l]
    key = np.concatenate([np.concatenate([u64(kb[j]), u64(ka[j])]) for j in range(beta)])
    c4 = R.intt(inp[4], 4)  # digit 2 = row 4 alone: Conv is x -> x mod t
    spots = {(r, x): R.ntt_at(c4 % R.primes[p], p, x) for p, r in zip(up[2].T, up[2].dst_row)
             for x in R.border_indices()[::3]}
    outs, fused = [], 0
    for D in reversed(Ds):  # the oracle first
        cj = [c.upload(D) for c in up]
        cv, cP = D.ptrs(cj), down.upload(D)
        IN, D0, D1, KEY = D.up(u64(inp)), D.up(u64(d0)), D.up(u64(d1)), D.up(key)
        E, scr, acc = D.alloc(beta * rows * n), D.alloc(2 * ell * n), D.alloc(2 * rows * n)
        acc1 = acc + rows * n * 8
        o0, o1 = D.alloc(ell * n, fill=0), D.alloc(ell * n, fill=0)
        res = {}
        D.call("sfp_modup", E, IN, ell, K, Lq, alpha, cv, scr)
        res["modup"] = D.down(E, (beta, rows, n))
        for (r, x), w in spots.items():
            assert int(res["modup"][2, r, x]) == w, ("modup 2^16 ragged digit", r, x)
        assert np.array_equal(res["modup"][2, 4], u64(inp[4]))
        D.call("sfp_ks_inner", acc, acc1, E, rows * n, KEY, beta, ell, K, Lq)
        res["inner"] = D.down(acc, (2 * rows, n))
        D.call("sfp_moddown2", o0, o1, acc, rows * n, ell, K, Lq, cP, pinv, 0, 0, scr, 0)
        once = D.down(o0, (ell, n))
        D.call("sfp_ks_inner", acc, acc1, E, rows * n, KEY, beta, ell, K, Lq)
        D.call("sfp_moddown2", o0, o1, acc, rows * n, ell, K, Lq, cP, pinv, 1, 0, scr, 0)
        res["moddown2"] = np.stack([D.down(o0, (ell, n)), D.down(o1, (ell, n))])  # out0: added to the first
        D.call("sfp_ks_inner_fold", acc, acc1, E, rows * n, KEY, beta, ell, K, Lq, D0, D1, fold_k)
        D.call("sfp_moddown_rescale", o0, o1, D0, D1, acc, rows * n, ell, K, Lq, cP, pinv, pmod, qlinv, scr, 0)
        res["mdrs"] = np.stack([D.down(o0, (l, n)), D.down(o1, (l, n))])
        q2 = H.qcol(R, ident(ell))
        assert_eq(res["moddown2"][0], 2 * obj(once) % q2, "moddown2 2^16 add0")
        if D.call("sfp_modup_inner_phase", acc, acc1, IN, ell, K, Lq, alpha, cv, KEY, None, None, 0, 0, NONE32,
                  E, scr, 0) == 0:
            fused += 1
            first = outs[0] if outs else res
            assert D.call("sfp_modup_inner", acc, acc1, IN, ell, K, Lq, alpha, cv, KEY, None, None, 0, 0, NONE32,
                          E, scr) == 0
            assert np.array_equal(D.down(acc, (2 * rows, n)), first["inner"]), "modup_inner 2^16"
            assert D.call("sfp_modup_inner", acc, acc1, IN, ell, K, Lq, alpha, cv, KEY, D0, D1, fold_k, 0, l,
                          E, scr) == 0
            D.call("sfp_moddown_rescale", o0, o1, D0, D1, acc, rows * n, ell, K, Lq, cP, pinv, pmod, qlinv, scr, 1)
            assert np.array_equal(np.stack([D.down(o0, (l, n)), D.down(o1, (l, n))]), first["mdrs"]), \
                "modup_inner fold + moddown_rescale row_done 2^16"
            assert D.call("sfp_modup_inner", acc, acc1, IN, ell, K, Lq, alpha, cv, KEY, None, None, 0, 0, ell,
                          E, scr) == 0
            D.call("sfp_moddown2", o0, o1, acc, rows * n, ell, K, Lq, cP, pinv, 0, 0, scr, 1)
            assert np.array_equal(D.down(o1, (ell, n)), first["moddown2"][1]), "modup_inner + moddown2 row_done 2^16"
        D.call("sfp_sync")
        for c in cj + [cP]:
            D.call("sfp_free_conv", c)
        D.release()
        outs.append(res)
    for res in outs[1:]:
        for k in res:
            assert np.array_equal(res[k], outs[0][k]), "%s at 2^16: the libraries differ" % k
    return fused
