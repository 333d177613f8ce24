"""sfp_decode_batch (k_dec_load / k_dec_tile / k_dec_stage) and sfp_encode / sfp_encode_batch
(k_enc_load / k_enc_stage / k_enc_tile / k_enc_round) against exact integers and against the
canonical embedding in extended precision -- references that share nothing with
core/encoder.cpp, the oracle's C restatement of it, or the kernels.

The embedding (S slots, n the ring, gap = n / 2S, w = exp(2 pi i / 4S)):

    z_j = sum_{i<S} v_i w^((i 5^j) mod 4S),   v_i = (c[i gap] + i c[n/2 + i gap]) / scale
    v_i = (1/S) sum_j z_j conj(w^((i 5^j) mod 4S))          (E^H E = S I: see embed_ref)

evaluated directly, O(S^2), with integer-exact exponents: in mpmath (100 bits) for S <= 8 and
in np.longdouble (64-bit mantissa, unit roots rounded from mpmath) above; the longdouble route
is checked against mpmath at S = 2 and 8, and its own worst-case error (S + 4) 2^-64 sum|v| is
added to every bound below (REF_ERR).

The tables handed to sfp_encode_setup are this file's own: rot[j] = 5^j mod 2n and ksi[k] the
float64 NEAREST to exp(2 pi i k / 2n) (rounded from mpmath, so each entry is within half an ulp,
which the bound below assumes).

The bound (u = 2^-53).  decButterfly forms w = b k as (bx kx - by ky, bx ky + by kx) without
FMA, then a + w and a - w.  With |k| = 1: each of the two components of w has two product
roundings and one of the subtraction/addition, |err_re| <= u (|bx kx| + |by ky|) + u |w_re| and
likewise for im; the vector (|bx||kx| + |by||ky|, |bx||ky| + |by||kx|) has norm at most
sqrt(2) |b|, so the product's rounding is at most (1 + sqrt 2) u |b|; a table entry within half
an ulp per component moves k by at most u, so w by u |b|; each output a +- w is rounded once, u
|a +- w|.  A node of stage s is a sum of 2^s inputs times unit factors, so its modulus is at
most A = the sum of those |v_i|, and |b| <= A(b) <= A(out).  Inherited errors add (|k| = 1).
Hence err(out) <= err(a) + err(b) + (3 + sqrt 2) u A(out), and by induction over the stages

    |got_j - z_j| <= (3 + sqrt 2) log2(S) u sum_i |v_i|          (first order in u).

C_BFLY = 4.5 >= 3 + sqrt 2 = 4.4142 leaves 2 % for the terms of second order (which are below
1e-13 of the first).  The inverse transform's butterfly (u = a + b; w = (a - b) k) has the same
operations -- one subtraction, the same product, one addition -- and the same induction, then
the exact division by S: |u_i - u_exact_i| <= C_BFLY log2(S) u sum_j |z_j| / S =: E.  The
coefficient is rint(fl(u_i scale)), so against round(scale u_exact) it may differ by

    B = 1 + ceil(scale (E + u (|u_exact_i| + E)))

(the 1: two roundings to an integer, half each; u (...): the product with the scale).

A float64 numpy restatement of each kernel chain's stage order is part of this file
(restate_decode / restate_encode).  The CPU tests hold it to the bounds on every input and show
that a restatement with ONE twiddle index off by one in ONE butterfly, or one stage's rot mask a
bit short, leaves them -- so the bounds and inputs would see such a kernel.  Achieved on the
device: bit equality with the restatements (they are operation for operation), asserted next to
the bound.

Exact part (slots = 1, no stage): output b is (float(c0) / scale, float(c_{n/2}) / scale) with c
the centred CRT lift -- Python's float(int) is the single round-to-nearest-even that
decU128ToDouble claims.  Values: see lift_values.  With primes of at most 60 bits the lift is
below 2^119, so `hi` never has fewer than 9 leading zeros: the all-ones `hi` is taken at the
smallest reachable lz instead of lz = 1.
"""
import ctypes as C
import math
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prims_cases as K  # noqa: E402
import prims_harness as H  # noqa: E402
from prims_harness import u64  # noqa: E402


U = 2.0 ** -53
C_BFLY = 4.5
LD = np.longdouble
FILLS = ((1 << 64) - 1, 1 << 63)  # words >= every prime, for coefficients that are not read
DEC_FILL = -7.25


# --------------------------------------------------------------------------------------------
# tables and the extended-precision embedding

_tables = {}


def tables(logn):
    """rot (uint64 [n/2]), ksi (float64 [2n + 1, 2], nearest), unit roots in longdouble [2n]"""
    if logn not in _tables:
        n = 1 << logn
        M = 2 * n
        rot = np.array([pow(5, j, M) for j in range(n // 2)], dtype=np.uint64)
        ksi = np.zeros((M + 1, 2), dtype=np.float64)
        ld = np.zeros(M + 1, dtype=np.clongdouble)
        with mp.workprec(100):
            for k in range(M + 1):
                a = 2 * mp.pi * k / M
                parts = []
                for x in (mp.cos(a), mp.sin(a)):
                    if k % (M // 4) == 0:  # the axes, exactly
                        x = mp.mpf(round(x))
                    hi = float(x)
                    parts.append((hi, float(x - hi)))
                ksi[k] = (parts[0][0], parts[1][0])
                ld[k] = complex(0) + (LD(parts[0][0]) + LD(parts[0][1])) + 1j * (LD(parts[1][0]) + LD(parts[1][1]))
        _tables[logn] = (rot, ksi, ld[:M])
    return _tables[logn]


def embed_ref(V, S, logn, inverse=False):
    """The embedding (or its inverse) of the columns of V [S, m], in longdouble, O(S^2).
    Inverse: for d = i' - i != 0 write d = 2^a d', d' odd; w^d has order N = 4S / 2^a >= 8 and
    5^j runs 2^a times over {h = 1 mod 4} mod N, where sum_h rho^(d' h) = rho^d' sum_m
    rho^(4 d' m) = 0 -- so E^H E = S I."""
    n = 1 << logn
    T = tables(logn)[2]
    step = (2 * n) // (4 * S)
    V = np.asarray(V, dtype=np.clongdouble).reshape(S, -1)
    p5 = np.array([pow(5, j, 4 * S) for j in range(S)], dtype=np.int64)
    i = np.arange(S, dtype=np.int64)
    out = np.zeros_like(V)
    for r0 in range(0, S, 256):
        r1 = min(S, r0 + 256)
        if inverse:  # rows: coefficient i, columns: slot j
            W = np.conj(T[(i[r0:r1, None] * p5[None, :] % (4 * S)) * step])
        else:  # rows: slot j, columns: coefficient i
            W = T[(p5[r0:r1, None] * i[None, :] % (4 * S)) * step]
        out[r0:r1] = W @ V
    return out / LD(S) if inverse else out


def embed_mp(v, S, inverse=False):
    """the same sums in mpmath at 100 bits; v: S complex numbers (exact doubles)"""
    with mp.workprec(100):
        w = [mp.expjpi(mp.mpf(k) / (2 * S)) for k in range(4 * S)]
        vv = [mp.mpc(float(x.real), float(x.imag)) for x in v]
        out = []
        for a in range(S):
            if inverse:
                out.append(sum(vv[j] * mp.conj(w[a * pow(5, j, 4 * S) % (4 * S)]) for j in range(S)) / S)
            else:
                out.append(sum(vv[i] * w[i * pow(5, a, 4 * S) % (4 * S)] for i in range(S)))
        return [complex(x) for x in out], out


def ref_err(S, sumabs):
    """worst case of embed_ref's own rounding (a longdouble dot product of S terms)"""
    return (S + 4) * 2.0 ** -64 * sumabs


def dec_bound(S, sumabs):
    return C_BFLY * math.log2(S) * U * sumabs


def enc_E(S, sumabs):
    return C_BFLY * math.log2(S) * U * sumabs / S


def enc_B(S, scale, sumabs, uabs):
    E = enc_E(S, sumabs) + ref_err(S, sumabs) / S
    return 1 + math.ceil(scale * (E + U * (uabs + E)))


# --------------------------------------------------------------------------------------------
# the kernels' stage order, restated in float64 numpy (no FMA: every product is rounded)

def brev_perm(S):
    logS = S.bit_length() - 1
    return np.array([H.brev(i, logS) if logS else 0 for i in range(S)], dtype=np.int64)


def _twiddles(S, ln, logn, inverse, mutate):
    """kx, ky [blocks, ln / 2] of stage `ln`.  mutate = ("idx", ln, block, j): that butterfly's
    table index + 1; ("mask", ln): the stage's rot mask one bit short."""
    rot, ksi, _ = tables(logn)
    M, lenh, lenq = 2 << logn, ln >> 1, ln << 2
    mask = lenq - 1
    if mutate and mutate[0] == "mask" and mutate[1] == ln:
        mask = (lenq >> 1) - 1
    r = rot[:lenh].astype(np.int64) & mask
    idx = ((lenq - r) if inverse else r) * (M // lenq)
    idx = np.broadcast_to(idx, (S // ln, lenh)).copy()
    if mutate and mutate[0] == "idx" and mutate[1] == ln:
        idx[mutate[2], mutate[3]] += 1
    return ksi[idx, 0], ksi[idx, 1]


def restate_decode(v, S, logn, mutate=None):
    """k_dec_load's bit reversal, then stages 2, 4, .., S of decButterfly"""
    x = np.zeros(S, dtype=np.complex128)
    x[brev_perm(S)] = v
    re, im = x.real.copy(), x.imag.copy()
    ln = 2
    while ln <= S:
        lenh = ln >> 1
        kx, ky = _twiddles(S, ln, logn, False, mutate)
        R, I = re.reshape(-1, ln), im.reshape(-1, ln)
        ax, ay, bx, by = R[:, :lenh], I[:, :lenh], R[:, lenh:], I[:, lenh:]
        wre = bx * kx - by * ky
        wim = bx * ky + by * kx
        re = np.concatenate([ax + wre, ax - wre], axis=1).ravel()
        im = np.concatenate([ay + wim, ay - wim], axis=1).ravel()
        ln <<= 1
    return re + 1j * im


def restate_encode(z, S, logn, mutate=None):
    """stages S, S/2, .., 2 of encButterfly, then k_enc_round's bit reversal and division"""
    z = np.asarray(z, dtype=np.complex128)
    re, im = z.real.copy(), z.imag.copy()
    ln = S
    while ln >= 2:
        lenh = ln >> 1
        kx, ky = _twiddles(S, ln, logn, True, mutate)
        R, I = re.reshape(-1, ln), im.reshape(-1, ln)
        ax, ay, bx, by = R[:, :lenh], I[:, :lenh], R[:, lenh:], I[:, lenh:]
        dre, dim = ax - bx, ay - by
        wre = dre * kx - dim * ky
        wim = dre * ky + dim * kx
        re = np.concatenate([ax + bx, wre], axis=1).ravel()
        im = np.concatenate([ay + by, wim], axis=1).ravel()
        ln >>= 1
    p = brev_perm(S)
    return (re[p] + 1j * im[p]) / float(S)


def enc_coeffs(u, scale):
    """k_enc_round: rint(q * scale) per component, as Python integers"""
    return [int(np.rint(x * scale)) for x in u.real], [int(np.rint(x * scale)) for x in u.imag]


# --------------------------------------------------------------------------------------------
# inputs

DEC_SHAPES = [(12, 2), (12, 8), (12, 2048), (13, 2048), (13, 4096)]
ENC_SLOTS = [1, 8, 2048]


def dec_inputs(S):
    """name -> (complex integer coefficients [S] as float64 pairs, scale)"""
    out = {}
    for pos in sorted({0, 1, S - 1}):
        for half, val in (("re", 3.0), ("im", 3.0j)):
            v = np.zeros(S, dtype=np.complex128)
            v[pos] = val
            out["delta_%s%d" % (half, pos)] = (v, 1.0)
    out["ones"] = (np.ones(S) + 1j * np.ones(S), 1.0)
    alt = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    out["alt"] = (alt - 1j * alt, 1.0)
    rng = np.random.default_rng(S)
    uni = lambda: rng.integers(-(1 << 40), (1 << 40) + 1, S).astype(np.float64)
    out["uniform"] = (uni() + 1j * uni(), 2.0 ** 30)
    if S > 2048:  # energy in ONE 2048-value tile of k_dec_tile (brev(i) < S / 2: i even)
        v = uni() + 1j * uni()
        v[1::2] = 0
        out["onetile"] = (v, 2.0 ** 30)
    return out


_dec_ref = {}


def dec_reference(logn, S):
    """names, V [S, m] (the v_i = c / scale, exact doubles), Z = embed_ref(V), sum|v| per input"""
    if (logn, S) not in _dec_ref:
        ins = dec_inputs(S)
        names = list(ins)
        V = np.stack([ins[k][0] / ins[k][1] for k in names], axis=1)
        _dec_ref[logn, S] = (names, ins, V, embed_ref(V, S, logn), np.abs(V).sum(axis=0))
    return _dec_ref[logn, S]


def enc_inputs(S, real):
    """name -> (values (fewer than S where S > 1: the rest is zero padding), scale)"""
    rng = np.random.default_rng(1000 + S + real)
    nv = max(1, S - S // 4 - 1) if S > 1 else 1
    cx = (lambda a: a) if real else (lambda a: a + 1j * np.roll(a, 1)[::-1])
    out = {"zero": (cx(np.zeros(nv)), 2.0 ** 40)}
    d = np.zeros(nv)
    d[0] = 1.0
    out["plus1"] = (cx(d), 2.0 ** 40)
    d = np.zeros(nv)
    d[nv - 1] = -1.0
    out["minus1"] = (cx(d), 2.0 ** 40)
    out["mask"] = (cx((rng.random(nv) < 0.5).astype(np.float64)), 2.0 ** 40)
    out["uniform"] = (cx(rng.uniform(-1.0, 1.0, nv)), 2.0 ** 40)
    out["mag255"] = (cx(255.0 * rng.choice([-1.0, 1.0], nv)), 2.0 ** 40)
    if S == 1:
        ps = H.prime_set(12)
        lim = 2.0e18 / 2.0 ** 59  # |value| scale < 2e18: the stated limit; |c| ~ 2^60.8
        out["limit+"] = (cx(np.array([np.nextafter(lim, 0.0)])), 2.0 ** 59)
        out["limit-"] = (cx(np.array([-np.nextafter(lim, 0.0)])), 2.0 ** 59)
        # negative multiples of a row's prime: the residue 0 must stay 0, not become q
        out["-q30"] = (cx(np.array([-float(ps[1])])), 1.0)
        out["-3q42"] = (cx(np.array([-3.0 * ps[2]])), 1.0)
        out["+q30"] = (cx(np.array([float(ps[1])])), 1.0)
    return out


def pad(vals, S):
    z = np.zeros(S, dtype=np.complex128)
    z[:len(vals)] = vals
    return z


_enc_ref = {}


def enc_reference(S, real, logn=12):
    """names, inputs, Zpad [S, m], Uex = the exact inverse embedding [S, m] (longdouble)"""
    if (S, real) not in _enc_ref:
        ins = enc_inputs(S, real)
        names = list(ins)
        Z = np.stack([pad(ins[k][0], S) for k in names], axis=1)
        _enc_ref[S, real] = (names, ins, Z, embed_ref(Z, S, logn, inverse=True))
    return _enc_ref[S, real]


def rounded(x):
    """round half to even of a longdouble, as a Python integer (|x| < 2^63)"""
    r = np.rint(x)
    hi = float(r)
    return int(hi) + int(float(r - LD(hi)))


# --------------------------------------------------------------------------------------------
# unmarked: the references check themselves, the restatements and the oracle's encoder


def test_tables_are_unit_roots_to_half_an_ulp():
    rot, ksi, ld = tables(12)
    assert rot[0] == 1 and rot[1] == 5 and rot[7] == pow(5, 7, 8192)
    assert np.array_equal(ksi[0], [1.0, 0.0]) and np.array_equal(ksi[2048], [0.0, 1.0])
    assert np.array_equal(ksi[8192], [1.0, 0.0])
    err = np.abs(ld.real - ksi[:-1, 0].astype(LD)) / np.maximum(np.abs(ld.real), LD(1e-300))
    assert float(err.max()) <= U * (1 + 2.0 ** -9)
    assert float(np.abs(np.abs(ld) - 1).max()) < 2.0 ** -62


@pytest.mark.parametrize("S", [2, 8])
def test_longdouble_route_matches_mpmath(S):
    rng = np.random.default_rng(S)
    v = rng.integers(-(1 << 40), 1 << 40, S) + 1j * rng.integers(-(1 << 40), 1 << 40, S)
    sumabs = float(np.abs(v).sum())
    for inverse in (False, True):
        got = embed_ref(v.reshape(S, 1), S, 12, inverse)[:, 0]
        _, want = embed_mp(v, S, inverse)
        for g, w in zip(got, want):
            with mp.workprec(100):
                gm = mp.mpc(mp.mpf(float(g.real)) + mp.mpf(float(g.real - LD(float(g.real)))),
                            mp.mpf(float(g.imag)) + mp.mpf(float(g.imag - LD(float(g.imag)))))
                assert abs(gm - w) <= ref_err(S, sumabs) / (S if inverse else 1)
    back = embed_ref(embed_ref(v.reshape(S, 1), S, 12), S, 12, inverse=True)[:, 0]
    assert float(np.abs(back - v).max()) <= 4 * ref_err(S, sumabs)


@pytest.mark.parametrize("logn,S", DEC_SHAPES)
def test_decode_restatement_within_the_bound_and_mutants_outside(logn, S):
    names, ins, V, Z, sumabs = dec_reference(logn, S)
    worst = 0.0

    def ratios(mutate):
        out = []
        for c, k in enumerate(names):
            got = restate_decode(V[:, c], S, logn, mutate)
            err = float(np.abs(got.astype(np.clongdouble) - Z[:, c]).max())
            out.append(err / (dec_bound(S, sumabs[c]) + ref_err(S, sumabs[c])))
        return out

    worst = max(ratios(None))
    assert worst <= 1.0, worst
    print("decode restatement S=%d: largest error / bound = %.4f" % (S, worst))
    last = S  # the last stage; for S = 8 it is the first whose mask matters
    mutants = [("idx", 2, (S // 2) // 2, 0), ("idx", last, 0, (last // 2) - 1)]
    if S >= 8:
        mutants += [("mask", last)]
        if S > 2048:
            mutants += [("mask", 2048), ("idx", 2048, 1, 5)]
    for mu in mutants:
        assert max(ratios(mu)) > 1.0, mu


@pytest.mark.parametrize("real", [1, 0], ids=["real", "complex"])
@pytest.mark.parametrize("S", ENC_SLOTS)
def test_encode_restatement_within_B_and_mutants_outside(S, real):
    names, ins, Z, Uex = enc_reference(S, real)

    def worst(mutate):
        w = 0.0
        for c, k in enumerate(names):
            scale = ins[k][1]
            sumabs = float(np.abs(Z[:, c]).sum())
            cre, cim = enc_coeffs(restate_encode(Z[:, c], S, 12, mutate), scale)
            for i in range(S):
                for got, ue in ((cre[i], Uex[i, c].real), (cim[i], Uex[i, c].imag)):
                    w = max(w, abs(got - rounded(ue * LD(scale))) / enc_B(S, scale, sumabs, abs(float(ue))))
        return w

    assert worst(None) <= 1.0
    if S > 1:
        for mu in [("idx", 2, (S // 2) // 2, 0), ("idx", S, 0, S // 2 - 1)] + ([("mask", S)] if S >= 8 else []):
            assert worst(mu) > 1.0, mu


def engine_tables(logn):
    """core/encoder.cpp's own table formula in float64 (what an engine context uploads)"""
    n = 1 << logn
    M = 2 * n
    ksi = np.array([[math.cos(2.0 * math.pi * k / M), math.sin(2.0 * math.pi * k / M)] for k in range(M + 1)])
    return tables(logn)[0], ksi


def codec_dev(lib, tag, primes, logn, own_tables=True):
    D = H.dev(lib, tag + ("" if own_tables else "-engine-tables"), primes, logn)
    rot, ksi = (tables(logn)[:2] if own_tables else engine_tables(logn))
    f = D.lib.sfp_encode_setup
    f.restype, f.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p]
    rot, ksi = np.ascontiguousarray(rot), np.ascontiguousarray(ksi)
    f(D.d, rot.ctypes.data_as(C.c_void_p), ksi.ctypes.data_as(C.c_void_p))
    D.check()
    return D


def encode_batch(D, vals_list, real, S, scale, m, stride, fill):
    """count = len(vals_list) encodings (one value count); returns the words [count, stride]"""
    count, nv = len(vals_list), len(vals_list[0])
    flat = np.concatenate([np.asarray(v, dtype=np.complex128).real if real else
                           np.asarray(v, dtype=np.complex128).view(np.float64) for v in vals_list])
    flat = np.ascontiguousarray(flat, dtype=np.float64)
    dst = D.alloc(count * stride, fill=fill)
    scratch = D.alloc(count * 2 * S + 2)
    if count == 1:
        f = D.lib.sfp_encode
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_double, H.Limbs,
                      C.c_void_p]
        f(D.d, dst, flat.ctypes.data_as(C.c_void_p), nv, real, S, scale, m, scratch)
    else:
        f = D.lib.sfp_encode_batch
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32,
                      C.c_double, H.Limbs, C.c_void_p]
        f(D.d, dst, stride, flat.ctypes.data_as(C.c_void_p), nv, count, real, S, scale, m, scratch)
    D.check()
    return D.down(dst, (count, stride)), dst


def lift2(a0, a1, q0, q1):
    """the centred CRT lift of (a0 mod q0, a1 mod q1)"""
    x = a0 + q0 * ((a1 - a0) * pow(q0, -1, q1) % q1)
    return x - q0 * q1 if x > (q0 * q1) // 2 else x


def check_encoding(Ds, S, real, logn=12):
    """Assertions 1 and 2 of the encoder on every library of Ds, and equal words between them.
    Returns per input name the coefficient integers (re list, im list)."""
    names, ins, Z, Uex = enc_reference(S, real)
    n, R = 1 << logn, H.ring(H.prime_set(logn), logn)
    gap = (n // 2) // S
    coeffs = {}
    by_scale = {}
    for k in names:
        by_scale.setdefault(ins[k][1], []).append(k)
    groups = [g[i:i + 3] for g in by_scale.values() for i in range(0, len(g), 3)]
    for mname in ("ident", "stride"):
        m = K.maps9()[mname]
        pr = [R.primes[p] for p in m.primes()]
        stride = (m.count + 1) * n
        for g in groups:
            scale = ins[g[0]][1]
            words = [encode_batch(D, [ins[k][0] for k in g], real, S, scale, m, stride, FILLS[1])[0] for D in Ds]
            for w in words[1:]:
                assert np.array_equal(w, words[0]), "the libraries' residues differ: %s %s" % (mname, g)
            for b, k in enumerate(g):
                rows = words[0][b, :m.count * n].reshape(m.count, n)
                assert (words[0][b, m.count * n:] == FILLS[1]).all(), "the fill between row sets was written"
                on = np.zeros(n, dtype=bool)
                on[np.arange(S) * gap] = on[n // 2 + np.arange(S) * gap] = True
                assert not rows[:, ~on].any(), "a coefficient off the gap lattice is not 0"
                if mname == "ident":  # the integer: CRT of the two 60-bit rows (primes 0 and 6)
                    cre = [lift2(int(rows[0, i * gap]), int(rows[6, i * gap]), pr[0], pr[6]) for i in range(S)]
                    cim = [lift2(int(rows[0, n // 2 + i * gap]), int(rows[6, n // 2 + i * gap]), pr[0], pr[6])
                           for i in range(S)]
                    c = list(names).index(k)
                    sumabs = float(np.abs(Z[:, c]).sum())
                    for i in range(S):
                        for got, ue in ((cre[i], Uex[i, c].real), (cim[i], Uex[i, c].imag)):
                            B = enc_B(S, scale, sumabs, abs(float(ue)))
                            assert abs(got - rounded(ue * LD(scale))) <= B, (k, i, got, B)
                    coeffs[k] = (cre, cim)
                cre, cim = coeffs[k]
                for r, q in enumerate(pr):  # every row is the residue of that one integer
                    want = np.zeros(n, dtype=object)
                    want[np.arange(S) * gap] = [x % q for x in cre]
                    want[n // 2 + np.arange(S) * gap] = [x % q for x in cim]
                    H.assert_eq(rows[r], want, "encode %s %s row %d (prime %d)" % (mname, k, r, q))
            for D in Ds:
                D.release()
    # sfp_encode is one row set of the batch
    m = K.maps9()["ident"]
    for D in Ds:
        k = names[-1]
        one = encode_batch(D, [ins[k][0]], real, S, ins[k][1], m, m.count * n, 0)[0][0].reshape(m.count, n)
        for r, q in enumerate(R.primes):
            assert [int(x) for x in one[r, np.arange(S) * gap]] == [x % q for x in coeffs[k][0]]
        D.release()
    return coeffs


@pytest.mark.parametrize("real", [1, 0], ids=["real", "complex"])
@pytest.mark.parametrize("S", ENC_SLOTS)
def test_oracle_encoder_is_consistent_and_close(oracle_lib, S, real):
    D = codec_dev(oracle_lib, "oracle-codec", H.prime_set(12), 12)
    coeffs = check_encoding([D], S, real)
    if S == 1:
        q30 = H.prime_set(12)[1]
        assert coeffs["-q30"][0] == [-q30] and coeffs["limit-"][0][0] < -(1 << 60)


def test_embedding_convention_is_the_engines(oracle_lib):
    """The pin of slot order and index convention: the oracle's encoder (bit-identical to the
    engine's, test_encode.py) under the engine's own table formula gives coefficients whose
    embedding by embed_ref is the value vector, in order, and is what the oracle engine decrypts
    from a fresh encryption of it to within the encryption noise (1e-4: test_gpu_decode.py)."""
    import sfhe
    S, scale = 8, 2.0 ** 40
    v = np.array([1.5, -2.25, 3.125, 4.0, -5.5, 6.75, 7.0, -8.875])
    D = codec_dev(oracle_lib, "oracle-codec", H.prime_set(12), 12, own_tables=False)
    m, n = H.ident(1), 1 << 12
    row = encode_batch(D, [v], 1, S, scale, m, n, 0)[0][0]
    D.release()
    q0, gap = D.primes[0], n // 2 // S
    cen = lambda a: int(a) - q0 if int(a) > q0 // 2 else int(a)
    c = np.array([cen(row[i * gap]) + 1j * cen(row[n // 2 + i * gap]) for i in range(S)]) / scale
    z = embed_ref(c.reshape(S, 1), S, 12)[:, 0]
    assert float(np.abs(z - v).max()) < 1e-9
    e = sfhe.Engine("oracle", mult_depth=2, ring_dim=n, batch_size=8, seed=5)
    dec = np.array(e.decrypt(e.encrypt(v.tolist(), S, 0)))
    e.close()
    assert float(np.abs(z.real.astype(np.float64) - dec).max()) < 1e-4
    assert float(np.abs(np.roll(v, 1) - dec).max()) > 1.0  # (a rotated order would not pass)


# --------------------------------------------------------------------------------------------
# the exact part of the decoder: lift, centring and the one rounding


def lift_primes(logn, which):
    m = 2 << logn
    p60 = H.prime_below(1 << 60, m)
    p60b = H.prime_below(p60, m)
    p30 = H.prime_below(1 << 30, m)  # the smallest size the context accepts
    return {"60x60": [p60, p60b], "30x60": [p30, p60], "60x30": [p60, p30]}[which]


def lift_values(q0, q1, nl):
    """Chosen lifts x in [0, Q), each with Q - x: 0, 1, q0 - 1, q0, Q/2 - 1, Q/2, Q/2 + 1, Q - 1
    (for nl = 1 Q = q0: its half and neighbours); for every k from 53 up to the bit length of
    Q/2 and both mantissa parities m, 2^k + m 2^(k-52) + h with h = the tie 2^(k-53), its two
    neighbours, and (k > 64) the tie plus the top bit of what `lo << lz` keeps; the all-ones
    pattern at the smallest reachable lz; 2^64, 2^64 + 1, 2^65 - 1 (lz = 63 and 62).
    Returns (values, the set of (k, m) the ties cover)."""
    Q = q0 * q1 if nl == 2 else q0
    half = Q // 2
    xs = [0, 1, q0 - 1, q0, half - 1, half, half + 1, Q - 1]
    L = half.bit_length()
    cover = set()
    for k in range(53, L + 1):
        t = 1 << (k - 53)
        for mpar in (0, 1):
            for h in [t - 1, t, t + 1] + ([t + (1 << (k - 64))] if k > 64 else []):
                x = (1 << k) + mpar * (1 << (k - 52)) + h
                if x <= half:
                    xs.append(x)
                    cover.add((k, mpar))
    xs += [(1 << (L - 1)) - 1, 1 << 64, (1 << 64) + 1, (1 << 65) - 1]
    xs = [x for x in xs if 0 <= x < Q]
    return xs + [Q - x for x in xs if x], cover, L


def test_tie_set_covers_every_exponent_and_parity():
    for which, nl in (("60x60", 2), ("30x60", 2), ("60x30", 2), ("60x60", 1), ("30x60", 1)):
        q0, q1 = lift_primes(12, which)
        xs, cover, L = lift_values(q0, q1, nl)
        assert cover == {(k, mpar) for k in range(53, L) for mpar in (0, 1)}, which
        if nl == 2 and which == "60x60":
            assert L == 119 and len(xs) > 800
        # both kinds of tie are there: round down to the even mantissa, up to the even mantissa
        if L > 54:
            assert float((1 << 60) + (1 << 7)) == float(1 << 60) and float((1 << 60) + 3 * (1 << 7)) == float((1 << 60) + (1 << 9))


def decode_batch(D, src, stride, count, nl, S, scales, out):
    f = D.lib.sfp_decode_batch
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    return f(D.d, src, stride, count, nl, S, sc.ctypes.data_as(C.c_void_p), out)


def down_f64(D, p, shape):
    return D.down(p, shape).view(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("logn,which,nl", [(12, "60x60", 2), (12, "30x60", 2), (12, "60x30", 2), (12, "60x60", 1),
                                           (12, "30x60", 1), (13, "60x60", 2), (13, "60x60", 1)])
def test_decode_lift_centring_and_rounding_exact(hip_lib, logn, which, nl):
    primes = lift_primes(logn, which)
    D = codec_dev(hip_lib, "hip-codec", primes, logn)
    assert D.has("sfp_decode_batch")
    n = 1 << logn
    q0, q1 = primes
    Q = q0 * q1 if nl == 2 else q0
    xs, _, _ = lift_values(q0, q1, nl)
    if len(xs) % 2:
        xs.append(0)
    count = len(xs) // 2
    assert 4 <= count <= 65535
    cen = [x - Q if x > Q // 2 else x for x in xs]
    stride = nl * n
    out = D.alloc(2 * count)
    results = {}
    for fill in FILLS:
        src = np.full((count, nl, n), fill, dtype=np.uint64)
        for r, q in enumerate(primes[:nl]):
            src[:, r, 0] = u64([x % q for x in xs[0::2]])
            src[:, r, n // 2] = u64([x % q for x in xs[1::2]])
        P = D.up(src)
        for sname, scale in (("one", 1.0), ("2^50", 2.0 ** 50), ("odd", 1099511627776.5)):
            if fill != FILLS[0] and sname != "odd":
                continue
            D.put(out, np.full(2 * count, DEC_FILL, dtype=np.float64).view(np.uint64))
            assert decode_batch(D, P, stride, count, nl, 1, [scale] * count, out) == 0
            D.check()
            got = down_f64(D, out, (2 * count,))
            want = np.array([float(c) / scale for c in cen], dtype=np.float64)
            bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
            assert not len(bad), "%d of %d differ; first: x = %d, got %r, exact %r (scale %s)" % (
                len(bad), len(xs), xs[bad[0]], got[bad[0]], want[bad[0]], sname)
            results[fill, sname] = got
    assert np.array_equal(results[FILLS[0], "odd"].view(np.uint64), results[FILLS[1], "odd"].view(np.uint64))
    D.release()


@pytest.mark.gpu
def test_decode_refused_shapes(hip_lib):
    """slots 0, 3, above n/2, nl 0 and 3: an error is recorded, 0 returned, nothing launched;
    `out` keeps its fill and sfp_clear_error clears the device error."""
    D = codec_dev(hip_lib, "hip-codec", lift_primes(12, "60x60"), 12)
    n = 1 << 12
    src = D.up(np.zeros(2 * n, dtype=np.uint64))
    fill = np.full(2 * n, DEC_FILL, dtype=np.float64).view(np.uint64)
    out = D.up(fill)
    clear = D.lib.sfp_clear_error
    clear.restype, clear.argtypes = None, [C.c_void_p]
    for slots, nl in ((0, 2), (3, 2), (n, 2), (8, 0), (8, 3)):
        assert decode_batch(D, src, 2 * n, 1, nl, slots, [1.0], out) == 0
        assert D.lib.sfp_last_error(D.d) is not None, (slots, nl)
        clear(D.d)
        D.check()
        assert np.array_equal(D.down(out, (2 * n,)), fill), (slots, nl)
    assert decode_batch(D, src, 2 * n, 1, 2, 8, [1.0], out) == 0  # and a plain call runs: zeros
    D.check()
    assert not down_f64(D, out, (16,)).any()
    D.release()


# --------------------------------------------------------------------------------------------
# the FFT on the device


@pytest.mark.gpu
@pytest.mark.parametrize("logn,S", DEC_SHAPES)
def test_decode_fft_is_the_embedding(hip_lib, logn, S):
    names, ins, V, Z, sumabs = dec_reference(logn, S)
    primes = lift_primes(logn, "60x60")
    D = codec_dev(hip_lib, "hip-codec", primes, logn)
    n, q0 = 1 << logn, primes[0]
    gap, count = n // 2 // S, len(names)
    src = np.full((count, n), FILLS[0], dtype=np.uint64)
    idx = np.arange(S) * gap
    for c, k in enumerate(names):
        v = ins[k][0]
        src[c, idx] = u64([int(x) % q0 for x in v.real])
        src[c, n // 2 + idx] = u64([int(x) % q0 for x in v.imag])
    out = D.alloc(2 * S * count)
    assert decode_batch(D, D.up(src), n, count, 1, S, [ins[k][1] for k in names], out) == 0
    D.check()
    got = down_f64(D, out, (count, S, 2))
    worst = 0.0
    for c, k in enumerate(names):
        g = got[c, :, 0] + 1j * got[c, :, 1]
        err = float(np.abs(g.astype(np.clongdouble) - Z[:, c]).max())
        ratio = err / (dec_bound(S, sumabs[c]) + ref_err(S, sumabs[c]))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k, ratio)
        r = restate_decode(V[:, c], S, logn)
        assert np.array_equal(g.view(np.uint64), r.view(np.uint64)), k + ": not the restatement's bits"
    print("decode device ring 2^%d S=%d: largest error / bound = %.4f" % (logn, S, worst))
    D.release()


@pytest.mark.gpu
@pytest.mark.parametrize("real", [1, 0], ids=["real", "complex"])
@pytest.mark.parametrize("S", ENC_SLOTS)
def test_encode_exact_close_and_round_trip(hip_lib, oracle_lib, S, real):
    primes = H.prime_set(12)
    Dh = codec_dev(hip_lib, "hip-codec", primes, 12)
    Do = codec_dev(oracle_lib, "oracle-codec", primes, 12)
    coeffs = check_encoding([Dh, Do], S, real)  # consistency, closeness, HIP == oracle
    names, ins, Z, Uex = enc_reference(S, real)
    n, m = 1 << 12, H.ident(2)  # rows 0, 1: the 60-bit and the 30-bit prime, as the decoder reads them
    q0, q1 = primes[:2]
    stride = 3 * n
    worstB = worstR = 0.0
    for k in names:
        scale = ins[k][1]
        cre, cim = coeffs[k]
        if max(abs(x) for x in cre + cim) >= (q0 * q1) // 2:
            continue
        c = names.index(k)
        sumz = float(np.abs(Z[:, c]).sum())
        for i in range(S):
            for got, ue in ((cre[i], Uex[i, c].real), (cim[i], Uex[i, c].imag)):
                worstB = max(worstB, abs(got - rounded(ue * LD(scale))) / enc_B(S, scale, sumz, abs(float(ue))))
        u = restate_encode(Z[:, c], S, 12)
        assert enc_coeffs(u, scale) == (cre, cim), k + ": not the restatement's integers"
        words, dst = encode_batch(Dh, [ins[k][0]] * 2, real, S, scale, m, stride, FILLS[0])
        out = Dh.alloc(2 * S * 2)
        assert decode_batch(Dh, dst, stride, 2, 2, S, [scale, scale], out) == 0
        Dh.check()
        got = down_f64(Dh, out, (2, S, 2))
        assert np.array_equal(got[0], got[1])
        g = got[0, :, 0] + 1j * got[0, :, 1]
        v = np.array([float(a) / scale + 1j * (float(b) / scale) for a, b in zip(cre, cim)])
        sumv = float(np.abs(v).sum())
        coeff_err = sum(math.sqrt(2.0) * enc_B(S, scale, sumz, abs(float(Uex[i, c].real)) + abs(float(Uex[i, c].imag)))
                        for i in range(S)) / scale
        bound = (dec_bound(S, sumv) if S > 1 else 0.0) + coeff_err + 2 * U * sumv
        err = float(np.abs(g - Z[:, c]).max())
        worstR = max(worstR, err / bound)
        assert err <= bound, (k, err, bound)
        Dh.release()
    print("encode device S=%d %s: largest |c - round| / B = %.4f, round trip error / bound = %.4f"
          % (S, "real" if real else "complex", worstB, worstR))
