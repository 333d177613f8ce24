"""The sum of m ciphertext products relinearised once (EvalMultSum, the Chebyshev
evaluator's remainder chains) on the CPU oracle.

Prim level: the composed form prims.h names for sfp_multn_relin_rescale_add -- m
sfp_tensor, sfp_add per component, sfp_modup, sfp_ks_inner_fold,
sfp_moddown_rescale, sfp_add of the addend -- against exact Python integers on
chosen residues (tests/prims_harness.py), ring 2^12, m = 1, 2, 3 and the cap.

Engine and series level: values, the conditions that throw, m = 2 against
mult_sum2 residue for residue, both evaluation orders bit for bit
(SFHE_PS_WAVES is read once per process: fresh children), the knob
SFHE_PS_DOT (read per call) and the number of relinearisations it saves, which
chain_savings() derives from the series' degree by restating the evaluator's
tree.
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prims_cases as K  # noqa: E402
import prims_harness as H  # noqa: E402
from prims_harness import assert_eq, ident, u64  # noqa: E402
from test_mult_sum2 import SHAPES, chain_primes  # noqa: E402

import sfhe  # noqa: E402
from oracle import cheb  # noqa: E402

CAP = 8  # SFP_MULT_SUM_MAX = CryptoContextImpl::kMultSumMaxTerms
SPINE_CAP = 6  # the evaluator's kSpineCap
H._SIGS.setdefault("sfp_multn_relin_rescale_add", ("i", "pppuuuuupppppppppppip"))


def sumn_case(devs, ell, kind, m, logn=12, addend=True, exact=True):
    """Every library's composed form, and its fused prim where it has one, against the exact
    integers.  Returns the number of libraries whose fused prim ran.  exact=False (ring 2^16,
    where the Python-integer reference takes 20 to 100 s a case): the reference is the first
    library's composed form, which the ring 2^12 cases hold to the exact integers."""
    ell, Lq, Kp, alpha = SHAPES.get(ell, (ell, ell, 2, (ell + 2) // 3))
    primes = chain_primes(Lq, Kp, logn)
    R = H.ring(primes, logn)
    n, rows, l, beta = R.n, ell + Kp, ell - 1, (ell + alpha - 1) // alpha
    up, down = K.ks_convs(R, ell, Kp, Lq, alpha)
    if exact:
        ops = [H.pattern_polys(R, ident(ell), 70 + i)[kind] for i in range(4 * m)]  # a0 a1 b0 b1 per product
        kb = [H.pattern_polys(R, ident(Lq + Kp), 30 + j)["uniform"] for j in range(beta)]
        ka = [H.pattern_polys(R, ident(Lq + Kp), 40 + j)["uniform"] for j in range(beta)]
    else:  # (generating the patterns is what costs at ring 2^16: one operand and one key pattern, reused)
        ops = [H.pattern_polys(R, ident(ell), 70)[kind]] * (4 * m)
        kb = ka = [H.pattern_polys(R, ident(Lq + Kp), 30)["uniform"]] * beta
    ql, q = H.qcol(R, ident(ell)), H.qcol(R, H.Limbs(rows, ell, Lq, 0, 0))
    kr = list(range(ell)) + [Lq + k for k in range(Kp)]
    P = down.prod
    pinv = u64([pow(P, -1, R.primes[i]) for i in range(ell)])
    pmod = u64([P % R.primes[i] for i in range(ell)])
    qlinv = u64([pow(R.primes[l], -1, R.primes[i]) for i in range(l)])
    fold_k = P % R.primes[l]
    key = np.concatenate([np.concatenate([u64(kb[j]), u64(ka[j])]) for j in range(beta)])
    quad = [ops[4 * i: 4 * i + 4] for i in range(m)]
    r = [H.pattern_polys(R, ident(l), 66)["uniform"], H.pattern_polys(R, ident(l), 67)["qm1"]]
    want = t2 = None
    if exact:
        t0 = sum(a0 * b0 for a0, a1, b0, b1 in quad) % ql
        t1 = sum(a0 * b1 + a1 * b0 for a0, a1, b0, b1 in quad) % ql
        t2 = sum(a1 * b1 for a0, a1, b0, b1 in quad) % ql
        ext = K.exact_modup(R, t2, up, ell, Kp)
        s = [sum(e * k[kr] for e, k in zip(ext, kk)) % q for kk in (kb, ka)]
        want = [K.exact_md_rescale(R, s[p], (t0, t1)[p], down, ell, Kp, Lq, fold_k) for p in range(2)]
        if addend:
            qk = H.qcol(R, ident(l))
            want = [(want[p] + r[p]) % qk for p in range(2)]
    fused = 0
    for D in devs(primes, logn):
        cj = [c.upload(D) for c in up]
        cv, cP = D.ptrs(cj), down.upload(D)
        dev = [D.up(u64(x)) for x in ops]
        KEY, R0, R1 = D.up(key), D.up(u64(r[0])), D.up(u64(r[1]))
        E, scr, acc = D.alloc(beta * rows * n), D.alloc(2 * ell * n), D.alloc(2 * rows * n)
        acc1 = acc + rows * n * 8
        o0, o1 = D.alloc(ell * n), D.alloc(ell * n)
        lm = ident(ell)
        d = [D.alloc(ell * n) for _ in range(6)]
        for i in range(m):
            w = d[3:] if i else d[:3]
            D.call("sfp_tensor", w[0], w[1], w[2], *dev[4 * i: 4 * i + 4], lm)
            if i:
                for c in range(3):
                    D.call("sfp_add", d[c], d[c], d[3 + c], lm)
        if t2 is not None:
            assert_eq(D.down(d[2], (ell, n)), t2, "summed d2 (%s)" % kind)
        D.call("sfp_modup", E, d[2], ell, Kp, Lq, alpha, cv, scr)
        D.call("sfp_ks_inner_fold", acc, acc1, E, rows * n, KEY, beta, ell, Kp, Lq, d[0], d[1], fold_k)
        D.call("sfp_moddown_rescale", o0, o1, d[0], d[1], acc, rows * n, ell, Kp, Lq, cP, pinv, pmod, qlinv, scr, 0)
        if addend:
            D.call("sfp_add", o0, o0, R0, ident(l))
            D.call("sfp_add", o1, o1, R1, ident(l))
        if want is None:
            want = [D.down(o, (l, n)).copy() for o in (o0, o1)]
        for p, o in enumerate((o0, o1)):
            assert_eq(D.down(o, (l, n)), want[p], "composed out%d (ell %d, m %d, %s)" % (p, ell, m, kind))
        if D.has("sfp_multn_relin_rescale_add"):
            D.put(o0, np.zeros(ell * n, dtype=np.uint64))
            D.put(o1, np.zeros(ell * n, dtype=np.uint64))
            rc = D.call("sfp_multn_relin_rescale_add", o0, o1, D.ptrs(dev), m, ell, Kp, Lq, alpha, cv, KEY, cP, pinv,
                        pmod, qlinv, acc, E, scr, R0 if addend else None, R1 if addend else None, 1, None)
            if rc == 0:
                fused += 1
                for p, o in enumerate((o0, o1)):
                    assert_eq(D.down(o, (l, n)), want[p], "fused out%d (ell %d, m %d, %s)" % (p, ell, m, kind))
            else:
                assert rc == -1
        D.call("sfp_sync")
        for c in cj + [cP]:
            D.call("sfp_free_conv", c)
        D.release()
    return fused


@pytest.fixture(scope="module")
def devs(oracle_lib):
    return lambda primes, logn: [H.dev(oracle_lib, "oracle", primes, logn)]


@pytest.mark.parametrize("m", [1, 2, 3, CAP])
@pytest.mark.parametrize("kind", ["uniform", "qm1"])
def test_composed_form_is_exact(devs, m, kind):
    assert sumn_case(devs, 3, kind, m) == 0  # (the oracle has no fused prim)


def test_composed_form_two_digits_without_addend(devs):
    assert sumn_case(devs, 13, "qm1", 3, addend=False) == 0


# ---- engine level ------------------------------------------------------------------


def sha(ct):
    return hashlib.sha256(ct.download().tobytes()).hexdigest()


def test_engine_values_special_cases_and_preconditions(oracle_lib):
    e = sfhe.Engine("oracle", mult_depth=4, ring_dim=1 << 13, batch_size=8, seed=77)
    rng = np.random.default_rng(3)
    vs = [rng.uniform(-1, 1, 8) for _ in range(2 * CAP + 2)]
    cs = [e.encrypt(v.tolist()) for v in vs]
    r = rng.uniform(-1, 1, 8)
    cr = e.encrypt(r.tolist(), level=1)
    e.op_stats(reset=True)
    for m in (1, 2, 3, CAP):
        terms = [(cs[2 * i], cs[2 * i + 1]) for i in range(m)]
        ref = sum(vs[2 * i] * vs[2 * i + 1] for i in range(m))
        # one product's usual error is below 1e-6 (tests/test_mult_sum2.py); m products add up
        assert np.max(np.abs(np.array(e.decrypt(e.mult_sum(terms, cr))) - (ref + r))) < 1e-6 * m
        assert np.max(np.abs(np.array(e.decrypt(e.mult_sum(terms))) - ref)) < 1e-6 * m
    assert e.sumn_counts() == (0, 8) and e.dot_counts() == (0, 0)
    assert sha(e.mult_sum([(cs[0], cs[1]), (cs[2], cs[3])], cr)) == sha(e.mult_sum2(cs[0], cs[1], cs[2], cs[3], cr))
    assert sha(e.mult_sum([(cs[0], cs[1]), (cs[2], cs[3])])) == sha(e.mult_sum2(cs[0], cs[1], cs[2], cs[3]))
    assert sha(e.mult_sum([(cs[0], cs[1])], cr)) == sha(e.add(e.mult(cs[0], cs[1]), cr))
    assert e.dot_counts() == (0, 2)
    with pytest.raises(sfhe.SfheError):
        e.mult_sum([(cs[0], cs[1]), (cs[2], cr)])  # operands at two levels
    with pytest.raises(sfhe.SfheError):
        e.mult_sum([(cs[0], cs[1]), (cs[2], cs[3])], cs[4])  # the addend is not at the result's level
    with pytest.raises(sfhe.SfheError):
        e.mult_sum([(cs[0], cs[1])] * (CAP + 1))  # more terms than the op takes
    # products of two scales: the same rows under another scale label
    other = e.relabel_scale(cs[2], 0.5)
    assert other.level == cs[0].level
    with pytest.raises(sfhe.SfheError, match="different scales"):
        e.mult_sum([(cs[0], cs[1]), (other, cs[3])])
    with pytest.raises(sfhe.SfheError, match="not canonical"):
        e.mult_sum([(cs[0], cs[1])], e.relabel_scale(cr, 0.5))  # the addend at the right level, another scale
    # both factors relabelled so that the products' scales agree: taken
    e.mult_sum([(cs[0], cs[1]), (e.relabel_scale(cs[2], 0.5), e.relabel_scale(cs[3], 2.0))])


def many_case(e, level=0):
    """EvalMultSumMany: batches of 2 and 4 ops of one shape, and ops of different term counts in one
    call, which must go out as separate batches; every result equals the op issued alone."""
    rng = np.random.default_rng(11)
    cs = [e.encrypt(rng.uniform(-1, 1, 8).tolist(), level=level) for _ in range(12)]
    rs = [e.encrypt(rng.uniform(-1, 1, 8).tolist(), level=level + 1) for _ in range(2)]

    def op(m, k, r=None):
        return ([(cs[(k + 2 * i) % 12], cs[(k + 2 * i + 1) % 12]) for i in range(m)], r)

    def alone(o):
        return sha(e.mult_sum(o[0], o[1]))

    for ops, batches in (([op(2, 0, rs[0]), op(2, 1)], 1),
                         ([op(3, 0), op(3, 1, rs[1]), op(3, 2), op(3, 3, rs[0])], 1),
                         ([op(2, 0, rs[0]), op(3, 1)], 2),  # two term counts: two batches
                         ([op(2, 0), op(2, 1), op(3, 2), op(2, 3)], 3)):  # (only consecutive ops share one)
        want = [alone(o) for o in ops]
        e.op_stats(reset=True)
        got = e.mult_sum_many(ops)
        assert e.sumn_batch_counts() == (batches, 0)
        assert sum(e.sumn_counts()) == len(ops)
        assert [sha(g) for g in got] == want
    return e.sumn_counts()


def test_many_batches(oracle_lib):
    e = sfhe.Engine("oracle", mult_depth=4, ring_dim=1 << 13, batch_size=8, seed=78)
    assert many_case(e) == (0, 4)


# ---- the evaluator -----------------------------------------------------------------


def chain_savings(deg, cap=SPINE_CAP):
    """Relinearisations the remainder chains save for a dense series of degree deg evaluated on a
    fresh ciphertext: chebyshev.cpp's tree (build / productLevel / natural / leafSumLevel and the
    choice of l) restated on degrees and levels.  T_j sits at level ceil(log2 j)."""
    ub = [5, 13, 27, 59, 119, 247, 495, 1007, 2031]
    D = 1 if deg <= 1 else 2 if deg == 2 else 3 + next(i for i, u in enumerate(ub) if deg <= u)
    best, bestc = 1, 1e300
    for l in range(1, 7):
        if l + 1 > D or (1 << D) - (1 << l) < deg:
            continue
        c = ((1 << l) - 1) + (D - 1 - l) + -(-deg // (1 << l))
        if c < bestc:
            best, bestc = l, c
    l = min(best, max(deg, 2).bit_length() - 1)
    k = 1 << l

    def lev(j):
        return (j - 1).bit_length()

    def descend(g, depth):
        while depth >= 1 and g + k <= (1 << (depth - 1)):
            depth -= 1
        return depth

    def natural(g, depth):  # g: the degree, -1 or 0 for a constant
        if g <= 0:
            return -1
        if g <= k:
            return lev(g) + 1
        depth = descend(g, depth)
        M = 1 << (depth - 1) if g >= (1 << (depth - 1)) else 1 << (depth - 2)
        return max(plevel(g - M, depth, M, 0), natural(M - 1, depth))

    def plevel(gq, depth, M, want):
        return max(max(natural(gq, depth - 1), lev(M)) + 1, want)

    saved = [0]

    def head(g, depth, want):  # a chain's head: walk it, start its quotients' and its tail's chains
        terms = 0
        Lp0 = None
        while g > k:
            depth = descend(g, depth)
            M = 1 << (depth - 1) if g >= (1 << (depth - 1)) else 1 << (depth - 2)
            Lp = plevel(g - M, depth, M, want)
            if terms and (g - M <= 0 or Lp != Lp0 or terms == cap):
                head(g, depth, want)  # the lower part: an op of its own
                return
            if g - M <= 0:  # a constant quotient: no chain here
                head(M - 1, depth, Lp)
                return
            if not terms:
                Lp0 = Lp
            else:
                saved[0] += 1
            terms += 1
            head(g - M, depth - 1, Lp - 1)
            g, want = M - 1, Lp

    head(deg, D, 0)
    return saved[0]


def test_chain_savings_model():
    # degree 27: six tree products become three; degree 59: eleven become four
    assert chain_savings(27) == 3 and chain_savings(59) == 7


@pytest.mark.parametrize("deg,depth", [(59, 7), (27, 6)])
def test_series_knob_and_relinearisation_count(oracle_lib, monkeypatch, deg, depth):
    e = sfhe.Engine("oracle", mult_depth=depth, ring_dim=1 << 13, batch_size=8, seed=5)
    c = np.random.default_rng(deg).uniform(-1, 1, deg + 1) / deg
    x = np.linspace(-0.95, 0.9, 8)
    cx = e.encrypt(x.tolist())
    out = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("SFHE_PS_DOT", knob)
        e.op_stats(reset=True)
        y = e.chebyshev(cx, c.tolist())
        out[knob] = (sha(y), e.op_stats(), e.sumn_counts())
        assert np.max(np.abs(np.array(e.decrypt(y)) - cheb.cheb_eval(c, x))) < 1e-5
    on, off = out["1"], out["0"]
    assert on[0] != off[0]
    assert off[2] == (0, 0) and on[2][0] == 0 and on[2][1] > 0
    assert e.sumn_batch_counts()[1] == 0  # no chain fell back to separate products
    saved = {59: 7, 27: 3}[deg]
    assert saved == chain_savings(deg)
    assert off[1]["keyswitch"] - on[1]["keyswitch"] == saved
    assert off[1]["rescale"] - on[1]["rescale"] == saved
    assert off[1]["tensor"] == on[1]["tensor"]  # one per term


_CHILD = r"""
import hashlib, json
import numpy as np
import sfhe
out = {}
for deg, depth in ((59, 7), (27, 6)):
    e = sfhe.Engine("oracle", mult_depth=depth, ring_dim=1 << 13, batch_size=8, seed=5)
    c = np.random.default_rng(deg).uniform(-1, 1, deg + 1) / deg
    y = e.chebyshev(e.encrypt(np.linspace(-0.95, 0.9, 8).tolist()), c.tolist())
    out[str(deg)] = [hashlib.sha256(y.download().tobytes()).hexdigest(), e.sumn_counts(), e.op_stats()["keyswitch"]]
print("RESULT " + json.dumps(out))
"""


def _child(**knobs):
    env = dict(os.environ)
    for k in ("SFHE_PS_WAVES", "SFHE_PS_DOT", "SFHE_MULT_SUM_FUSED"):
        env.pop(k, None)
    env.update(knobs)
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(re.search(r"RESULT (.*)", r.stdout).group(1))


def test_evaluation_orders_agree(oracle_lib):
    assert _child() == _child(SFHE_PS_WAVES="0")
