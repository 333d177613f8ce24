"""The sum of two ciphertext products relinearised once (EvalMultSum2, the sign
polynomials' paired products) on the CPU oracle.

Prim level: the composed form prims.h names for sfp_mult2_relin_rescale_add --
sfp_tensor twice, sfp_add per component, sfp_modup, sfp_ks_inner_fold,
sfp_moddown_rescale, sfp_add of the addend -- against exact Python integers on
chosen residues (tests/prims_harness.py), ring 2^12, one digit (ell = 3, one
special prime) and two digits (ell = 13).  The all-(q-1) operands drive the
extra modular addition of every summed component to its largest inputs.

Engine and sign level: decryptions, both issue orders bit for bit, the knob
and the counters.  SFHE_SIGN_BATCH is read once per process, so the issue
orders run in fresh children; SFHE_SIGN_DOT is read per call.
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

import sfhe  # noqa: E402

LOGN = 12
# (ell, Lq, K, alpha): one digit with one special prime; two digits (7 + 6 rows) with two
SHAPES = {3: (3, 4, 1, 3), 13: (13, 13, 2, 7)}
H._SIGS.setdefault("sfp_mult2_relin_rescale_add", ("i", "ppppppppppuuuupppppppppppip"))


def chain_primes(Lq, Kp, logn=LOGN):
    """q_0 of 60 bits, the other q rows below 2^42 (FP64 rows on the device), P rows below 2^60."""
    m = 2 << logn
    out = [H.prime_below(1 << 60, m)]
    b = H.FP_BOUND
    for _ in range(Lq - 1):
        b = H.prime_below(b, m)
        out.append(b)
    b = out[0]
    for _ in range(Kp):
        b = H.prime_below(b, m)
        out.append(b)
    assert len(set(out)) == Lq + Kp
    return out


def sum2_case(devs, ell, kind, logn=LOGN, addend=True):
    """Every library's composed form, and its fused prim where it has one, against the exact
    integers.  Returns the number of libraries whose fused prim ran."""
    ell, Lq, Kp, alpha = SHAPES.get(ell, (ell, ell, 2, (ell + 2) // 3))
    primes = chain_primes(Lq, Kp, logn)
    R = H.ring(primes, logn)
    n, rows, l, beta = R.n, ell + Kp, ell - 1, (ell + alpha - 1) // alpha
    up, down = K.ks_convs(R, ell, Kp, Lq, alpha)
    ops = [H.pattern_polys(R, ident(ell), 70 + i)[kind] for i in range(8)]  # a0 a1 b0 b1 c0 c1 e0 e1
    a0, a1, b0, b1, c0, c1, e0, e1 = ops
    kb = [H.pattern_polys(R, ident(Lq + Kp), 30 + j)["uniform"] for j in range(beta)]
    ka = [H.pattern_polys(R, ident(Lq + Kp), 40 + j)["uniform"] for j in range(beta)]
    ql, q = H.qcol(R, ident(ell)), H.qcol(R, H.Limbs(rows, ell, Lq, 0, 0))
    kr = list(range(ell)) + [Lq + k for k in range(Kp)]
    P = down.prod
    pinv = u64([pow(P, -1, R.primes[i]) for i in range(ell)])
    pmod = u64([P % R.primes[i] for i in range(ell)])
    qlinv = u64([pow(R.primes[l], -1, R.primes[i]) for i in range(l)])
    fold_k = P % R.primes[l]
    key = np.concatenate([np.concatenate([u64(kb[j]), u64(ka[j])]) for j in range(beta)])
    # exact: the summed tensor, its relinearisation, ModDown + rescale, the addend
    t0 = (a0 * b0 + c0 * e0) % ql
    t1 = (a0 * b1 + a1 * b0 + c0 * e1 + c1 * e0) % ql
    t2 = (a1 * b1 + c1 * e1) % ql
    ext = K.exact_modup(R, t2, up, ell, Kp)
    s = [sum(e * k[kr] for e, k in zip(ext, kk)) % q for kk in (kb, ka)]
    want = [K.exact_md_rescale(R, s[p], (t0, t1)[p], down, ell, Kp, Lq, fold_k) for p in range(2)]
    r = [H.pattern_polys(R, ident(l), 66)["uniform"], H.pattern_polys(R, ident(l), 67)["qm1"]]
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
        m = ident(ell)
        # the composed form
        d = [D.alloc(ell * n) for _ in range(6)]
        D.call("sfp_tensor", d[0], d[1], d[2], dev[0], dev[1], dev[2], dev[3], m)
        D.call("sfp_tensor", d[3], d[4], d[5], dev[4], dev[5], dev[6], dev[7], m)
        for i in range(3):
            D.call("sfp_add", d[i], d[i], d[3 + i], m)
        assert_eq(D.down(d[2], (ell, n)), t2, "summed d2 (%s)" % kind)
        D.call("sfp_modup", E, d[2], ell, Kp, Lq, alpha, cv, scr)
        D.call("sfp_ks_inner_fold", acc, acc1, E, rows * n, KEY, beta, ell, Kp, Lq, d[0], d[1], fold_k)
        D.call("sfp_moddown_rescale", o0, o1, d[0], d[1], acc, rows * n, ell, Kp, Lq, cP, pinv, pmod, qlinv, scr, 0)
        if addend:
            D.call("sfp_add", o0, o0, R0, ident(l))
            D.call("sfp_add", o1, o1, R1, ident(l))
        for p, o in enumerate((o0, o1)):
            assert_eq(D.down(o, (l, n)), want[p], "composed out%d (ell %d, %s)" % (p, ell, kind))
        # the fused prim, where the library has it and takes the shape
        if D.has("sfp_mult2_relin_rescale_add"):
            D.put(o0, np.zeros(ell * n, dtype=np.uint64))
            D.put(o1, np.zeros(ell * n, dtype=np.uint64))
            rc = D.call("sfp_mult2_relin_rescale_add", o0, o1, *dev, ell, Kp, Lq, alpha, cv, KEY, cP, pinv, pmod,
                        qlinv, acc, E, scr, R0 if addend else None, R1 if addend else None, 1, None)
            if rc == 0:
                fused += 1
                for p, o in enumerate((o0, o1)):
                    assert_eq(D.down(o, (l, n)), want[p], "fused out%d (ell %d, %s)" % (p, ell, kind))
        D.call("sfp_sync")
        for c in cj + [cP]:
            D.call("sfp_free_conv", c)
        D.release()
    return fused


@pytest.fixture(scope="module")
def devs(oracle_lib):
    return lambda primes, logn: [H.dev(oracle_lib, "oracle", primes, logn)]


@pytest.mark.parametrize("ell", [3, 13])
@pytest.mark.parametrize("kind", ["uniform", "qm1"])
def test_composed_form_is_exact(devs, ell, kind):
    assert sum2_case(devs, ell, kind) == 0  # (the oracle has no fused prim)


def test_composed_form_without_addend(devs):
    assert sum2_case(devs, 3, "uniform", addend=False) == 0


# ---- engine level ------------------------------------------------------------------


def test_engine_value_and_preconditions(oracle_lib):
    e = sfhe.Engine("oracle", mult_depth=4, ring_dim=1 << 13, batch_size=8, seed=77)
    rng = np.random.default_rng(3)
    a, b, a2, b2, r = (rng.uniform(-1, 1, 8) for _ in range(5))
    ca, cb, ca2, cb2 = (e.encrypt(v.tolist()) for v in (a, b, a2, b2))
    cr = e.encrypt(r.tolist(), level=1)
    e.op_stats(reset=True)
    got = np.array(e.decrypt(e.mult_sum2(ca, cb, ca2, cb2, cr)))
    # the product's usual error (tests/test_gpu_parity.py test_ops_bitexact: 1e-6 for one product)
    assert np.max(np.abs(got - (a * b + a2 * b2 + r))) < 2e-6
    got = np.array(e.decrypt(e.mult_sum2(ca, cb, ca2, cb2)))
    assert np.max(np.abs(got - (a * b + a2 * b2))) < 2e-6
    assert e.dot_counts() == (0, 2)
    # a product among the operands is settled by the C API, then taken
    p = e.mult(ca, cb)  # level 1
    out = e.mult_sum2(p, cr, cr, p)
    assert out.level == 2
    assert np.max(np.abs(np.array(e.decrypt(out)) - 2 * a * b * r)) < 2e-6
    with pytest.raises(sfhe.SfheError):
        e.mult_sum2(ca, cb, ca2, cr)  # operands at two levels
    with pytest.raises(sfhe.SfheError):
        e.mult_sum2(ca, cb, ca2, cb2, ca)  # the addend is not at the result's level


# ---- sign level --------------------------------------------------------------------

V = [0.02, -0.02, 0.01, -0.01, 0.4, -0.6, 1, -1]
KW = dict(mult_depth=18, ring_dim=1 << 13, batch_size=8, scaling_mod_size=50, seed=1234)

_CHILD = r"""
import hashlib, json, os
import sfhe
kw = %r
v = %r
e = sfhe.Engine("oracle", **kw)
x = e.encrypt(v)
e.op_stats(reset=True)
s = e.sign(x, 3, 4, 2)
out = dict(level=int(s.level), sha=hashlib.sha256(s.download().tobytes()).hexdigest(), dots=e.dot_counts(),
           ops=e.op_stats())
e2 = sfhe.Engine("oracle", mult_depth=9, ring_dim=1 << 12, batch_size=8, scaling_mod_size=50, seed=1234)
s2 = e2.sign(e2.encrypt(v), 4, 1, 1)  # f_4: degree 15, pairs at the root and at the root's hi child
out["sha15"] = hashlib.sha256(s2.download().tobytes()).hexdigest()
out["dots15"] = e2.dot_counts()
print("RESULT " + json.dumps(out))
""" % (KW, V)


def _child(**knobs):
    env = dict(os.environ)
    for k in ("SFHE_SIGN_BATCH", "SFHE_SIGN_DOT", "SFHE_MULT_SUM2_FUSED"):
        env.pop(k, None)
    env.update(knobs)
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(re.search(r"RESULT (.*)", r.stdout).group(1))


def test_issue_orders_agree_and_counters(oracle_lib):
    on, off = _child(), _child(SFHE_SIGN_BATCH="0")
    assert on["level"] == off["level"] == 18
    assert on["sha"] == off["sha"] and on["sha15"] == off["sha15"]
    assert on["ops"] == off["ops"]
    # one paired product per degree-7 polynomial: six in sign(3, 4, 2); two in one f_4
    for r in (on, off):
        assert r["dots"] == [0, 6] and r["dots15"] == [0, 2]


def test_knob_off_is_the_two_product_route(oracle_lib, monkeypatch):
    e = sfhe.Engine("oracle", **KW)
    x = e.encrypt(V)
    e.op_stats(reset=True)
    on = e.sign(x, 3, 4, 2)
    assert e.dot_counts() == (0, 6)
    ops_on = e.op_stats(reset=True)
    monkeypatch.setenv("SFHE_SIGN_DOT", "0")
    off = e.sign(x, 3, 4, 2)
    assert e.dot_counts() == (0, 0)
    ops_off = e.op_stats()
    # six relinearisations and rescales fewer: one per polynomial
    assert ops_off["keyswitch"] - ops_on["keyswitch"] == 6 and ops_off["rescale"] - ops_on["rescale"] == 6
    assert hashlib.sha256(on.download().tobytes()).digest() != hashlib.sha256(off.download().tobytes()).digest()
    a, b = np.array(e.decrypt(on)), np.array(e.decrypt(off))
    # The two routes evaluate one polynomial composition and differ by key-switch rounding
    # alone: at a 50-bit scale that is below 1e-11 per product, and six polynomials whose
    # slopes stay below 4.6 (g_3) and 2.2 (f_3) amplify it by less than 4.6^4 2.2^2 < 2200.
    assert np.max(np.abs(a - b)) < 1e-7
    big = np.abs(np.array(V)) >= 0.4
    assert np.max(np.abs(a[big] - np.sign(np.array(V))[big])) < 0.01
