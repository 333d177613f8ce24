"""Sums folded into the last NTT pass of the producing op: HIP against the oracle.

The polynomial evaluators add a ciphertext or a constant right after a
product or a rescale.  On the HIP engine that sum rides in the epilogue of the
product's / rescale's last forward NTT pass (prims.h sfp_*_add: RowGroup
esum / ecst in k_ntt and k_ntt_small), and a weighted sum's two polynomials
go out as one launch.  The C oracle has none of those entry points (they are
weak symbols, null there), so it runs product, then add, then add-constant as
separate primitives: every comparison below is fused against unfused, residue
for residue.

A silent fall-back on HIP would make that comparison vacuous, so each case
also reads the evaluator's SFHE_PS_DEBUG report (the context's running count
of folded sums, constants and paired weighted sums) and requires the HIP
engine to have folded some and the oracle none.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sfhe
from oracle import cheb

pytestmark = pytest.mark.gpu

_REPORT = re.compile(r"PSFMA (\S+) \| fused sums (\d+) \| fused constants (\d+) \| paired weighted sums (\d+)")


def same(a, b):
    x, y = a.download(), b.download()
    assert x.shape == y.shape
    bad = int(np.count_nonzero(x != y))
    assert bad == 0, f"{bad} of {x.size} residues differ"


def run_pair(capfd, monkeypatch, ring, depth, x, op, scaling=40):
    """op(engine, ciphertext) on both engines: (hip result, oracle result,
    hip counts, oracle counts, hip engine); counts = (sums, constants, pairs)."""
    monkeypatch.setenv("SFHE_PS_DEBUG", "1")
    res, counts, engines = {}, {}, {}
    for backend in ("hip", "oracle"):
        e = sfhe.Engine(backend, mult_depth=depth, ring_dim=ring, batch_size=len(x), scaling_mod_size=scaling,
                        secure=False, seed=4321)
        e.set_quiet(True)
        ct = e.encrypt(list(x))
        capfd.readouterr()
        res[backend] = op(e, ct)
        e.sync()
        reports = _REPORT.findall(capfd.readouterr().err)
        assert reports, f"{backend}: no SFHE_PS_DEBUG report from the evaluator"
        counts[backend] = tuple(int(v) for v in reports[-1][1:])
        engines[backend] = e
    return res["hip"], res["oracle"], counts["hip"], counts["oracle"], engines["hip"]


def dense_series(degree, seed):
    """Every coefficient non-zero: every leaf has a constant term and the
    remainders of the Paterson-Stockmeyer nodes are leaves, nodes and, at the
    lowest split, constants."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.05, 0.4, degree + 1) * rng.choice([-1.0, 1.0], degree + 1) / (degree + 1)
    return c


X8 = np.linspace(-0.9, 0.9, 8)


def check_series(capfd, monkeypatch, ring, depth, c, tol, scaling=40):
    hg, ho, ng, no, g = run_pair(capfd, monkeypatch, ring, depth, X8,
                                 lambda e, ct: e.chebyshev(ct, list(map(float, c))), scaling)
    print(f"ring {ring} degree {len(c) - 1}: hip folded {ng}, oracle {no}")
    same(hg, ho)
    assert no == (0, 0, 0), f"the oracle has no fused form, yet reports {no}"
    err = float(np.max(np.abs(np.array(g.decrypt(hg))[:8] - cheb.cheb_eval(np.array(c), X8))))
    assert err < tol, err
    return ng


def test_doubled_sinc_ring13(hip_lib, oracle_lib, capfd, monkeypatch):
    """The sort's own kind of series (degree 26, sparse tail): node sums whose
    r is a leaf, the ladder's '- 1' / '- T_1', leaves with a constant term."""
    sums, consts, _ = check_series(capfd, monkeypatch, 1 << 13, 6, cheb.doubled_sinc_coeffs(2), 1e-5)
    assert sums > 0 and consts > 0


def test_dense_series_ring13(hip_lib, oracle_lib, capfd, monkeypatch):
    """Degree 59 > the baby-step count, all coefficients non-zero: leaf, node
    (the separate batched sum) and constant remainders between the nodes."""
    sums, consts, _ = check_series(capfd, monkeypatch, 1 << 13, 7, dense_series(59, 11), 1e-5)
    assert sums > 0 and consts > 0


def test_constant_remainder_ring13(hip_lib, oracle_lib, capfd, monkeypatch):
    """p = c0/2 + c_33 T_33 ... : a node whose remainder is a non-zero constant
    and leaves without a constant term."""
    c = np.zeros(40)
    c[0] = 0.5
    c[33:40] = [0.11, -0.07, 0.05, 0.09, -0.03, 0.02, 0.06]
    sums, consts, _ = check_series(capfd, monkeypatch, 1 << 13, 7, c, 1e-5)
    assert consts > 0


def test_merged_waves_ring16(hip_lib, oracle_lib, capfd, monkeypatch):
    """The metric ring's tiles; degree 59 at 8 baby steps: the ladder's wave
    T_5..T_8 and the first node wave are 3-4 products (merged NG = 4)."""
    sums, consts, _ = check_series(capfd, monkeypatch, 1 << 16, 7, dense_series(59, 5), 1e-5)
    assert sums > 0 and consts > 0


def test_single_waves_ring16(hip_lib, oracle_lib, capfd, monkeypatch):
    """Degree 5 at 2 baby steps: every wave is one product (NG = 1)."""
    sums, consts, _ = check_series(capfd, monkeypatch, 1 << 16, 4, dense_series(5, 3), 1e-5)
    assert sums + consts > 0


@pytest.mark.parametrize("logn", [10, 11])
def test_small_ring(hip_lib, oracle_lib, capfd, monkeypatch, logn):
    """One-tile rings: k_ntt_small's epilogue (the relinearisation's fused
    ModDown + rescale and the leaf rescale, with the sums)."""
    sums, consts, _ = check_series(capfd, monkeypatch, 1 << logn, 5, dense_series(13, 9), 1e-4)
    assert sums > 0 and consts > 0


def test_sign_constant_ring13(hip_lib, oracle_lib, capfd, monkeypatch):
    """sign(n = 4): g_4 is a degree-27 Chebyshev series (odd: leaves without
    a constant term, the ladder's '- 1' constants, leaf remainders), f_4 an
    odd polynomial whose single-input weighted sums (c x at a level) go out
    as one launch for both polynomials.  f_4 runs after g_4's report, so a
    short series afterwards reads the context's running counters again."""
    v = [0.5, -0.5, 0.3, -0.3, 0.8, -0.8, 1, -1]

    def op(e, ct):
        out = e.sign(ct, 4, 1, 1)
        e.chebyshev(ct, [0.2, 0.3, 0.1, 0.05])
        return out

    sg, so, ng, no, g = run_pair(capfd, monkeypatch, 1 << 13, 12, v, op, scaling=50)
    print(f"sign: hip folded {ng}, oracle {no}")
    same(sg, so)
    assert no == (0, 0, 0)
    assert ng[0] > 0 and ng[1] > 0 and ng[2] > 0
    got = np.array(g.decrypt(sg))[:8]
    assert np.all(np.sign(got) == np.sign(v))


# The single weighted sum with a constant term (LinearWSumRescale(...,
# constant): the rescale of ONE ciphertext, npoly = 2, the constant's residues
# for c0 and zeros for c1) is what a leaf takes when the leaves are not
# precomputed, and what EvalPolyLinear takes.  SFHE_PS_UNBATCHED is read once
# per process, so this case runs in a child process of its own.
_CHILD = r"""
import json, sys
import numpy as np
import sfhe
from oracle import cheb

out = {}
x = np.linspace(-0.9, 0.9, 8)
rng = np.random.default_rng(21)
for logn, depth, degree in ((13, 6, 27), (11, 5, 13)):
    c = rng.uniform(0.05, 0.4, degree + 1) * rng.choice([-1.0, 1.0], degree + 1) / (degree + 1)
    raw = {}
    for backend in ("hip", "oracle"):
        e = sfhe.Engine(backend, mult_depth=depth, ring_dim=1 << logn, batch_size=8, scaling_mod_size=40,
                        secure=False, seed=99)
        e.set_quiet(True)
        h = e.chebyshev(e.encrypt(x.tolist()), c.tolist())
        raw[backend] = h.download()
        if backend == "hip":
            err = float(np.max(np.abs(np.array(e.decrypt(h))[:8] - cheb.cheb_eval(c, x))))
    out[str(logn)] = {"differ": int(np.count_nonzero(raw["hip"] != raw["oracle"])), "size": int(raw["hip"].size),
                      "err": err}
print("RESULT " + json.dumps(out))
"""


def test_unbatched_leaf_constants(hip_lib, oracle_lib):
    """Leaves formed one by one (SFHE_PS_UNBATCHED=1), every one with a
    constant term, at ring 2^13 (k_ntt) and 2^11 (k_ntt_small): bit for bit
    against the oracle, the constants folded into each leaf's own rescale and
    each leaf's two weighted sums issued as one launch."""
    env = dict(os.environ, SFHE_PS_UNBATCHED="1", SFHE_PS_DEBUG="1")
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(re.search(r"RESULT (.*)", r.stdout).group(1))
    reports = [tuple(int(v) for v in m[1:]) for m in _REPORT.findall(r.stderr)]
    print(res, reports)
    assert len(reports) == 4  # (hip, oracle) per ring, each a fresh context
    for logn, v in res.items():
        assert v["differ"] == 0, (logn, v)
        assert v["err"] < 1e-4, (logn, v)
    for hip, orc in (reports[0:2], reports[2:4]):
        assert orc == (0, 0, 0), orc
        assert hip[1] > 0 and hip[2] > 0, hip  # constants in the single-sum rescale; c0 / c1 paired
