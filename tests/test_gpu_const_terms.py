"""The sign polynomials' coefficient terms c*x as constant rescales, bit for bit.

A one-input LinearWSumRescale is Rescale(k x): the HIP engine and the oracle
take it as the fused constant rescale (sfp_mul_const_rescale: no weighted-sum
launch, no temporary), and OddPolyWaves hands the four terms of a degree-7
polynomial to ConstTermsRescale, which on the HIP engine issues them as one
inverse and one forward NTT launch pair (sfp_const_terms_rescale: a row-group
set per term; the oracle has no such prim and forms them one by one).
SFHE_CONST_TERMS=0, read per call, takes the weighted sum followed by a
rescale.  All three compute the same integers: every comparison below is on
downloaded residues, and Engine.const_term_counts() = (merged, single,
composed) shows that the path under test ran.

Levels: a fresh ciphertext is at level 0 with depth + 1 limbs, so the terms
of the first polynomial (at levels 1, 2, 2, 3) rescale at ell = depth + 1,
depth, depth, depth - 1 limbs: the forward launch of the merged prim has
8 * depth - 8 rows.

The issue asks for a (3, 2, 2) sign at depth 6; four degree-7 polynomials need
12 levels, so (3, 2, 2) runs at depth 12 and the depth-6 case is the sign that
fits it, (3, 1, 1).

A one-input LinearWSumRescale outside the sign, with and without a constant
term (sfp_mul_const_rescale_add / sfp_mul_const_rescale), is a Chebyshev leaf
with one non-zero T_j when the leaves are formed one by one
(SFHE_PS_UNBATCHED=1, read once per process: a child process).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sfhe
from oracle import slotsim

pytestmark = pytest.mark.gpu

V = [0.02, -0.02, 0.01, -0.01, 0.4, -0.6, 1, -1]


def engine(backend, ring, depth, batch=8, rotations=(), scaling=50):
    e = sfhe.Engine(backend, mult_depth=depth, ring_dim=ring, batch_size=batch, scaling_mod_size=scaling,
                    secure=False, seed=1234, rotations=rotations)
    e.set_quiet(True)
    return e


def sign_run(backend, ring, depth, cfg):
    """(residues, level, const_term_counts) of one sign on a fresh engine."""
    e = engine(backend, ring, depth)
    s = e.sign(e.encrypt(V), *cfg)
    e.sync()
    return s.download(), int(s.level), e.const_term_counts()


def identical(a, b, what):
    assert a.shape == b.shape, what
    bad = int(np.count_nonzero(a != b))
    assert bad == 0, f"{what}: {bad} of {a.size} residues differ"


def fwd_rows(depth):
    ells = (depth + 1, depth, depth, depth - 1)
    return sum(2 * (ell - 1) for ell in ells)


@pytest.mark.parametrize("logn", [12, 13])
@pytest.mark.parametrize("cfg,depth,polys", [((3, 2, 2), 12, 4), ((3, 1, 1), 6, 2)])
def test_sign_three_ways(hip_lib, oracle_lib, monkeypatch, logn, cfg, depth, polys):
    """(a) HIP default, HIP with the knob off and the oracle: identical
    residues; the counters name the path each took."""
    monkeypatch.delenv("SFHE_CONST_TERMS", raising=False)
    on, lv_on, c_on = sign_run("hip", 1 << logn, depth, cfg)
    orc, lv_or, c_or = sign_run("oracle", 1 << logn, depth, cfg)
    monkeypatch.setenv("SFHE_CONST_TERMS", "0")
    off, lv_off, c_off = sign_run("hip", 1 << logn, depth, cfg)
    print(f"ring 2^{logn} {cfg}: counts on {c_on} off {c_off} oracle {c_or}")
    assert lv_on == lv_off == lv_or == depth
    identical(on, off, "knob on vs off")
    identical(on, orc, "hip vs oracle")
    assert c_on == (4 * polys, 0, 0)
    assert c_off == (0, 0, 4 * polys)
    assert c_or == (0, 4 * polys, 0)  # the oracle: every term through the fused single call


@pytest.mark.parametrize("logn,oracle", [(12, True), (16, False), (17, False)])
def test_one_polynomial(hip_lib, oracle_lib, monkeypatch, logn, oracle):
    """(b) One degree-7 polynomial (sign config (3, 1, 0)): four terms over
    three levels in one call of the prim -- the inverse launch's four equal
    sets alternate, the forward launch's unequal sets are concatenated -- at
    depth 6, at ring 2^12, at the metric ring, and at ring 2^17, the largest
    ring whose few-row launches (here 8 and 40 rows) still take 1024-word
    tiles (two columns per COL tile)."""
    depth, cfg = 6, (3, 1, 0)
    monkeypatch.delenv("SFHE_CONST_TERMS", raising=False)
    on, lv_on, c_on = sign_run("hip", 1 << logn, depth, cfg)
    monkeypatch.setenv("SFHE_CONST_TERMS", "0")
    off, lv_off, c_off = sign_run("hip", 1 << logn, depth, cfg)
    print(f"ring 2^{logn}: counts on {c_on} off {c_off}")
    assert lv_on == lv_off == 3
    identical(on, off, "knob on vs off")
    assert c_on == (4, 0, 0)
    assert c_off == (0, 0, 4)
    if oracle:
        monkeypatch.delenv("SFHE_CONST_TERMS")
        orc, lv_or, c_or = sign_run("oracle", 1 << logn, depth, cfg)
        assert lv_or == 3 and c_or == (0, 4, 0)
        identical(on, orc, "hip vs oracle")


@pytest.mark.parametrize("depth,small", [(4, True), (12, False)])
def test_both_tiles_ring16(hip_lib, monkeypatch, depth, small):
    """(c) The forward launch of the merged prim picks its tile by its total
    rows: 1024-word tiles up to 64 rows (depth 4: 24), 2048-word tiles above
    (depth 12: 88); the separate rescales it is compared with all run
    1024-word tiles (at most 24 rows each).  The tile choice is inferred from
    the row totals asserted here and the launcher's rule, not observed: nothing
    above the library sees a launch's tile (a kernel trace does; the one under
    profiles/r09_const_terms shows both tiles in the merged launches)."""
    assert (fwd_rows(depth) <= 64) == small
    assert fwd_rows(4) == 24 and fwd_rows(12) == 88
    cfg = (3, 1, 0)
    monkeypatch.delenv("SFHE_CONST_TERMS", raising=False)
    monkeypatch.delenv("SFHE_NTT_T1K_ROWS", raising=False)
    on, lv_on, c_on = sign_run("hip", 1 << 16, depth, cfg)
    monkeypatch.setenv("SFHE_CONST_TERMS", "0")
    off, lv_off, c_off = sign_run("hip", 1 << 16, depth, cfg)
    assert lv_on == lv_off == 3
    identical(on, off, "knob on vs off")
    assert c_on == (4, 0, 0) and c_off == (0, 0, 4)


def test_captured_graph(hip_lib, monkeypatch):
    """(d) DirectSort<16> at ring 2^12, twice on one sorter: the second sort is
    captured.  Its output equals the eager sort's with the knob off, and the
    graph has fewer nodes than the knob-off graph."""
    N = 16
    depth, rots = sfhe.direct_sort_params(N, "hip")
    x = slotsim.input_vector(N).tolist()
    cfg = slotsim.default_sign_config(N)
    monkeypatch.setenv("SFHE_GRAPH", "1")

    def two_sorts():
        e = engine("hip", 1 << 12, depth, batch=N, rotations=rots, scaling=40)
        s = e.sorter(N)
        ct = e.encrypt(x)
        eager = s.sort(ct, *cfg).download()
        assert s.graph_nodes() == 0
        captured = s.sort(ct, *cfg).download()
        return eager, captured, s.graph_nodes(), e.const_term_counts()

    monkeypatch.setenv("SFHE_CONST_TERMS", "0")
    eager_off, cap_off, nodes_off, c_off = two_sorts()
    monkeypatch.delenv("SFHE_CONST_TERMS")
    eager_on, cap_on, nodes_on, c_on = two_sorts()
    print(f"graph nodes: knob on {nodes_on}, off {nodes_off}; counts on {c_on} off {c_off}")
    assert c_off[0] == 0 and c_off[1] == 0 and c_off[2] > 0
    assert c_on[0] > 0 and c_on[2] == 0
    identical(cap_on, eager_off, "captured (knob on) vs eager (knob off)")
    identical(eager_on, eager_off, "eager, knob on vs off")
    identical(cap_off, eager_off, "captured vs eager, knob off")
    assert 0 < nodes_on < nodes_off


# One-input Chebyshev leaves, formed one by one (SFHE_PS_UNBATCHED=1 for the
# whole child): c1 T_1 without and with a constant term, and c2 T_2 with one
# (an input one level below x).  Per ring and series: HIP default, HIP with
# SFHE_CONST_TERMS=0 (read per call: set inside the child) and the oracle.
_CHILD = r"""
import json, os
import numpy as np
import sfhe
from oracle import cheb

x = np.linspace(-0.9, 0.9, 8)
series = {"c1": [0.0, 0.37], "c0+c1": [0.5, -0.29], "c0+c2": [-0.3, 0.0, 0.21]}
out = {}
for logn in (12, 13):
    for name, c in series.items():
        runs = {}
        for tag, backend, knob in (("on", "hip", None), ("off", "hip", "0"), ("oracle", "oracle", None)):
            os.environ.pop("SFHE_CONST_TERMS", None)
            if knob is not None:
                os.environ["SFHE_CONST_TERMS"] = knob
            e = sfhe.Engine(backend, mult_depth=4, ring_dim=1 << logn, batch_size=8, scaling_mod_size=40,
                            secure=False, seed=77)
            e.set_quiet(True)
            h = e.chebyshev(e.encrypt(x.tolist()), c)
            e.sync()
            runs[tag] = (h.download(), e.const_term_counts())
            if tag == "on":
                err = float(np.max(np.abs(np.array(e.decrypt(h))[:8] - cheb.cheb_eval(np.array(c), x))))
        os.environ.pop("SFHE_CONST_TERMS", None)
        out[f"{logn}/{name}"] = {
            "off_differ": int(np.count_nonzero(runs["on"][0] != runs["off"][0])),
            "oracle_differ": int(np.count_nonzero(runs["on"][0] != runs["oracle"][0])),
            "size": int(runs["on"][0].size), "err": err,
            "counts": {t: list(runs[t][1]) for t in runs}}
print("RESULT " + json.dumps(out))
"""


def test_one_input_leaf_with_constant(hip_lib, oracle_lib):
    """(a), the direct case: a one-input LinearWSumRescale from the Chebyshev
    evaluator, constant term in the rescale's last pass, at rings 2^12 and
    2^13.  Decryption error bound: the evaluator tests' 1e-4 at these rings."""
    env = dict(os.environ, SFHE_PS_UNBATCHED="1")
    env.pop("SFHE_CONST_TERMS", None)
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(re.search(r"RESULT (.*)", r.stdout).group(1))
    assert len(res) == 6
    for key, v in res.items():
        print(key, v)
        assert v["size"] > 0 and v["off_differ"] == 0 and v["oracle_differ"] == 0, (key, v)
        assert v["err"] < 1e-4, (key, v)
        on, off, orc = (tuple(v["counts"][t]) for t in ("on", "off", "oracle"))
        assert on == (0, 1, 0), (key, on)   # the fused single call
        assert off == (0, 0, 1), (key, off)  # the weighted sum, then the rescale
        assert orc == (0, 1, 0), (key, orc)
