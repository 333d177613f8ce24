"""The sum of two products relinearised once on the HIP engine: the fused launch
chain (prims.h sfp_mult2_relin_rescale_add) against the composed form, residue
for residue.

The oracle has no fused prim, so HIP-vs-oracle parity compares fused against
composed; SFHE_MULT_SUM2_FUSED=0 (read per call) composes on the HIP engine as
well.  Shapes: ring 2^12 (two-pass kernels at their smallest) with one digit
and a special-prime tier (ell = 3) and two digits (ell = 13); ring 2^16, the
first ring with 1024-word tiles and real COL / ROW passes, at a tier level
(ell = 5) and at three digits on 2048-word tiles (ell = 26).  Residues are
compared, never decryptions.
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_gpu_parity import pair, same
from test_mult_sum2 import H, sum2_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devs(hip_lib, oracle_lib):
    return lambda primes, logn: [H.dev(hip_lib, "hip", primes, logn), H.dev(oracle_lib, "oracle", primes, logn)]


@pytest.mark.parametrize("ell", [3, 13])
@pytest.mark.parametrize("kind", ["uniform", "qm1"])
def test_prim_is_exact(devs, ell, kind):
    """Composed and fused on the device, composed on the oracle, against exact integers."""
    assert sum2_case(devs, ell, kind) == 1  # (the HIP library's fused prim took the shape)


def test_prim_without_addend(devs):
    assert sum2_case(devs, 3, "uniform", addend=False) == 1


@pytest.fixture(scope="module")
def engines(hip_lib, oracle_lib):
    return {12: pair(1 << 12, 12, 8), 16: pair(1 << 16, 25, 8)}


@pytest.mark.parametrize("logn,level,ell", [(12, 10, 3), (12, 0, 13), (16, 21, 5), (16, 0, 26)])
def test_fused_equals_composed(engines, monkeypatch, logn, level, ell):
    g, o = engines[logn]
    rng = np.random.default_rng(ell)
    vals = [rng.uniform(-1, 1, 8).tolist() for _ in range(5)]
    cts = {e: [e.encrypt(v, level=level) for v in vals[:4]] + [e.encrypt(vals[4], level=level + 1)] for e in (g, o)}
    assert (12 if logn == 12 else 25) + 1 - level == ell  # (limbs at `level`: Lq - level)
    ref ={True: o.mult_sum2(*cts[o]), False: o.mult_sum2(*cts[o][:4])}
    for addend in (True, False):
        args = cts[g] if addend else cts[g][:4]
        g.op_stats(reset=True)
        fused = g.mult_sum2(*args)
        assert g.dot_counts() == (1, 0)
        same(fused, ref[addend])
        monkeypatch.setenv("SFHE_MULT_SUM2_FUSED", "0")
        composed = g.mult_sum2(*args)
        monkeypatch.delenv("SFHE_MULT_SUM2_FUSED")
        assert g.dot_counts() == (1, 1)
        same(composed, ref[addend])
    got = np.array(g.decrypt(g.mult_sum2(*cts[g])))
    v = [np.array(x) for x in vals]
    assert np.max(np.abs(got - (v[0] * v[1] + v[2] * v[3] + v[4]))) < 2e-6


def test_sign_bitexact_and_knob(hip_lib, oracle_lib, monkeypatch):
    """g_3 then f_3 (degree 7 each) at ring 2^13: one paired product per polynomial."""
    g, o = pair(1 << 13, 6, 8, scaling=50)
    v = [0.02, -0.02, 0.01, -0.01, 0.4, -0.6, 1, -1]
    xg, xo = g.encrypt(v), o.encrypt(v)
    g.op_stats(reset=True)
    sg, so = g.sign(xg, 3, 1, 1), o.sign(xo, 3, 1, 1)
    assert g.dot_counts() == (2, 0) and o.dot_counts() == (0, 2)
    same(sg, so)
    assert sg.level == so.level == 6
    # the knob: two separate products per pair (the route before the paired form), on both backends
    monkeypatch.setenv("SFHE_SIGN_DOT", "0")
    g.op_stats(reset=True)
    o.op_stats(reset=True)
    tg, to = g.sign(xg, 3, 1, 1), o.sign(xo, 3, 1, 1)
    assert g.dot_counts() == (0, 0) and o.dot_counts() == (0, 0)
    same(tg, to)
    assert not np.array_equal(tg.download(), sg.download())


def test_graph_paths(hip_lib, oracle_lib, monkeypatch):
    """DirectSort<8> on a persistent sorter -- eager, captured, replayed twice -- with the
    paired products inside the graph (their second row set travels through the graph's
    constant arena): each bit-identical to the oracle."""
    N = 8
    depth, rots = sfhe.direct_sort_params(N, "hip")
    g, o = pair(1 << 12, depth, N, rotations=rots)
    x = slotsim.input_vector(N).tolist()
    cfg = slotsim.default_sign_config(N)
    o.set_quiet(True)
    g.set_quiet(True)
    ref = o.sorter(N).sort(o.encrypt(x), *cfg).download()
    s = g.sorter(N)
    ct = g.encrypt(x)
    monkeypatch.setenv("SFHE_GRAPH", "1")
    g.op_stats(reset=True)
    eager = s.sort(ct, *cfg).download()
    fused, composed = g.dot_counts()
    assert fused > 0 and composed == 0 and s.graph_nodes() == 0
    cap = s.sort(ct, *cfg).download()
    assert s.graph_nodes() > 0
    runs = [("eager", eager), ("captured", cap)] + [("replay %d" % i, s.sort(ct, *cfg).download()) for i in (1, 2)]
    for name, got in runs:
        assert np.array_equal(got, ref), name
