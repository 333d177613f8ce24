"""The sum of m products relinearised once on the HIP engine: the fused launch
chain (prims.h sfp_multn_relin_rescale_add) against the composed form, residue
for residue.

The oracle has no fused prim, so HIP-vs-oracle parity compares fused against
composed; SFHE_MULT_SUM_FUSED=0 (read per call) composes on the HIP engine as
well.  Shapes as tests/test_gpu_mult_sum2.py: ring 2^12 with one digit and a
special-prime tier (ell = 3) and two digits (ell = 13); ring 2^16 at a tier
level (ell = 5, 1024-word tiles) and on 2048-word tiles (ell = 26).  Residues
are compared, never decryptions.
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_gpu_parity import pair, same
from test_mult_sumn import CAP, H, many_case, sumn_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devs(hip_lib, oracle_lib):
    return lambda primes, logn: [H.dev(hip_lib, "hip", primes, logn), H.dev(oracle_lib, "oracle", primes, logn)]


@pytest.mark.parametrize("ell", [3, 13])
@pytest.mark.parametrize("m", [2, 3, CAP])
@pytest.mark.parametrize("kind", ["uniform", "qm1"])
def test_prim_is_exact(devs, ell, m, kind):
    """Composed and fused on the device, composed on the oracle, against exact integers."""
    assert sumn_case(devs, ell, kind, m) == 1  # (the HIP library's fused prim took the shape)


@pytest.mark.parametrize("ell,m", [(3, 2), (3, CAP), (13, 3)])
def test_prim_without_addend(devs, ell, m):
    assert sumn_case(devs, ell, "qm1", m, addend=False) == 1


@pytest.mark.parametrize("ell,m", [(5, 2), (5, CAP), (26, CAP)])
def test_prim_worst_case_at_ring_2_16(devs, ell, m):
    """All-(q-1) operands on the 1024-word (ell = 5) and 2048-word (ell = 26) tile shapes: the
    longest accumulations of the tensor epilogue and of the k_ntt_ks fold (2m products, 2m FP64
    terms).  Fused = composed on the device = composed on the oracle; the exact integers are
    held at ring 2^12, where the Python reference is affordable.  One operand pattern and one key
    pattern are reused for every row set and digit: generating 4m + 2 beta of them takes longer
    than everything else in the case."""
    assert sumn_case(devs, ell, "qm1", m, logn=16, exact=False) == 1


def test_prim_declines_past_the_cap(devs):
    assert sumn_case(devs, 3, "uniform", CAP + 1) == 0  # (declined: -1, nothing done; the composed form is exact)


@pytest.fixture(scope="module")
def engines(hip_lib, oracle_lib):
    return {12: pair(1 << 12, 12, 8), 16: pair(1 << 16, 25, 8)}


def _operands(e, vals, level):
    return [e.encrypt(v, level=level) for v in vals[:-1]] + [e.encrypt(vals[-1], level=level + 1)]


@pytest.mark.parametrize("logn,level,ell", [(12, 10, 3), (12, 0, 13), (16, 21, 5), (16, 0, 26)])
def test_fused_equals_composed(engines, monkeypatch, logn, level, ell):
    g, o = engines[logn]
    rng = np.random.default_rng(ell)
    vals = [rng.uniform(-1, 1, 8).tolist() for _ in range(2 * CAP + 1)]
    cg, co = _operands(g, vals, level), _operands(o, vals, level)
    assert (12 if logn == 12 else 25) + 1 - level == ell  # (limbs at `level`: Lq - level)
    for m in (2, 3, CAP):
        for addend in (True, False):
            tg = [(cg[2 * i], cg[2 * i + 1]) for i in range(m)]
            to = [(co[2 * i], co[2 * i + 1]) for i in range(m)]
            ref = o.mult_sum(to, co[-1] if addend else None)
            g.op_stats(reset=True)
            same(g.mult_sum(tg, cg[-1] if addend else None), ref)
            assert g.sumn_counts() == (1, 0)
            monkeypatch.setenv("SFHE_MULT_SUM_FUSED", "0")
            same(g.mult_sum(tg, cg[-1] if addend else None), ref)
            monkeypatch.delenv("SFHE_MULT_SUM_FUSED")
            assert g.sumn_counts() == (1, 1)
    same(g.mult_sum([(cg[0], cg[1]), (cg[2], cg[3])], cg[-1]), o.mult_sum2(co[0], co[1], co[2], co[3], co[-1]))


@pytest.mark.parametrize("logn,level", [(12, 10), (16, 21), (16, 0)])
def test_many_batches(engines, logn, level):
    """Batches of 2 and 4 fused ops, and ops of two term counts in separate batches."""
    assert many_case(engines[logn][0], level) == (4, 0)


@pytest.mark.parametrize("logn,deg,depth", [(13, 59, 7), (16, 59, 7), (13, 70, 8)])
def test_series_bitexact_and_knob(hip_lib, oracle_lib, monkeypatch, logn, deg, depth):
    """The evaluator's chains in merged batches (several heads of one level and term count)."""
    g, o = pair(1 << logn, depth, 8)
    if deg == 70:
        c = np.array(sfhe.doubled_sinc_coeffs(8, "hip"))
        assert len(c) - 1 == 70
    else:
        c = np.random.default_rng(deg).uniform(-1, 1, deg + 1) / deg
    x = np.linspace(-0.95, 0.9, 8).tolist()
    xg, xo = g.encrypt(x), o.encrypt(x)
    g.op_stats(reset=True)
    o.op_stats(reset=True)
    yg, yo = g.chebyshev(xg, c.tolist()), o.chebyshev(xo, c.tolist())
    fg, cg = g.sumn_counts()
    fo, co = o.sumn_counts()
    assert fg > 0 and cg == 0 and fo == 0 and co == fg
    assert g.sumn_batch_counts()[1] == 0 and o.sumn_batch_counts()[1] == 0  # no chain fell back
    same(yg, yo)
    monkeypatch.setenv("SFHE_PS_DOT", "0")
    g.op_stats(reset=True)
    o.op_stats(reset=True)
    zg, zo = g.chebyshev(xg, c.tolist()), o.chebyshev(xo, c.tolist())
    assert g.sumn_counts() == (0, 0) and o.sumn_counts() == (0, 0)
    same(zg, zo)
    assert not np.array_equal(zg.download(), yg.download())


def test_graph_paths(hip_lib, oracle_lib, monkeypatch):
    """DirectSort<8> on a persistent sorter -- eager, captured, replayed twice -- with the
    chains inside the graph (their row-set arrays travel through the graph's constant
    arena): each bit-identical to the oracle."""
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
    fused, composed = g.sumn_counts()
    assert fused > 0 and composed == 0 and s.graph_nodes() == 0
    cap = s.sort(ct, *cfg).download()
    assert s.graph_nodes() > 0
    runs = [("eager", eager), ("captured", cap)] + [("replay %d" % i, s.sort(ct, *cfg).download()) for i in (1, 2)]
    for name, got in runs:
        assert np.array_equal(got, ref), name
