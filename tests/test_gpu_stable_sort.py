"""The stable rank sort on the device against the C oracle, residue for
residue (`==` on Ct.download()).

Both backends run the same integer program (core/context.cpp EvalTieTerm);
the product forms each batch's tie term's tensor in one launch (prims.h
sfp_tie_tensor, kernel k_tie_tensor), the oracle composes it of sfp_mul,
sfp_add_const and sfp_tensor, and SFHE_TIE_FUSED=0 makes the product compose
it too.  Engines share a seed, so equal residues in means equal residues out.

Shapes as tests/test_stable_sort.py: N = 8 at ring 2^12 (one batch) and
N = 64 at ring 2^12 (P = 32, B = 2: the wrap crosses the batch boundary and
both lanes run); inputs (b) every value twice and (c) one value at every other
index.  tie_counts is (B, 0) per rank on the product and (0, B) on the oracle.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_stable_sort import GATE, make_input, stable_rank

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PY = os.path.join(os.path.dirname(HERE), "sorting-fhe_amd", "python")
SHAPES = [(8, 12, 1), (64, 12, 2)]  # N, log2 ring, batches B


def engines(N, logn):
    depth, rots = sfhe.direct_sort_params(N, "hip")
    out = {}
    for b in ("hip", "oracle"):
        e = sfhe.Engine(b, mult_depth=depth + 1, ring_dim=1 << logn, batch_size=N, rotations=rots,
                        seed=20251205 + N)
        e.set_quiet(True)
        out[b] = (e, e.sorter(N))
    return out, depth + 1, slotsim.default_sign_config(N)


def same(a, b, what):
    x, y = a.download(), b.download()
    assert x.shape == y.shape and a.level == b.level, (what, x.shape, y.shape, a.level, b.level)
    bad = int(np.count_nonzero(x != y))
    assert bad == 0, f"{what}: {bad} of {x.size} residues differ"


KINDS = ["b", "c"]


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per shape: both engines with their sorters, the inputs encrypted on
    both in the same order right after the sorter (equal residues: the tests
    below only evaluate, so their order does not matter), and the oracle's
    stable ranks, computed once."""
    out = {}
    for N, logn, B in SHAPES:
        eng, depth, cfg = engines(N, logn)
        cts = {b: {k: e.encrypt(make_input(N, k).tolist()) for k in KINDS} for b, (e, _) in eng.items()}
        eo, so = eng["oracle"]
        eo.op_stats(reset=True)
        ref = {k: so.rank_stable(cts["oracle"][k], *cfg) for k in KINDS}
        assert eo.tie_counts() == (0, B * len(KINDS))
        out[N] = (eng, cfg, cts, ref)
    yield out
    for eng, _, _, _ in out.values():
        for e, _ in eng.values():
            e.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_rank_stable_bitexact(pairs, monkeypatch, N, logn, B, kind):
    monkeypatch.delenv("SFHE_TIE_FUSED", raising=False)
    eng, cfg, cts, ref = pairs[N]
    e, s = eng["hip"]
    e.op_stats(reset=True)
    rank = s.rank_stable(cts["hip"][kind], *cfg)
    assert e.tie_counts() == (B, 0)
    same(rank, ref[kind], "rank_stable")
    got = np.array(e.decrypt(rank))[:N]
    assert np.array_equal(np.rint(got), stable_rank(make_input(N, kind)))


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_knob_composes_the_same_residues(pairs, monkeypatch, N, logn, B):
    eng, cfg, cts, ref = pairs[N]
    e, s = eng["hip"]
    ct = cts["hip"]["c"]
    monkeypatch.delenv("SFHE_TIE_FUSED", raising=False)
    e.op_stats(reset=True)
    fused = s.rank_stable(ct, *cfg)
    assert e.tie_counts() == (B, 0)
    monkeypatch.setenv("SFHE_TIE_FUSED", "0")
    e.op_stats(reset=True)
    composed = s.rank_stable(ct, *cfg)
    assert e.tie_counts() == (0, B)
    same(fused, composed, "SFHE_TIE_FUSED=0")
    same(composed, ref["c"], "SFHE_TIE_FUSED=0 vs oracle")


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_sort_stable_eager_captured_replayed(hip_lib, oracle_lib, monkeypatch, N, logn, B):
    monkeypatch.delenv("SFHE_TIE_FUSED", raising=False)
    monkeypatch.setenv("SFHE_GRAPH", "1")
    eng, depth, cfg = engines(N, logn)
    x = make_input(N, "b")
    (eh, sh), (eo, so) = eng["hip"], eng["oracle"]
    cth, cto = eh.encrypt(x.tolist()), eo.encrypt(x.tolist())
    ref = so.sort_stable(cto, *cfg)
    eager = sh.sort_stable(cth, *cfg)
    assert sh.graph_nodes() == 0
    eh.op_stats(reset=True)
    captured = sh.sort_stable(cth, *cfg)
    nodes = sh.graph_nodes()
    assert nodes > 0
    assert eh.tie_counts() == (B, 0)  # recorded into the graph: the fused launch is capturable
    replayed = sh.sort_stable(cth, *cfg)
    for what, ct in (("eager", eager), ("captured", captured), ("replayed", replayed)):
        same(ct, ref, f"sort_stable ({what})")
    assert replayed.level == depth
    err = float(np.max(np.abs(np.array(eh.decrypt(replayed))[:N] - np.sort(x))))
    assert err < GATE, err
    # the plain sort keeps its own graph beside the stable one
    plain = [sh.sort(cth, *cfg) for _ in range(3)]
    plain_nodes = sh.graph_nodes()
    assert plain_nodes > 0 and plain_nodes != nodes, (plain_nodes, nodes)
    same(plain[2], so.sort(cto, *cfg), "plain sort after stable sorts")
    same(sh.sort_stable(cth, *cfg), ref, "stable replay after plain sorts")
    assert sh.graph_nodes() == nodes
    print(f"N={N}: stable graph {nodes} nodes, plain graph {plain_nodes} nodes, max err {err:.3g}")
    eh.close()
    eo.close()


CHILD = """
import sys, numpy as np
sys.path[:0] = sys.argv[1:4]
import sfhe
from oracle import slotsim
from test_stable_sort import make_input
N, ring, out = int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
depth, rots = sfhe.direct_sort_params(N, "hip")
e = sfhe.Engine("hip", mult_depth=depth + 1, ring_dim=ring, batch_size=N, seed=20251205 + N, rotations=rots)
e.set_quiet(True)
s = e.sorter(N)
cts = {k: e.encrypt(make_input(N, k).tolist()) for k in ("b", "c")}  # (the fixture's order: same residues)
e.op_stats(reset=True)
r = s.rank_stable(cts["c"], *slotsim.default_sign_config(N))
np.save(out, r.download())
print("tie_counts", *e.tie_counts())
"""


def test_host_thread_lanes(pairs, tmp_path):
    """SFHE_HOST_THREADS=1 (each lane issued by its own host thread; read once
    per process, hence the child): the two batches' tie terms on two threads."""
    N, logn, B = SHAPES[1]
    out = str(tmp_path / "rank.npy")
    r = subprocess.run([sys.executable, "-u", "-c", CHILD, os.path.dirname(HERE), PY, HERE, str(N), str(1 << logn), out],
                       env=dict(os.environ, SFHE_HOST_THREADS="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("tie_counts")[-1].split() == [str(B), "0"]
    ref = pairs[N][3]["c"].download()
    got = np.load(out)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)
