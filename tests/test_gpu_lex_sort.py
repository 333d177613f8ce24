"""The lexicographic rank and the record sort / selection by several keys on the device against
the C oracle, residue for residue (`==` on Ct.download()).

Both backends run the same integer program (core/context.cpp EvalLexStep); the product forms
each Horner step's tensor in one launch (prims.h sfp_lex_tensor, kernel k_lex_tensor), the
oracle composes it of the generic prims, and SFHE_LEX_FUSED=0 makes the product compose it
too.  Engines share a seed, so equal residues in means equal residues out.

Shapes and inputs as tests/test_lex_sort.py: N = 8 and N = 64 at ring 2^12 with m = 2, N = 8
with m = 3.  lex_counts is ((m - 1) B, 0) per rank on the product, (0, (m - 1) B) on the oracle.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_lex_sort import GATE, SHAPES, lex_input, lex_input3, lex_order, lex_rank

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PY = os.path.join(os.path.dirname(HERE), "sorting-fhe_amd", "python")
KINDS = ["g", "e"]


def engines(N, logn, m):
    cfg = slotsim.default_sign_config(N)
    depth = sfhe.lex_sort_depth(N, cfg, m, "hip")
    _, rots = sfhe.select_params(N, "hip")
    out = {}
    for b in ("hip", "oracle"):
        e = sfhe.Engine(b, mult_depth=depth, ring_dim=1 << logn, batch_size=N, rotations=rots, seed=20251205 + N)
        e.set_quiet(True)
        out[b] = (e, e.sorter(N, rotations=rots))
    return out, depth, cfg


def same(a, b, what):
    x, y = a.download(), b.download()
    assert x.shape == y.shape and a.level == b.level, (what, x.shape, y.shape, a.level, b.level)
    bad = int(np.count_nonzero(x != y))
    assert bad == 0, f"{what}: {bad} of {x.size} residues differ"


def cases(N, m):
    if m == 3:
        return {"m3": lex_input3(N)}
    return {k: lex_input(N, k) for k in KINDS}


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per (N, m): both engines with their sorters, every case's key columns (and two payload
    columns) encrypted on both in the same order right after the sorter, and the oracle's
    ranks, computed once."""
    out = {}
    for N, logn, B, m in [s + (2,) for s in SHAPES] + [(8, 12, 1, 3)]:
        eng, depth, cfg = engines(N, logn, m)
        rng = np.random.default_rng(7)
        cols = [rng.permutation(N) / N, 1.0 - 2.0 * rng.permutation(N) / N]
        cts = {}
        for b, (e, _) in eng.items():
            cts[b] = {k: [e.encrypt(c.tolist()) for c in keys] for k, (keys, _) in cases(N, m).items()}
            cts[b]["cols"] = [e.encrypt(c.tolist()) for c in cols]
        eo, so = eng["oracle"]
        eo.op_stats(reset=True)
        ref = {k: so.rank_lex(cts["oracle"][k], desc, *cfg) for k, (_, desc) in cases(N, m).items()}
        assert eo.lex_counts() == (0, (m - 1) * B * len(ref))
        out[N, m] = (eng, cfg, cts, ref, cols, depth)
    yield out
    for v in out.values():
        for e, _ in v[0].values():
            e.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_rank_lex_bitexact(pairs, monkeypatch, N, logn, B, kind):
    monkeypatch.delenv("SFHE_LEX_FUSED", raising=False)
    eng, cfg, cts, ref, _, _ = pairs[N, 2]
    keys, desc = lex_input(N, kind)
    e, s = eng["hip"]
    e.op_stats(reset=True)
    rank = s.rank_lex(cts["hip"][kind], desc, *cfg)
    assert e.lex_counts() == (B, 0)
    same(rank, ref[kind], "rank_lex")
    got = np.array(e.decrypt(rank))[:N]
    assert np.array_equal(np.rint(got), lex_rank(keys, desc))


def test_rank_lex_three_keys_bitexact(pairs, monkeypatch):
    monkeypatch.delenv("SFHE_LEX_FUSED", raising=False)
    N = 8
    eng, cfg, cts, ref, _, _ = pairs[N, 3]
    keys, desc = lex_input3(N)
    e, s = eng["hip"]
    e.op_stats(reset=True)
    rank = s.rank_lex(cts["hip"]["m3"], desc, *cfg)
    assert e.lex_counts() == (2, 0)
    same(rank, ref["m3"], "rank_lex m = 3")
    assert np.array_equal(np.rint(np.array(e.decrypt(rank))[:N]), lex_rank(keys, desc))


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_knob_composes_the_same_residues(pairs, monkeypatch, N, logn, B):
    eng, cfg, cts, ref, _, _ = pairs[N, 2]
    _, desc = lex_input(N, "g")
    e, s = eng["hip"]
    ct = cts["hip"]["g"]
    monkeypatch.delenv("SFHE_LEX_FUSED", raising=False)
    e.op_stats(reset=True)
    fused = s.rank_lex(ct, desc, *cfg)
    assert e.lex_counts() == (B, 0)
    monkeypatch.setenv("SFHE_LEX_FUSED", "0")
    e.op_stats(reset=True)
    composed = s.rank_lex(ct, desc, *cfg)
    assert e.lex_counts() == (0, B)
    same(fused, composed, "SFHE_LEX_FUSED=0")
    same(composed, ref["g"], "SFHE_LEX_FUSED=0 vs oracle")


def test_records_lex_bitexact(pairs, monkeypatch):
    """sort_records_lex and select_records_lex at N = 64 (two batches) against the oracle."""
    monkeypatch.delenv("SFHE_LEX_FUSED", raising=False)
    N = 64
    eng, cfg, cts, _, cols, depth = pairs[N, 2]
    keys, desc = lex_input(N, "g")
    order = lex_order(keys, desc)
    got = {}
    for b, (e, s) in eng.items():
        ks, outs = s.sort_records_lex(cts[b]["g"], cts[b]["cols"], desc, *cfg)
        sk, so = s.select_records_lex(cts[b]["g"], cts[b]["cols"], range(4), desc, *cfg)
        got[b] = (ks + outs, sk + so)
    for i, (a, o) in enumerate(zip(got["hip"][0], got["oracle"][0])):
        same(a, o, f"sort_records_lex column {i}")
        assert a.level == depth
    for i, (a, o) in enumerate(zip(got["hip"][1], got["oracle"][1])):
        same(a, o, f"select_records_lex column {i}")
    e = eng["hip"][0]
    for src, a, t in zip(keys + cols, *got["hip"]):
        assert float(np.max(np.abs(np.array(e.decrypt(a))[:N] - src[order]))) < GATE
        assert float(np.max(np.abs(np.array(e.decrypt(t))[:4] - src[order][:4]))) < GATE


CHILD = """
import sys, numpy as np
sys.path[:0] = sys.argv[1:4]
import sfhe
from oracle import slotsim
from test_lex_sort import lex_input
from test_gpu_lex_sort import KINDS
N, ring, out = int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
cfg = slotsim.default_sign_config(N)
depth = sfhe.lex_sort_depth(N, cfg, 2, "hip")
_, rots = sfhe.select_params(N, "hip")
e = sfhe.Engine("hip", mult_depth=depth, ring_dim=ring, batch_size=N, seed=20251205 + N, rotations=rots)
e.set_quiet(True)
s = e.sorter(N, rotations=rots)
cts = {k: [e.encrypt(c.tolist()) for c in lex_input(N, k)[0]] for k in KINDS}  # (the fixture's order)
e.op_stats(reset=True)
r = s.rank_lex(cts["g"], lex_input(N, "g")[1], *cfg)
np.save(out, r.download())
print("lex_counts", *e.lex_counts())
"""


def test_host_thread_lanes(pairs, tmp_path):
    """SFHE_HOST_THREADS=1 (each lane issued by its own host thread; read once per process,
    hence the fresh child): the two batches' signs, tie terms and Horner steps on two threads."""
    N, logn, B = SHAPES[1]
    out = str(tmp_path / "rank.npy")
    r = subprocess.run([sys.executable, "-u", "-c", CHILD, os.path.dirname(HERE), PY, HERE, str(N), str(1 << logn), out],
                       env=dict(os.environ, SFHE_HOST_THREADS="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("lex_counts")[-1].split() == [str(B), "0"]
    ref = pairs[N, 2][3]["g"].download()
    got = np.load(out)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)
