"""The sign's odd polynomials as batched waves (CryptoContext::MaterializeMany,
csrc/algo/sign.cpp OddPolyWaves) on the HIP engine, bit for bit.

A merged launch computes the same integers as the separate launches, and the
oracle never merges (sfp_batch_begin returns 0), so HIP-vs-oracle parity
compares merged against unmerged.  Shapes: ring 2^12, batch 8, depth just
enough for the composition -- the smallest where every wave still has two
members and two different levels meet.  Residues are compared, never
decryptions.

SFHE_SIGN_BATCH, SFHE_BATCH and SFHE_LAZY are read once per process: every
setting other than the default runs in a fresh child.
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
from test_gpu_parity import pair, same

pytestmark = pytest.mark.gpu

V = [0.02, -0.02, 0.01, -0.01, 0.4, -0.6, 1, -1]


@pytest.mark.parametrize("cfg,depth", [((3, 2, 2), 12), ((4, 1, 1), 9)])
def test_sign_bitexact(hip_lib, oracle_lib, cfg, depth):
    """(3, 2, 2): four degree-7 polynomials in a row (an aligned power and a
    sum cross every polynomial boundary); (4, 1, 1): f_4, degree 15, four
    waves."""
    g, o = pair(1 << 12, depth, 8, scaling=50)
    sg, so = g.sign(g.encrypt(V), *cfg), o.sign(o.encrypt(V), *cfg)
    same(sg, so)
    assert sg.level == so.level == depth


# One (3, 2, 2) sign on HIP and on the oracle in a child: residue digests,
# levels and the merged / single launch counts around the HIP sign.
_CHILD = r"""
import hashlib, json
import sfhe
kw = dict(mult_depth=12, ring_dim=1 << 12, batch_size=8, scaling_mod_size=50, seed=1234)
v = [0.02, -0.02, 0.01, -0.01, 0.4, -0.6, 1, -1]
out = {}
for backend in ("hip", "oracle"):
    e = sfhe.Engine(backend, **kw)
    x = e.encrypt(v)
    e.sync()
    m0, s0 = e.stack_stats()
    s = e.sign(x, 3, 2, 2)
    e.sync()
    m1, s1 = e.stack_stats()
    out[backend] = dict(level=int(s.level), sha=hashlib.sha256(s.download().tobytes()).hexdigest(),
                        merged=m1 - m0, single=s1 - s0)
print("RESULT " + json.dumps(out))
"""


def _child(**knobs):
    env = dict(os.environ)
    for k in ("SFHE_SIGN_BATCH", "SFHE_BATCH", "SFHE_LAZY"):
        env.pop(k, None)
    env.update(knobs)
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(re.search(r"RESULT (.*)", r.stdout).group(1))
    print(knobs, res)
    return res


@pytest.fixture(scope="module")
def default_run(hip_lib, oracle_lib):
    return _child()


@pytest.fixture(scope="module")
def knob_off_run(hip_lib, oracle_lib):
    return _child(SFHE_SIGN_BATCH="0")


def test_knob_off_equals_on(default_run, knob_off_run):
    for r in (default_run, knob_off_run):
        assert r["hip"]["sha"] == r["oracle"]["sha"] and r["hip"]["level"] == r["oracle"]["level"] == 12
    assert default_run["hip"]["sha"] == knob_off_run["hip"]["sha"]


def test_merge_happens(default_run, knob_off_run):
    """With the knob off the only merged launches of a (3, 2, 2) sign are the
    paired weighted sums of its coefficient terms (c0 and c1 of one term in one
    launch): 4 polynomials x 4 terms = 16.  With it on, the waves' launches
    merge across ops: more merged launches.  (The counters cover launches
    issued inside batches only, so totals are not comparable.)"""
    on, off = default_run["hip"], knob_off_run["hip"]
    assert default_run["oracle"]["merged"] == 0 and knob_off_run["oracle"]["merged"] == 0
    assert off["merged"] <= 16 and off["single"] == 0  # (a paired sum never leaves a launch alone)
    assert on["merged"] > 0 and on["merged"] > off["merged"]


@pytest.mark.parametrize("knob", ["SFHE_BATCH", "SFHE_LAZY"])
def test_fallback_paths(hip_lib, oracle_lib, knob, default_run):
    r = _child(**{knob: "0"})
    assert r["hip"]["sha"] == r["oracle"]["sha"] and r["hip"]["level"] == 12
    if knob == "SFHE_BATCH":  # nothing merges; the same integers as the batched waves
        assert r["hip"]["merged"] == 0
        assert r["hip"]["sha"] == default_run["hip"]["sha"]


def test_graph_paths(hip_lib, oracle_lib, monkeypatch):
    """DirectSort<8> on a persistent sorter: eager, captured, replayed -- the
    capture undo records of batch-materialised ciphertexts -- each
    bit-identical to the oracle."""
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
    eager = s.sort(ct, *cfg).download()
    assert s.graph_nodes() == 0
    cap = s.sort(ct, *cfg).download()
    assert s.graph_nodes() > 0
    rep = s.sort(ct, *cfg).download()
    for name, got in (("eager", eager), ("captured", cap), ("replayed", rep)):
        assert np.array_equal(got, ref), name
