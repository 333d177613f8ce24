"""Grouping by an encrypted key on the device against the C oracle, residue for residue (`==`
on Ct.download()).

Both backends run the same integer program (core/context.cpp EvalGateSumMany); the product forms
the gated column sums' tensors in one launch per tile of two columns (prims.h
sfp_gate_tensor_cols, kernels k_gate_tensor_cols<2> and <1>), the oracle composes them of the
generic prims, and SFHE_GROUP_FUSED=0 makes the product compose them too.  Engines share a seed,
so equal residues in means equal residues out.

Shapes and inputs as tests/test_group.py: N = 8 (one batch) and N = 64 (two batches, both lanes)
at ring 2^12, cases (g) and (d), C = 3 columns so that a tile of two and a remainder of one run.
group_counts is (1, 0) per call on the product and (0, 1) on the oracle.
"""
import numpy as np
import pytest

import sfhe
from test_group import SHAPES, Ctx, check_group, group_keys, payload

pytestmark = pytest.mark.gpu

KINDS = ["g", "d"]
OUTPUTS = ["count", "index", "sum0", "sum1", "sum2"]


def flat(got):
    return [got["count"], got["index"]] + got["sums"]


def same(a, b, what):
    x, y = a.download(), b.download()
    assert x.shape == y.shape and a.level == b.level, (what, x.shape, y.shape, a.level, b.level)
    bad = int(np.count_nonzero(x != y))
    assert bad == 0, f"{what}: {bad} of {x.size} residues differ"


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per N: both contexts, every case's key and the three payload columns encrypted on both in
    the same order, and the oracle's results, computed once."""
    out = {}
    for N, logn, _ in SHAPES:
        ctx = {b: Ctx(b, N, logn) for b in ("hip", "oracle")}
        cts = {b: {"keys": {k: c.enc([group_keys(N, k)])[0] for k in KINDS}, "cols": c.enc(payload(N, 3))}
               for b, c in ctx.items()}
        o = ctx["oracle"]
        o.e.op_stats(reset=True)
        ref = {k: o.s.group(cts["oracle"]["keys"][k], cts["oracle"]["cols"], True, *o.cfg) for k in KINDS}
        assert o.e.group_counts() == (0, len(KINDS))
        out[N] = (ctx, cts, ref)
    yield out
    for ctx, _, _ in out.values():
        for c in ctx.values():
            c.e.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_group_bitexact(pairs, monkeypatch, N, logn, B, kind):
    monkeypatch.delenv("SFHE_GROUP_FUSED", raising=False)
    ctx, cts, ref = pairs[N]
    c = ctx["hip"]
    c.e.op_stats(reset=True)
    got = c.s.group(cts["hip"]["keys"][kind], cts["hip"]["cols"], True, *c.cfg)
    assert c.e.group_counts() == (1, 0)
    for name, a, o in zip(OUTPUTS, flat(got), flat(ref[kind])):
        same(a, o, f"N={N} ({kind}) {name}")
    check_group(c, got, group_keys(N, kind), payload(N, 3), f"hip N={N} ({kind})")


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_knob_composes_the_same_residues(pairs, monkeypatch, N, logn, B):
    ctx, cts, ref = pairs[N]
    c = ctx["hip"]
    monkeypatch.setenv("SFHE_GROUP_FUSED", "0")
    c.e.op_stats(reset=True)
    composed = c.s.group(cts["hip"]["keys"]["g"], cts["hip"]["cols"], True, *c.cfg)
    assert c.e.group_counts() == (0, 1)
    for name, a, o in zip(OUTPUTS, flat(composed), flat(ref["g"])):
        same(a, o, f"SFHE_GROUP_FUSED=0 N={N} {name}")
    check_group(c, composed, group_keys(N, "g"), payload(N, 3), f"hip composed N={N} (g)")


def test_gate_sum_many_bitexact(pairs, monkeypatch):
    """The op alone, B = 2 and C = 3 with the operands above the gates' level, fused, composed
    and on the oracle."""
    monkeypatch.delenv("SFHE_GROUP_FUSED", raising=False)
    N = 8
    ctx, _, _ = pairs[N]
    rng = np.random.default_rng(13)
    q = [rng.uniform(0, 1, N) for _ in range(2)]
    u = [[rng.uniform(-1, 1, N) for _ in range(2)] for _ in range(3)]
    outs = {}
    for b, c in ctx.items():
        qct = [c.e.mult_const(x, 1.0) for x in c.enc(q)]
        uct = [c.enc(col) for col in u]
        c.e.op_stats(reset=True)
        outs[b] = c.e.gate_sum_many(qct, uct)
        assert c.e.group_counts() == ((1, 0) if b == "hip" else (0, 1))
        if b == "hip":
            monkeypatch.setenv("SFHE_GROUP_FUSED", "0")
            outs["composed"] = c.e.gate_sum_many(qct, uct)
            monkeypatch.delenv("SFHE_GROUP_FUSED")
            assert c.e.group_counts() == (1, 1)
    for i in range(3):
        same(outs["hip"][i], outs["oracle"][i], f"gate_sum_many column {i}")
        same(outs["composed"][i], outs["oracle"][i], f"gate_sum_many composed column {i}")
        want = sum((1 - a) * x for a, x in zip(q, u[i]))
        assert float(np.max(np.abs(ctx["hip"].dec(outs["hip"][i]) - want))) < 1e-6
