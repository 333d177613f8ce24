"""Window sums over an encrypted key on the device against the C oracle, residue for residue
(`==` on Ct.download()).

Both backends run the same integer program (core/context.cpp EvalWeightSumMany); the product
forms the weighted column sums' tensors in one launch per tile of two columns (prims.h
sfp_weight_tensor_cols, kernels k_weight_tensor_cols<2> and <1>), the oracle composes them of the
generic prims, and SFHE_WINDOW_FUSED=0 makes the product compose them too.  Engines share a seed,
so equal residues in means equal residues out.

Shapes and inputs as tests/test_window.py: N = 8 (one batch) and N = 64 (two batches, both lanes)
at ring 2^12, cases (g) and (d), frames rows and range, C = 3 columns so that a tile of two and a
remainder of one run.  window_counts is (1, 0) per call on the product and (0, 1) on the oracle.
"""
import numpy as np
import pytest

from test_gpu_group import same
from test_group import SHAPES, group_keys, payload
from test_window import WCtx, check_window

pytestmark = pytest.mark.gpu

KINDS = ["g", "d"]
FRAMES = ["rows", "range"]
OUTPUTS = ["count", "sum0", "sum1", "sum2"]


def flat(got):
    return [got["count"]] + got["sums"]


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per N: both contexts, every case's key and the three payload columns encrypted on both in
    the same order, and the oracle's results, computed once."""
    out = {}
    for N, logn, _ in SHAPES:
        ctx = {b: WCtx(b, N, logn) for b in ("hip", "oracle")}
        cts = {b: {"keys": {k: c.enc([group_keys(N, k)])[0] for k in KINDS}, "cols": c.enc(payload(N, 3))}
               for b, c in ctx.items()}
        o = ctx["oracle"]
        o.e.op_stats(reset=True)
        ref = {(k, f): o.s.window(cts["oracle"]["keys"][k], cts["oracle"]["cols"], f, True, *o.cfg)
               for k in KINDS for f in FRAMES}
        assert o.e.window_counts() == (0, len(ref))
        out[N] = (ctx, cts, ref)
    yield out
    for ctx, _, _ in out.values():
        for c in ctx.values():
            c.e.close()


@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_window_bitexact(pairs, monkeypatch, N, logn, B, kind, frame):
    monkeypatch.delenv("SFHE_WINDOW_FUSED", raising=False)
    ctx, cts, ref = pairs[N]
    c = ctx["hip"]
    c.e.op_stats(reset=True)
    got = c.s.window(cts["hip"]["keys"][kind], cts["hip"]["cols"], frame, True, *c.cfg)
    assert c.e.window_counts() == (1, 0)
    for name, a, o in zip(OUTPUTS, flat(got), flat(ref[kind, frame])):
        same(a, o, f"N={N} {frame} ({kind}) {name}")
    check_window(c, got, group_keys(N, kind), payload(N, 3), frame, f"hip N={N} {frame} ({kind})")


@pytest.mark.parametrize("N,logn,B", SHAPES)
def test_knob_composes_the_same_residues(pairs, monkeypatch, N, logn, B):
    ctx, cts, ref = pairs[N]
    c = ctx["hip"]
    monkeypatch.setenv("SFHE_WINDOW_FUSED", "0")
    c.e.op_stats(reset=True)
    composed = c.s.window(cts["hip"]["keys"]["g"], cts["hip"]["cols"], "rows", True, *c.cfg)
    assert c.e.window_counts() == (0, 1)
    for name, a, o in zip(OUTPUTS, flat(composed), flat(ref["g", "rows"])):
        same(a, o, f"SFHE_WINDOW_FUSED=0 N={N} {name}")
    check_window(c, composed, group_keys(N, "g"), payload(N, 3), "rows", f"hip composed N={N} rows (g)")


def test_weight_sum_many_bitexact(pairs, monkeypatch):
    """The op alone, B = 2 and C = 3 with the operands above the gates' level, fused, composed
    and on the oracle."""
    monkeypatch.delenv("SFHE_WINDOW_FUSED", raising=False)
    N = 8
    ctx, _, _ = pairs[N]
    rng = np.random.default_rng(13)
    v = [rng.uniform(-0.5, 0.5, N) for _ in range(2)]
    p = [rng.integers(0, 2, N).astype(float) for _ in range(2)]
    u = [[rng.uniform(-1, 1, N) for _ in range(2)] for _ in range(3)]
    outs = {}
    for b, c in ctx.items():
        vct = [c.e.mult_const(x, 1.0) for x in c.enc(v)]
        uct = [c.enc(col) for col in u]
        c.e.op_stats(reset=True)
        outs[b] = c.e.weight_sum_many(vct, p, uct)
        assert c.e.window_counts() == ((1, 0) if b == "hip" else (0, 1))
        if b == "hip":
            monkeypatch.setenv("SFHE_WINDOW_FUSED", "0")
            outs["composed"] = c.e.weight_sum_many(vct, p, uct)
            monkeypatch.delenv("SFHE_WINDOW_FUSED")
            assert c.e.window_counts() == (1, 1)
    for i in range(3):
        same(outs["hip"][i], outs["oracle"][i], f"weight_sum_many column {i}")
        same(outs["composed"][i], outs["oracle"][i], f"weight_sum_many composed column {i}")
        want = sum((w + a) * x for w, a, x in zip(p, v, u[i]))
        assert float(np.max(np.abs(ctx["hip"].dec(outs["hip"][i]) - want))) < 1e-6
