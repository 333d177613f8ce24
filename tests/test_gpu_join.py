"""The join of two encrypted tables on the device against the C oracle, residue for residue (`==`
on Ct.download()).

Both backends run the same integer program (core/context.cpp EvalGateOr under
DirectSort<N>::joinAggregate); the product forms each OR's tensor in one launch (prims.h
sfp_or_tensor, kernel k_or_tensor), the oracle composes it of the generic prims, and
SFHE_JOIN_FUSED=0 makes the product compose it too.  Engines share a seed, so equal residues in
means equal residues out.

Shapes and inputs as tests/test_join.py: N = 8 (one batch) and N = 64 (two batches, both lanes)
at ring 2^12; one key in cases (h) and (d), the two-key cross case with C = 3 columns, three keys
at N = 8.  join_counts is (B (m - 1), 0) per call on the product and (0, B (m - 1)) on the oracle
and under the knob.
"""
import numpy as np
import pytest

import sfhe
from test_group import SHAPES, payload
from test_join import Ctx, check_join, join_keys, multi_keys

pytestmark = pytest.mark.gpu

# (name, N, m): what every join test runs
CASES = [(k, N, 1) for N, _, _ in SHAPES for k in ("h", "d")] + [("cross", N, 2) for N, _, _ in SHAPES] + \
    [("cross", 8, 3)]
LOGN = {N: logn for N, logn, _ in SHAPES}
BATCHES = {N: B for N, _, B in SHAPES}
COLS = 3


def keys_of(name, N, m):
    return join_keys(N, name) if m == 1 else multi_keys(N, m)


def flat(got):
    return [got["count"]] + got["sums"]


def same(a, b, what):
    x, y = a.download(), b.download()
    assert x.shape == y.shape and a.level == b.level, (what, x.shape, y.shape, a.level, b.level)
    bad = int(np.count_nonzero(x != y))
    assert bad == 0, f"{what}: {bad} of {x.size} residues differ"


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per (N, m): both contexts, the case's keys and the three payload columns encrypted on both
    in the same order, and the oracle's result, computed once."""
    out = {}
    for N, m in sorted({(N, m) for _, N, m in CASES}):
        ctx = {b: Ctx(b, N, LOGN[N], m) for b in ("hip", "oracle")}
        cts, ref = {b: {} for b in ctx}, {}
        for name in [n for n, N2, m2 in CASES if (N2, m2) == (N, m)]:
            ka, kb = keys_of(name, N, m)
            for b, c in ctx.items():
                cts[b][name] = (c.enc(ka), c.enc(kb), c.enc(payload(N, COLS)))
            o = ctx["oracle"]
            o.e.op_stats(reset=True)
            ref[name] = o.s.join(*cts["oracle"][name], *o.cfg)
            assert o.e.join_counts() == (0, BATCHES[N] * (m - 1))
        out[(N, m)] = (ctx, cts, ref)
    yield out
    for ctx, _, _ in out.values():
        for c in ctx.values():
            c.e.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name,N,m", CASES)
def test_join_bitexact(pairs, monkeypatch, name, N, m, fused):
    if fused:
        monkeypatch.delenv("SFHE_JOIN_FUSED", raising=False)
    else:
        monkeypatch.setenv("SFHE_JOIN_FUSED", "0")
    ctx, cts, ref = pairs[(N, m)]
    c = ctx["hip"]
    c.e.op_stats(reset=True)
    got = c.s.join(*cts["hip"][name], *c.cfg)
    ors = BATCHES[N] * (m - 1)
    assert c.e.join_counts() == ((ors, 0) if fused else (0, ors))
    for i, (a, o) in enumerate(zip(flat(got), flat(ref[name]))):
        same(a, o, f"N={N} m={m} ({name}) output {i}{'' if fused else ' SFHE_JOIN_FUSED=0'}")
    ka, kb = keys_of(name, N, m)
    check_join(c, got, ka, kb, payload(N, COLS), f"hip N={N} m={m} ({name})")  # the decrypted gate


def test_gate_or_bitexact(pairs, monkeypatch):
    """The op alone, the operands at one level and at two, fused, composed and on the oracle."""
    monkeypatch.delenv("SFHE_JOIN_FUSED", raising=False)
    N = 8
    ctx, _, _ = pairs[(N, 1)]
    rng = np.random.default_rng(13)
    a, b = rng.uniform(0, 1, N), rng.uniform(0, 1, N)
    a[:4], b[:4] = [0, 0, 1, 1], [0, 1, 0, 1]
    outs = {}
    for be, c in ctx.items():
        act, bct = c.enc([a, b])
        low = c.e.mult_const(bct, 1.0)  # one level down: fewer limbs than a
        ops = [(act, bct), (act, low), (low, act)]
        c.e.op_stats(reset=True)
        outs[be] = [c.e.gate_or(x, y) for x, y in ops]
        assert c.e.join_counts() == ((3, 0) if be == "hip" else (0, 3))
        if be == "hip":
            monkeypatch.setenv("SFHE_JOIN_FUSED", "0")
            outs["composed"] = [c.e.gate_or(x, y) for x, y in ops]
            monkeypatch.delenv("SFHE_JOIN_FUSED")
            assert c.e.join_counts() == (3, 3)
    for i in range(3):
        same(outs["hip"][i], outs["oracle"][i], f"gate_or form {i}")
        same(outs["composed"][i], outs["oracle"][i], f"gate_or composed form {i}")
        assert outs["hip"][i].level == (1 if i == 0 else 2)
        assert float(np.max(np.abs(ctx["hip"].dec(outs["hip"][i]) - (a + b - a * b)))) < 1e-6
