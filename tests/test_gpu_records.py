"""Records on the device against the C oracle, residue for residue (`==` on
Ct.download()): place_many / sort_records.

Both backends run the same integer program; the product forms the columns'
giant-step sums with prims.h sfp_mac_plain2_cols (kernel k_mac_plain2_cols:
tiles of giants x columns under one plaintext set), the oracle -- and the
product under SFHE_PLACE_COLS=0 -- with the per-column path.  Engines share a
seed, so equal residues in means equal residues out.

Shapes as tests/test_records.py, and what each reaches in the fused kernel
(every launch covers the integer row q_0, 128-bit sums, together with the
FP64 rows; the sums run at 3 limbs):
  N = 8  @ 2^12: B = 1, one lane; nin = 2 masked inputs, ng = 4 giants;
  N = 64 @ 2^12: B = 2, both lanes; nin = 8, ng = 4.
Columns C in {1, 3, 5} with the default 4 x 2 (giants x columns) tile: C = 1 a
lone partial tile <4, 1>; 3 = 2 + 1 and 5 = 2 + 2 + 1 full tiles <4, 2> and a
partial one.  SFHE_PLACE_TILE=2x4 (the A/B tile) splits the 4 giants into
ng = 2 tiles: <2, 1>, <2, 3>, and 5 = 4 + 1 columns <2, 4> + <2, 1>.
"""
import numpy as np
import pytest

import sfhe
from oracle import slotsim
from test_records import batches, payload
from test_stable_sort import GATE, make_input

pytestmark = pytest.mark.gpu

SHAPES = [(8, 12), (64, 12)]
COUNTS = [1, 3, 5]
NG = 4  # giant steps per batch at both shapes


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


@pytest.fixture(scope="module")
def pairs(hip_lib, oracle_lib):
    """Per shape: both engines, the keys and five columns encrypted on both in
    the same order, each backend's stable rank, and the oracle's place_many
    of the five columns (column c of it is place(rank, cols[c]), whatever the
    count: tests/test_records.py), computed once."""
    out = {}
    for N, logn in SHAPES:
        eng, depth, cfg = engines(N, logn)
        cts, ranks = {}, {}
        for b, (e, s) in eng.items():
            k = e.encrypt(make_input(N, "b").tolist())
            cts[b] = (k, [e.encrypt(payload(N, c).tolist()) for c in range(max(COUNTS))])
            ranks[b] = s.rank_stable(k, *cfg)
        same(ranks["hip"], ranks["oracle"], "rank_stable")
        eo, so = eng["oracle"]
        eo.op_stats(reset=True)
        ref = so.place_many(ranks["oracle"], cts["oracle"][1])
        assert eo.place_counts() == (batches(N, logn), max(COUNTS), 0, max(COUNTS) * batches(N, logn) * NG)
        out[N] = (eng, cfg, cts, ranks, ref)
    yield out
    for v in out.values():
        for e, _ in v[0].values():
            e.close()


@pytest.mark.parametrize("tile", [None, "2x4"])
@pytest.mark.parametrize("C", COUNTS)
@pytest.mark.parametrize("N,logn", SHAPES)
def test_place_many_bitexact(pairs, monkeypatch, N, logn, C, tile):
    monkeypatch.delenv("SFHE_PLACE_COLS", raising=False)
    if tile:
        monkeypatch.setenv("SFHE_PLACE_TILE", tile)
    else:
        monkeypatch.delenv("SFHE_PLACE_TILE", raising=False)
    eng, cfg, cts, ranks, ref = pairs[N]
    e, s = eng["hip"]
    e.op_stats(reset=True)
    outs = s.place_many(ranks["hip"], cts["hip"][1][:C])
    assert e.place_counts() == (batches(N, logn), C, C * batches(N, logn) * NG, 0)
    for c, o in enumerate(outs):
        same(o, ref[c], f"place_many column {c} of {C}")
    order = np.argsort(make_input(N, "b"), kind="stable")
    err = max(float(np.max(np.abs(np.array(e.decrypt(o))[:N] - payload(N, c)[order]))) for c, o in enumerate(outs))
    assert err < GATE, err


@pytest.mark.parametrize("N,logn", SHAPES)
def test_knob_takes_the_per_column_path(pairs, monkeypatch, N, logn):
    eng, cfg, cts, ranks, ref = pairs[N]
    e, s = eng["hip"]
    C = 3
    monkeypatch.setenv("SFHE_PLACE_COLS", "0")
    e.op_stats(reset=True)
    outs = s.place_many(ranks["hip"], cts["hip"][1][:C])
    assert e.place_counts() == (batches(N, logn), C, 0, C * batches(N, logn) * NG)
    for c, o in enumerate(outs):
        same(o, ref[c], f"SFHE_PLACE_COLS=0 column {c}")
    # ... and the single-column entry point gives the same residues on the device
    same(s.place(ranks["hip"], cts["hip"][1][0]), ref[0], "place")


@pytest.mark.parametrize("N,logn", SHAPES)
def test_sort_records_eager_captured_replayed(hip_lib, oracle_lib, monkeypatch, N, logn):
    monkeypatch.delenv("SFHE_PLACE_COLS", raising=False)
    monkeypatch.delenv("SFHE_PLACE_TILE", raising=False)
    monkeypatch.setenv("SFHE_GRAPH", "1")
    eng, depth, cfg = engines(N, logn)
    (eh, sh), (eo, so) = eng["hip"], eng["oracle"]
    C = 3
    x = make_input(N, "b")
    data = [payload(N, c) for c in range(C)]
    other = [payload(N, c + 7) for c in range(C)]  # a second set of payloads for the replay
    kh, ko = eh.encrypt(x.tolist()), eo.encrypt(x.tolist())
    ch, co = ([e.encrypt(v.tolist()) for v in data] for e in (eh, eo))
    ch2, co2 = ([e.encrypt(v.tolist()) for v in other] for e in (eh, eo))
    rk, rc = so.sort_records(ko, co, True, *cfg)
    rk2, rc2 = so.sort_records(ko, co2, True, *cfg)

    def check(got, want, what):
        same(got[0], want[0], f"{what}: keys")
        for c in range(C):
            same(got[1][c], want[1][c], f"{what}: column {c}")

    check(sh.sort_records(kh, ch, True, *cfg), (rk, rc), "eager")
    assert sh.records_graph_nodes() == 0
    eh.op_stats(reset=True)
    check(sh.sort_records(kh, ch, True, *cfg), (rk, rc), "captured")
    nodes = sh.records_graph_nodes()
    assert nodes > 0 and sh.graph_nodes() == 0
    B = batches(N, logn)
    assert eh.place_counts() == (B, C + 1, (C + 1) * B * NG, 0)  # recorded into the graph
    replayed = sh.sort_records(kh, ch, True, *cfg)
    check(replayed, (rk, rc), "replayed")
    # the replay reads all 1 + C inputs through the copy-in: other payloads, their result
    check(sh.sort_records(kh, ch2, True, *cfg), (rk2, rc2), "replayed with other payloads")
    assert sh.records_graph_nodes() == nodes
    order = np.argsort(x, kind="stable")
    err = max(float(np.max(np.abs(np.array(eh.decrypt(o))[:N] - data[c][order]))) for c, o in enumerate(replayed[1]))
    assert err < GATE and replayed[0].level == depth, (err, replayed[0].level)
    # the plain and the stable sort keep their own graphs and residues
    stable = [sh.sort_stable(kh, *cfg) for _ in range(3)]
    stable_nodes = sh.graph_nodes()
    plain = [sh.sort(kh, *cfg) for _ in range(3)]
    plain_nodes = sh.graph_nodes()
    assert stable_nodes > 0 and plain_nodes > 0 and plain_nodes != stable_nodes
    same(stable[2], so.sort_stable(ko, *cfg), "stable sort after record sorts")
    same(stable[2], rk, "the record sort's keys are the stable sort's")
    same(plain[2], so.sort(ko, *cfg), "plain sort after record sorts")
    check(sh.sort_records(kh, ch, True, *cfg), (rk, rc), "record replay after the other sorts")
    assert sh.records_graph_nodes() == nodes
    print(f"N={N}: records graph {nodes} nodes, stable {stable_nodes}, plain {plain_nodes}, max err {err:.3g}")
    eh.close()
    eo.close()
