"""Records on the C oracle: several payload columns placed by one rank
(DirectSort<N>::placeMany / sortRecords).

The placement's indicator `hit` depends on the rank alone, so place_many
evaluates it once per batch and runs only the linear tail per column.  All
arithmetic is exact on canonical residues: column c of place_many(rank, cols)
must equal place(rank, cols[c]) residue for residue (`==` on Ct.download()).

Shapes as tests/test_stable_sort.py: N = 8 at ring 2^12 (B = 1, one lane,
npPlace = 2: 2 masked inputs per giant, 4 giants) and N = 64 at ring 2^12
(P = 32, B = 2, npPlace = 8: 8 masked inputs, 4 giants, both lanes, the blind
rotation crosses the batch boundary).  Keys are input (b), every value twice,
so stability is visible; payload column k is (index + 1) / N with alternating
sign, permuted by a seed of its own: all in [-1, 1], all distinct, so the
input order can be read back.  C in {1, 2, 3, 5} columns: with the fused
kernel's 2-column tile (GPU, tests/test_gpu_records.py) 3 and 5 leave a
partial tile; on the oracle every column takes the per-column path.
"""
import numpy as np
import pytest

import sfhe
from test_shard import compare
from test_stable_sort import GATE, SHAPES, Ctx, make_input

COUNTS = [1, 2, 3, 5]


def payload(N, k):
    idx = np.random.default_rng(977 + 31 * k + N).permutation(N)
    return (idx + 1) / N * np.where(idx % 2 == 0, 1.0, -1.0)


def batches(N, logn):
    P = min(N, (1 << logn) // 2 // N)
    return N // P


@pytest.fixture(scope="module")
def ctxs(oracle_lib):
    """Per shape: the context, the keys and five payload columns encrypted,
    the stable rank, and place(rank, column) of each column -- computed once."""
    out = {}
    for N, logn in SHAPES:
        c = Ctx("oracle", N, logn)
        keys = make_input(N, "b")
        kct = c.e.encrypt(keys.tolist())
        cols = [c.e.encrypt(payload(N, k).tolist()) for k in range(max(COUNTS))]
        rank = c.s.rank_stable(kct, *c.cfg)
        ref = [c.s.place(rank, ct).download() for ct in cols]
        out[N, logn] = (c, keys, kct, cols, rank, ref)
    yield out
    for v in out.values():
        v[0].e.close()


@pytest.mark.parametrize("C", COUNTS)
@pytest.mark.parametrize("N,logn", SHAPES)
def test_place_many_equals_place(ctxs, N, logn, C):
    c, _, _, cols, rank, ref = ctxs[N, logn]
    c.e.op_stats(reset=True)
    outs = c.s.place_many(rank, cols[:C])
    assert len(outs) == C
    for k, o in enumerate(outs):
        got = o.download()
        assert got.shape == ref[k].shape
        bad = int(np.count_nonzero(got != ref[k]))
        assert bad == 0, f"column {k} of {C}: {bad} of {got.size} residues differ"
        assert o.slots == N and cols[k].slots == N * min(N, (1 << logn) // 2 // N)
    # the indicator ran once per batch, not once per batch and column
    hits, columns, fused, composed = c.e.place_counts()
    assert (hits, columns, fused) == (batches(N, logn), C, 0)
    assert composed == C * batches(N, logn) * 4  # 4 giant steps per batch at both shapes


@pytest.mark.parametrize("N,logn", SHAPES)
def test_sort_records_stable(ctxs, N, logn):
    c, keys, kct, cols, _, _ = ctxs[N, logn]
    C = 3
    c.e.op_stats(reset=True)
    skeys, souts = c.s.sort_records(kct, cols[:C], True, *c.cfg)
    assert c.e.place_counts()[:2] == (batches(N, logn), C + 1)
    order = np.argsort(keys, kind="stable")
    kerr = float(np.max(np.abs(np.array(c.e.decrypt(skeys))[:N] - keys[order])))
    errs = [float(np.max(np.abs(np.array(c.e.decrypt(o))[:N] - payload(N, k)[order]))) for k, o in enumerate(souts)]
    print(f"N={N}: keys err {kerr:.3g}, column errs {[f'{e:.3g}' for e in errs]}, level {skeys.level}/{c.depth}")
    assert kerr < GATE, kerr
    assert max(errs) < GATE, errs
    assert skeys.level == c.depth and all(o.level == c.depth for o in souts)
    # the sorted keys are the stable sort's own residues
    assert np.array_equal(skeys.download(), c.s.sort_stable(kct, *c.cfg).download())


def test_sort_records_keys_only_and_unstable(ctxs):
    N, logn = SHAPES[0]
    c, _, _, cols, _, _ = ctxs[N, logn]
    x = make_input(N, "a")
    ct = c.e.encrypt(x.tolist())
    skeys, souts = c.s.sort_records(ct, [], False, *c.cfg)
    assert souts == []
    assert np.array_equal(skeys.download(), c.s.sort(ct, *c.cfg).download())
    skeys, souts = c.s.sort_records(ct, cols[:1], False, *c.cfg)
    got = np.array(c.e.decrypt(souts[0]))[:N]
    assert float(np.max(np.abs(got - payload(N, 0)[np.argsort(x)]))) < GATE


def test_argument_errors(ctxs):
    N, logn = SHAPES[0]
    c, _, kct, cols, rank, _ = ctxs[N, logn]
    nine = [cols[0]] * (sfhe.MAX_COLUMNS + 1)
    for bad in ([], nine, [cols[0], None]):
        with pytest.raises(sfhe.SfheError, match="sfhe error -1"):
            c.s.place_many(rank, bad)
    for bad in (nine, [None]):
        with pytest.raises(sfhe.SfheError, match="sfhe error -1"):
            c.s.sort_records(kct, bad, True, *c.cfg)
    assert len(c.s.place_many(rank, [cols[0]] * sfhe.MAX_COLUMNS)) == sfhe.MAX_COLUMNS
    assert c.s.records_graph_nodes() == 0  # the oracle has no graphs


def test_depth_one_short_is_an_error(oracle_lib):
    N, logn = SHAPES[0]
    c = Ctx("oracle", N, logn, extra=0)
    kct = c.e.encrypt(make_input(N, "b").tolist())
    col = c.e.encrypt(payload(N, 0).tolist())
    with pytest.raises(sfhe.SfheError, match=rf"sfhe error -2: .*depth {c.depth + 1}\b"):
        c.s.sort_records(kct, [col], True, *c.cfg)
    skeys, souts = c.s.sort_records(kct, [col], False, *c.cfg)  # (the plain rank fits)
    assert skeys.level == c.depth and souts[0].level == c.depth
    c.e.close()


def test_sharded_place_many_bitexact(ctxs):
    """A host-collective context (limbs dealt over two thread ranks) gives the
    unsplit context's residues at N = 8."""
    N, logn = SHAPES[0]
    c = ctxs[N, logn][0]
    depth, rots = sfhe.direct_sort_params(N, "oracle")
    kw = dict(mult_depth=depth + 1, ring_dim=1 << logn, batch_size=N, rotations=rots, seed=4711)

    def prog(e):
        e.set_quiet(True)
        s = e.sorter(N)
        kct = e.encrypt(make_input(N, "b").tolist())
        cols = [e.encrypt(payload(N, k).tolist()) for k in range(2)]
        placed = s.place_many(s.rank_stable(kct, *c.cfg), cols)
        skeys, souts = s.sort_records(kct, cols, True, *c.cfg)
        return {"p0": placed[0].download(), "p1": placed[1].download(), "k": skeys.download(),
                "s0": souts[0].download(), "s1": souts[1].download()}

    ref = prog(sfhe.Engine("oracle", **kw))
    outs = sfhe.run_sharded_threads("oracle", 2, prog, **kw)
    for r in range(2):
        compare(ref, outs[r])


def test_abi_lists_the_record_entry_points(oracle_lib):
    for name in ("sfhe_sorter_place_many", "sfhe_sorter_sort_records", "sfhe_sorter_records_graph_nodes",
                 "sfhe_place_counts"):
        assert hasattr(oracle_lib, name), name
