#!/usr/bin/env python3
"""A/B of the selection by rank on one GPU, through the Python binding.

Alternating in one process, medians and ranges of --reps rounds:
  sort_graph   sort(), captured and replayed (its default): the only way to these values before
  sort_eager   sort(), SFHE_GRAPH=0
  rank         rank() alone (the part a selection shares with the sort)
  select_K     select(range(K)), eager (it is never captured), fused folds (the default)
  select_K_f0  ... under SFHE_SELECT_FOLD=0 (the folds composed of the generic prims)
Before anything is timed every selection is decrypted and compared with numpy
(gate 0.01), the two fold forms are compared residue for residue, and with
--oracle the fused form is compared residue for residue with the C oracle's
select on the same seed (slow at the metric configuration: minutes per call).
Prints one JSON line.

  python tools/select_ab.py --n 256 --logn 16 --ks 1,16,128,256 --reps 7
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sorting-fhe_amd", "python")]

import numpy as np  # noqa: E402

import sfhe  # noqa: E402
from oracle import slotsim  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--logn", type=int, default=16)
    ap.add_argument("--ks", default="1,16,128,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--backend", default="hip")
    ap.add_argument("--oracle", action="store_true")
    a = ap.parse_args()
    N = a.n
    depth, rots = sfhe.select_params(N, a.backend)
    cfg = slotsim.default_sign_config(N)
    seed = 1234

    def engine(backend):
        e = sfhe.Engine(backend, mult_depth=depth, ring_dim=1 << a.logn, batch_size=N, rotations=rots, seed=seed)
        e.set_quiet(True)
        return e

    e = engine(a.backend)
    x = np.random.default_rng(5).permutation(N) / N
    ct = e.encrypt(x.tolist())
    ks = [int(k) for k in a.ks.split(",")]
    result = {"N": N, "ring": 1 << a.logn, "depth": depth, "reps": a.reps, "sign": list(cfg)}

    def timed(fn):
        e.sync()
        t = time.perf_counter()
        fn()
        e.sync()
        return (time.perf_counter() - t) * 1e3

    def with_env(env, fn):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return fn()
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    graph, eager, sel = e.sorter(N, rotations=rots), e.sorter(N, rotations=rots), e.sorter(N, rotations=rots)
    kw = dict(n=cfg[0], dg=cfg[1], df=cfg[2])
    runs = {
        "sort_graph": lambda: graph.sort(ct, *cfg),
        "sort_eager": lambda: with_env({"SFHE_GRAPH": "0"}, lambda: eager.sort(ct, *cfg)),
        "rank": lambda: sel.rank(ct, *cfg),
    }
    for K in ks:
        runs[f"select_{K}"] = (lambda K: lambda: sel.select(ct, list(range(K)), **kw))(K)
        runs[f"select_{K}_f0"] = (lambda K: lambda: with_env({"SFHE_SELECT_FOLD": "0"},
                                                             lambda: sel.select(ct, list(range(K)), **kw)))(K)
    # checks (these calls are also the warm-up: masks, the sort's capture)
    xs = np.sort(x)
    errs = {}
    for _ in range(3):
        out = runs["sort_graph"]()
    errs["sort"] = float(np.max(np.abs(np.array(e.decrypt(out))[:N] - xs)))
    runs["sort_eager"]()
    runs["rank"]()
    oracle = engine("oracle") if a.oracle else None
    for K in ks:
        e.op_stats(reset=True)
        fused = runs[f"select_{K}"]()
        counts = e.select_counts()
        hip = a.backend == "hip"  # (the oracle has no fused fold: a rehearsal of this tool only)
        assert not hip or (counts[1] > 0 and counts[2] == 0), counts
        e.op_stats(reset=True)
        comp = runs[f"select_{K}_f0"]()
        c0 = e.select_counts()
        assert not hip or (c0[1] == 0 and c0[2] == counts[1]), c0
        assert np.array_equal(fused.download(), comp.download()), f"K={K}: fused and composed folds differ"
        want = np.r_[xs[:K], np.zeros(N - K)]
        errs[f"select_{K}"] = float(np.max(np.abs(np.array(e.decrypt(fused))[:N] - want)))
        assert errs[f"select_{K}"] < 0.01, (K, errs)
        if oracle:
            ref = oracle.sorter(N, rotations=rots).select(oracle.encrypt(x.tolist()), list(range(K)), **kw)
            assert np.array_equal(fused.download(), ref.download()), f"K={K}: differs from the oracle"
        result.setdefault("batches", {})[str(K)] = counts[0]
    assert errs["sort"] < 0.01, errs
    result["max_err"] = {k: float(f"{v:.3g}") for k, v in errs.items()}
    result["oracle_checked"] = bool(oracle)
    times = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            times[name].append(timed(fn))
    result["median_ms"] = {k: round(statistics.median(v), 3) for k, v in times.items()}
    result["min_ms"] = {k: round(min(v), 3) for k, v in times.items()}
    result["max_ms"] = {k: round(max(v), 3) for k, v in times.items()}
    result["sort_graph_nodes"] = graph.graph_nodes()
    print(json.dumps(result))
    e.close()


if __name__ == "__main__":
    main()
