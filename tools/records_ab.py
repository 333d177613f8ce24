#!/usr/bin/env python3
"""A/B of the record sort on one GPU, through the Python binding.

Per column count C, alternating in one process, medians of --reps rounds:
  composed   rank_stable + (C + 1) x place       (the entry points before sort_records: eager)
  eager      sort_records, SFHE_GRAPH=0
  graph      sort_records, captured and replayed (the default)
  cols0      ... captured under SFHE_PLACE_COLS=0 (per-column giant-step sums)
  tile2x4    ... captured under SFHE_PLACE_TILE=2x4 (the other fused tile)
Each graph variant has a sorter of its own (a captured graph keeps the knobs it
was recorded with).  Every variant's outputs are compared residue for residue
with the composed path's before anything is timed.  Prints one JSON line.

  python tools/records_ab.py --n 256 --logn 16 --cols 1,4 --reps 7
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
    ap.add_argument("--cols", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--backend", default="hip")
    a = ap.parse_args()
    N = a.n
    depth, rots = sfhe.direct_sort_params(N, a.backend)
    cfg = slotsim.default_sign_config(N)
    e = sfhe.Engine(a.backend, mult_depth=depth + 1, ring_dim=1 << a.logn, batch_size=N, rotations=rots, seed=1234)
    e.set_quiet(True)
    rng = np.random.default_rng(5)
    keys = e.encrypt(((rng.permutation(N) // 2) / N).tolist())
    knobs = {"graph": {}, "cols0": {"SFHE_PLACE_COLS": "0"}, "tile2x4": {"SFHE_PLACE_TILE": "2x4"}}
    result = {"N": N, "ring": 1 << a.logn, "depth": depth + 1, "reps": a.reps, "cols": {}}

    def timed(fn):
        e.sync()
        t = time.perf_counter()
        out = fn()
        e.sync()
        return (time.perf_counter() - t) * 1e3, out

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

    for C in [int(c) for c in a.cols.split(",")]:
        cols = [e.encrypt((rng.permutation(N) / N * 2 - 1).tolist()) for _ in range(C)]
        base = e.sorter(N)

        def composed(s=base):
            r = s.rank_stable(keys, *cfg)
            return [s.place(r, c) for c in [keys] + cols]

        def records(s):
            k, o = s.sort_records(keys, cols, True, *cfg)
            return [k] + o

        runs = {"composed": composed, "eager": lambda: with_env({"SFHE_GRAPH": "0"}, lambda: records(base))}
        sorters = {}
        for name, env in knobs.items():
            s = sorters[name] = e.sorter(N)
            with_env(env, lambda: [records(s) for _ in range(2)])  # eager, then captured
            runs[name] = (lambda s: lambda: records(s))(s)
        for name, fn in runs.items():
            fn()  # warm-up (the composed and eager paths build their masks)
            # (a sorter's sums start from its own encryption of zero: compare on the same sorter)
            ref = [c.download() for c in composed(sorters.get(name, base))]
            got = [c.download() for c in fn()]
            assert all(np.array_equal(x, y) for x, y in zip(ref, got)), name
        times = {name: [] for name in runs}
        for _ in range(a.reps):
            for name, fn in runs.items():
                times[name].append(timed(fn)[0])
        e.op_stats(reset=True)
        runs["eager"]()
        counts = e.place_counts()
        result["cols"][str(C)] = {
            "median_ms": {k: round(statistics.median(v), 3) for k, v in times.items()},
            "min_ms": {k: round(min(v), 3) for k, v in times.items()},
            "max_ms": {k: round(max(v), 3) for k, v in times.items()},
            "graph_nodes": {k: s.records_graph_nodes() for k, s in sorters.items()},
            "place_counts_eager": counts,
        }
    s = e.sorter(N)
    for _ in range(2):
        s.sort_stable(keys, *cfg)
    result["sort_stable_graph_nodes"] = s.graph_nodes()
    print(json.dumps(result))
    e.close()


if __name__ == "__main__":
    main()
