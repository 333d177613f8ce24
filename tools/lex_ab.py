#!/usr/bin/env python3
"""A/B of the sort by several keys on one GPU, through the Python binding.

Alternating in one process after a warm-up, medians [min-max] of --reps rounds:
  rank_stable      one stable rank (one key)
  rank_stable_x2   two stable ranks, one per key: the cost of two signs
  rank_lex         the lexicographic rank by two keys (fused Horner step)
  rank_lex_c       ... under SFHE_LEX_FUSED=0 (the step composed of generic launches)
and per payload column count C:
  records          sort_records (one key, stable, SFHE_GRAPH=0) of 1 + (C + 1) columns
  records_lex      sort_records_lex (two keys) of 2 + C columns: the same column count
  records_lex_c    ... under SFHE_LEX_FUSED=0
Before anything is timed the fused and composed variants' outputs are compared residue for
residue and every output is decrypted against numpy (gate 0.01).  Prints one JSON line.

  python tools/lex_ab.py --n 256 --logn 16 --cols 1,4 --reps 7
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

GATE = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--logn", type=int, default=16)
    ap.add_argument("--cols", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--backend", default="hip")
    a = ap.parse_args()
    N = a.n
    cfg = slotsim.default_sign_config(N)
    depth = sfhe.lex_sort_depth(N, cfg, 2, a.backend)
    _, rots = sfhe.direct_sort_params(N, a.backend)
    e = sfhe.Engine(a.backend, mult_depth=depth, ring_dim=1 << a.logn, batch_size=N, rotations=rots, seed=1234)
    e.set_quiet(True)
    s = e.sorter(N)
    rng = np.random.default_rng(5)
    k1, k2 = rng.integers(0, 4, N) / N, (rng.permutation(N) // 2) / N  # four groups, every value twice
    order = np.lexsort((np.arange(N), k2, k1))
    want_rank = np.argsort(order, kind="stable")
    keys = [e.encrypt(k1.tolist()), e.encrypt(k2.tolist())]
    result = {"N": N, "ring": 1 << a.logn, "depth": depth, "reps": a.reps, "cols": {}}

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

    def dec(ct):
        return np.array(e.decrypt(ct))[:N]

    def stats(times):
        return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                    "max_ms": round(max(v), 3)} for k, v in times.items()}

    composed_env = {"SFHE_LEX_FUSED": "0"}
    runs = {
        "rank_stable": lambda: s.rank_stable(keys[0], *cfg),
        "rank_stable_x2": lambda: [s.rank_stable(k, *cfg) for k in keys],
        "rank_lex": lambda: s.rank_lex(keys, None, *cfg),
        "rank_lex_c": lambda: with_env(composed_env, lambda: s.rank_lex(keys, None, *cfg)),
    }
    for fn in runs.values():
        fn()  # warm-up: masks, encodings
    e.op_stats(reset=True)
    fused, composed = runs["rank_lex"](), runs["rank_lex_c"]()
    result["lex_counts"] = e.lex_counts()
    assert np.array_equal(fused.download(), composed.download()), "fused and composed ranks differ"
    got = dec(fused)
    result["rank_err"] = float(np.max(np.abs(got - want_rank)))
    assert np.array_equal(np.rint(got), want_rank), result["rank_err"]
    times = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, fn in runs.items():
            times[name].append(timed(fn)[0])
    result["rank"] = stats(times)

    for C in [int(c) for c in a.cols.split(",")]:
        vals = [rng.permutation(N) / N * 2 - 1 for _ in range(C + 1)]
        cols = [e.encrypt(v.tolist()) for v in vals]
        key1 = keys[0].clone()  # (a placement leaves its inputs at the partition's slot count)

        def records():
            k, o = s.sort_records(key1, cols, True, *cfg)
            return [k] + o

        def records_lex():
            k, o = s.sort_records_lex(keys, cols[:C], None, *cfg)
            return k + o

        cruns = {
            "records": lambda: with_env({"SFHE_GRAPH": "0"}, records),
            "records_lex": records_lex,
            "records_lex_c": lambda: with_env(composed_env, records_lex),
        }
        for fn in cruns.values():
            fn()
        f, c = cruns["records_lex"](), cruns["records_lex_c"]()
        assert all(np.array_equal(x.download(), y.download()) for x, y in zip(f, c)), "fused / composed differ"
        err = max(float(np.max(np.abs(dec(ct) - v[order]))) for ct, v in zip(f, [k1, k2] + vals[:C]))
        assert err < GATE, err
        by_primary = np.argsort(k1, kind="stable")
        err1 = max(float(np.max(np.abs(dec(ct) - v[by_primary]))) for ct, v in zip(cruns["records"](), [k1] + vals))
        assert err1 < GATE, err1
        times = {name: [] for name in cruns}
        for _ in range(a.reps):
            for name, fn in cruns.items():
                times[name].append(timed(fn)[0])
        result["cols"][str(C)] = dict(stats(times), output_err=err)
    print(json.dumps(result))
    e.close()


if __name__ == "__main__":
    main()
