#!/usr/bin/env python3
"""A/B of the join of two encrypted tables on one GPU, through the Python binding.

One engine at join_params(N, 2)'s depth.  Per payload column count C, alternating in one process
after a warm-up, medians [min-max] of --reps rounds:
  group     Sorter.group of table B without the index: the single-table cost at this depth
  join1     Sorter.join on one key (only the A side's source differs from group)
  join2     Sorter.join on two keys (a second sign and B ORs, fused: sfp_or_tensor)
  join2_c   ... under SFHE_JOIN_FUSED=0 (each OR composed of 11 generic launches)
Before anything is timed: the one-key self-join is compared residue for residue with group, the
fused and composed two-key joins with each other, and every output is decrypted against numpy
(gate 0.01; rint of the counts exact).  Prints one JSON line.

  python tools/join_ab.py --n 256 --logn 16 --cols 1,4 --reps 7
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
    depth, rots = sfhe.join_params(N, 2, a.backend)
    e = sfhe.Engine(a.backend, mult_depth=depth, ring_dim=1 << a.logn, batch_size=N, rotations=rots, seed=1234)
    e.set_quiet(True)
    s = e.sorter(N, rotations=rots)
    rng = np.random.default_rng(5)
    # one key: B holds N/2 values twice, A all N grid values (half of A's rows unmatched);
    # two keys: a few values each, so that rows agree on one key and differ on the other
    a1, b1 = rng.permutation(N) / N, (rng.permutation(N) // 2) / N
    a2, b2 = rng.integers(0, 4, N) / N, rng.integers(0, 4, N) / N
    a3, b3 = rng.integers(0, 4, N) / N, rng.integers(0, 4, N) / N
    eq1 = a1[:, None] == b1[None, :]
    eq2 = (a2[:, None] == b2[None, :]) & (a3[:, None] == b3[None, :])
    eqg = b1[:, None] == b1[None, :]
    A1, B1, A2, B2, A3, B3 = (e.encrypt(v.tolist()) for v in (a1, b1, a2, b2, a3, b3))
    result = {"N": N, "ring": 1 << a.logn, "depth": depth, "group_depth": sfhe.group_params(N, a.backend)[0],
              "reps": a.reps, "rotation_keys": len(rots), "cols": {}}

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

    def flat(got):
        return [got["count"]] + got["sums"]

    def errors(got, eq, vals):
        err = {"count": float(np.max(np.abs(dec(got["count"]) - eq.sum(1)))),
               "sums": max(float(np.max(np.abs(dec(ct) - eq.astype(float) @ v))) for ct, v in zip(got["sums"], vals))}
        assert np.array_equal(np.rint(dec(got["count"])), eq.sum(1)), err
        assert max(err.values()) < GATE, err
        return err

    def stats(times):
        return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                    "max_ms": round(max(v), 3)} for k, v in times.items()}

    for C in [int(c) for c in a.cols.split(",")]:
        vals = [rng.permutation(N) / N * 2 - 1 for _ in range(C)]
        cols = [e.encrypt(v.tolist()) for v in vals]
        runs = {
            "group": lambda: s.group(B1, cols, False, *cfg),
            "join1": lambda: s.join([A1], [B1], cols, *cfg),
            "join2": lambda: s.join([A2, A3], [B2, B3], cols, *cfg),
            "join2_c": lambda: with_env({"SFHE_JOIN_FUSED": "0"}, lambda: s.join([A2, A3], [B2, B3], cols, *cfg)),
        }
        for fn in runs.values():
            fn()  # warm-up: masks, encodings
        e.op_stats(reset=True)
        f, c = runs["join2"](), runs["join2_c"]()
        counts = e.join_counts()
        assert counts[0] == counts[1] >= 1, counts  # one OR per batch, fused then composed
        assert all(np.array_equal(x.download(), y.download()) for x, y in zip(flat(f), flat(c))), \
            "fused and composed differ"
        g, selfj = runs["group"](), s.join([B1], [B1], cols, *cfg)
        assert all(np.array_equal(x.download(), y.download()) for x, y in
                   zip(flat(selfj), [g["count"]] + g["sums"])), "the one-key self-join differs from group"
        err = {"group": errors(g, eqg, vals), "join1": errors(runs["join1"](), eq1, vals),
               "join2": errors(f, eq2, vals)}
        times = {name: [] for name in runs}
        for _ in range(a.reps):
            for name, fn in runs.items():
                times[name].append(timed(fn)[0])
        result["cols"][str(C)] = dict(stats(times), err=err, ors_per_join2=counts[0],
                                      levels={"join1": [x.level for x in flat(runs["join1"]())],
                                              "join2": [x.level for x in flat(f)]})
    print(json.dumps(result))
    e.close()


if __name__ == "__main__":
    main()
