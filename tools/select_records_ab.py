#!/usr/bin/env python3
"""A/B of the record selection on one GPU, through the Python binding.

ORDER BY key LIMIT K over rows of a key and C payload columns, stable rank,
alternating in one process, medians and ranges of --reps rounds after warm-up:
  a  separate   rank_stable + (C + 1) x select_ranked (the only way before select_records)
  b  records    select_records, defaults (shared indicator, column-tiled fold kernel)
  c  cols0      select_records under SFHE_SELECT_COLS=0 (shared indicator, folds per column)
  d  tile       select_records under SFHE_SELECT_TILE=<the other tile width>
Before anything is timed every variant's outputs are compared residue for
residue with the separate select_ranked calls, decrypted and compared with
numpy (gate 0.01), and the counters are checked to say which path ran.
Prints one JSON line; --md writes the table.

  python tools/select_records_ab.py --n 256 --logn 16 --ks 1,16,128 --cs 1,4 --reps 7
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

VARIANTS = ["separate", "records", "cols0", "tile"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--logn", type=int, default=16)
    ap.add_argument("--ks", default="1,16,128")
    ap.add_argument("--cs", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--backend", default="hip")
    ap.add_argument("--default-tile", type=int, default=2, help="prims_hip.hip kFoldTileDefault")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    N = a.n
    depth, rots = sfhe.select_params(N, a.backend)
    depth += 1  # the stable rank
    cfg = slotsim.default_sign_config(N)
    kw = dict(n=cfg[0], dg=cfg[1], df=cfg[2])
    other_tile = 2 if a.default_tile == 4 else 4
    e = sfhe.Engine(a.backend, mult_depth=depth, ring_dim=1 << a.logn, batch_size=N, rotations=rots, seed=1234)
    e.set_quiet(True)
    s = e.sorter(N, rotations=rots)
    ks = [int(k) for k in a.ks.split(",")]
    cs = [int(c) for c in a.cs.split(",")]
    x = np.random.default_rng(5).permutation(N) / N
    i = np.arange(N)
    cols = [x] + [np.cos((j + 1) * i + j) for j in range(max(cs))]
    cts = [e.encrypt(v.tolist()) for v in cols]
    order = np.argsort(x)

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

    def separate(K, C):
        rank = s.rank_stable(cts[0], *cfg)
        return [s.select_ranked(rank, ct, list(range(K))) for ct in cts[: C + 1]]

    def records(K, C):
        k, outs = s.select_records(cts[0], cts[1: C + 1], list(range(K)), stable=True, **kw)
        return [k] + outs

    envs = {"separate": {}, "records": {}, "cols0": {"SFHE_SELECT_COLS": "0"},
            "tile": {"SFHE_SELECT_TILE": str(other_tile)}}
    runs = {}
    for K in ks:
        for C in cs:
            for v in VARIANTS:
                fn = separate if v == "separate" else records
                runs[K, C, v] = (lambda fn, K, C, env: lambda: with_env(env, lambda: fn(K, C)))(fn, K, C, envs[v])

    def timed(fn):
        e.sync()
        t = time.perf_counter()
        fn()
        e.sync()
        return (time.perf_counter() - t) * 1e3

    # checks (these calls are also the warm-up: masks, plaintext encodings)
    hip = a.backend == "hip"  # (the oracle has no tiled kernel: a rehearsal of this tool only)
    max_err = 0.0
    for K in ks:
        for C in cs:
            ref = [o.download() for o in runs[K, C, "separate"]()]
            for v in VARIANTS[1:]:
                e.op_stats(reset=True)
                outs = runs[K, C, v]()
                columns, fused, composed = e.select_cols_counts()
                assert columns == C + 1, (K, C, v, columns)
                if hip:
                    assert (fused == 0 and composed > 0) if v == "cols0" else (fused > 0 and composed == 0), \
                        (K, C, v, fused, composed)
                for c, (out, want) in enumerate(zip(outs, ref)):
                    assert np.array_equal(out.download(), want), f"K={K} C={C} {v}: column {c} differs"
                    dec = np.array(e.decrypt(out))[:N]
                    err = float(np.max(np.abs(dec - np.r_[cols[c][order][:K], np.zeros(N - K)])))
                    assert err < 0.01, (K, C, v, c, err)
                    max_err = max(max_err, err)
    times = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    rows = []
    for K in ks:
        for C in cs:
            row = {"K": K, "C": C}
            for v in VARIANTS:
                t = times[K, C, v]
                row[v] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3),
                          "max_ms": round(max(t), 3)}
            row["separate_over_records"] = round(row["separate"]["median_ms"] / row["records"]["median_ms"], 3)
            rows.append(row)
    result = {"N": N, "ring": 1 << a.logn, "depth": depth, "reps": a.reps, "sign": list(cfg), "stable": True,
              "default_tile": a.default_tile, "other_tile": other_tile, "max_err": float(f"{max_err:.3g}"),
              "rows": rows}
    print(json.dumps(result))
    if a.md:
        def cell(r):
            return f"{r['median_ms']:.1f} [{r['min_ms']:.1f}–{r['max_ms']:.1f}]"
        lines = [f"N = {N}, ring 2^{a.logn}, depth {depth}, stable, CompositeSign{tuple(cfg)}, {a.reps} alternating "
                 f"rounds, median [min–max] ms; default tile CT = {a.default_tile}", "",
                 f"| K | C | (a) rank_stable + (C+1) × select_ranked | (b) select_records | (c) SFHE_SELECT_COLS=0 | "
                 f"(d) SFHE_SELECT_TILE={other_tile} | (a)/(b) |", "|---|---|---|---|---|---|---|"]
        for r in rows:
            lines.append(f"| {r['K']} | {r['C']} | " + " | ".join(cell(r[v]) for v in VARIANTS) +
                         f" | {r['separate_over_records']:.2f}× |")
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    e.close()


if __name__ == "__main__":
    main()
