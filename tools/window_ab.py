#!/usr/bin/env python3
"""A/B of the window sums over an encrypted key on one GPU, through the Python binding.

Per payload column count C, alternating in one process after a warm-up, medians [min-max] of
--reps rounds:
  rank_stable   one stable rank at the same depth: the cost of the sign and its tie term alone
  window        Sorter.window with the count and C columns (fused weighted sums)
  window_c      ... under SFHE_WINDOW_FUSED=0 (the weighted sums composed of generic launches)
Before anything is timed the fused and composed variants' outputs are compared residue for
residue and every output of every frame is decrypted against numpy (gate 0.01; rint of the count
exact).  The timed frame is --frame.  Prints one JSON line.

  python tools/window_ab.py --n 256 --logn 16 --cols 1,4 --reps 7
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


def members(k, frame):
    """member[r, j]: row j is in row r's frame"""
    idx = np.arange(len(k))
    less, eq = k[None, :] < k[:, None], k[None, :] == k[:, None]
    if frame == "rows":
        return less | (eq & (idx[None, :] <= idx[:, None]))
    return less | eq if frame == "range" else less


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--logn", type=int, default=16)
    ap.add_argument("--cols", default="1,4")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frame", default="rows", choices=sorted(sfhe.FRAMES))
    ap.add_argument("--backend", default="hip")
    a = ap.parse_args()
    N = a.n
    cfg = slotsim.default_sign_config(N)
    depth, rots = sfhe.window_params(N, a.backend)
    e = sfhe.Engine(a.backend, mult_depth=depth, ring_dim=1 << a.logn, batch_size=N, rotations=rots, seed=1234)
    e.set_quiet(True)
    s = e.sorter(N, rotations=rots)
    rng = np.random.default_rng(5)
    sizes = [N // 2, N // 4, N // 8, N - N // 2 - N // 4 - N // 8]  # four groups of uneven sizes
    k = rng.permutation(np.repeat(np.arange(4), sizes)) / N
    key = e.encrypt(k.tolist())
    result = {"N": N, "ring": 1 << a.logn, "depth": depth, "reps": a.reps, "rotation_keys": len(rots),
              "frame": a.frame, "cols": {}}

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

    def stats(times):
        return {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                    "max_ms": round(max(v), 3)} for k, v in times.items()}

    def check(got, frame, vals):
        member = members(k, frame)
        err = {"count": float(np.max(np.abs(dec(got["count"]) - member.sum(1)))),
               "sums": max(float(np.max(np.abs(dec(ct) - member.astype(float) @ v)))
                           for ct, v in zip(got["sums"], vals))}
        assert np.array_equal(np.rint(dec(got["count"])), member.sum(1)), (frame, err)
        assert max(err.values()) < GATE, (frame, err)
        return err

    for C in [int(c) for c in a.cols.split(",")]:
        vals = [rng.permutation(N) / N * 2 - 1 for _ in range(C)]
        cols = [e.encrypt(v.tolist()) for v in vals]
        runs = {
            "rank_stable": lambda: s.rank_stable(key, *cfg),
            "window": lambda: s.window(key, cols, a.frame, True, *cfg),
            "window_c": lambda: with_env({"SFHE_WINDOW_FUSED": "0"},
                                         lambda: s.window(key, cols, a.frame, True, *cfg)),
        }
        for fn in runs.values():
            fn()  # warm-up: masks, encodings
        e.op_stats(reset=True)
        f, c = runs["window"](), runs["window_c"]()
        counts = e.window_counts()
        assert counts == (1, 1), counts
        assert all(np.array_equal(x.download(), y.download()) for x, y in zip(flat(f), flat(c))), \
            "fused and composed differ"
        err = {a.frame: check(f, a.frame, vals)}
        for frame in sorted(set(sfhe.FRAMES) - {a.frame}):
            err[frame] = check(s.window(key, cols, frame, True, *cfg), frame, vals)
        times = {name: [] for name in runs}
        for _ in range(a.reps):
            for name, fn in runs.items():
                times[name].append(timed(fn)[0])
        result["cols"][str(C)] = dict(stats(times), err=err, levels=[x.level for x in flat(f)])
    print(json.dumps(result))
    e.close()


if __name__ == "__main__":
    main()
