"""Merged launches whose groups do not fill their argument-set slots.

A batch of w independent products becomes one launch per step whose
ArgSet<T, NG> is the next of 2 / 4 / 8 sets: at 3 ops an ArgSet<T, 4>, at 5
and at 7 an ArgSet<T, 8>, the unused slots padded with the last set, which
gets no rows (launchSets' concatenated path; the default width of 8 and
groups of 2 or 4 fill their slots and alternate rows instead).

Shape: a dense Chebyshev series of degree 200 at ring 2^12 -- 16 baby steps,
so the ladder's wave T_9..T_16 is eight independent products, which
SFHE_BATCH_WIDTH = 3 / 5 / 7 cuts into batches of 3+3+2, 5+3 and 7+1.
Residues are compared, never decryptions: a merged launch computes the same
integers as the separate launches, and the oracle never merges.

SFHE_BATCH_WIDTH is read once per process: every width runs in a fresh child.
"""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_CHILD = r"""
import hashlib, json
import numpy as np
import sfhe
rng = np.random.default_rng(7)
c = rng.uniform(0.05, 0.4, 201) * rng.choice([-1.0, 1.0], 201) / 201
x = np.linspace(-0.9, 0.9, 8)
out = {}
for backend in ("hip", "oracle"):
    e = sfhe.Engine(backend, mult_depth=9, ring_dim=1 << 12, batch_size=8, scaling_mod_size=40, secure=False, seed=4321)
    e.set_quiet(True)
    ct = e.encrypt(x.tolist())
    e.sync()
    m0, s0 = e.stack_stats()
    h = e.chebyshev(ct, c.tolist())
    e.sync()
    m1, s1 = e.stack_stats()
    out[backend] = dict(level=int(h.level), sha=hashlib.sha256(h.download().tobytes()).hexdigest(),
                        merged=m1 - m0, single=s1 - s0)
print("RESULT " + json.dumps(out))
"""


def _child(width):
    env = dict(os.environ)
    for k in ("SFHE_BATCH_WIDTH", "SFHE_BATCH", "SFHE_PS_L", "SFHE_PS_UNBATCHED", "SFHE_PS_LANES"):
        env.pop(k, None)
    if width:
        env["SFHE_BATCH_WIDTH"] = str(width)
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(re.search(r"RESULT (.*)", r.stdout).group(1))
    print("width", width or "default", res)
    return res


@pytest.fixture(scope="module")
def default_run(hip_lib, oracle_lib):
    return _child(None)


def test_default_width(default_run):
    r = default_run
    assert r["hip"]["sha"] == r["oracle"]["sha"] and r["hip"]["level"] == r["oracle"]["level"]
    assert r["hip"]["merged"] > 0 and r["oracle"]["merged"] == 0


@pytest.mark.parametrize("width", [3, 5, 7])
def test_padded_width(hip_lib, oracle_lib, default_run, width):
    r = _child(width)
    assert r["hip"]["sha"] == r["oracle"]["sha"] and r["hip"]["level"] == r["oracle"]["level"]
    assert r["hip"]["sha"] == default_run["hip"]["sha"]
    assert r["hip"]["merged"] > 0 and r["oracle"]["merged"] == 0
