"""The sign's odd polynomials issued wave by wave (SFHE_SIGN_BATCH, default
on) against the one-op-at-a-time order (SFHE_SIGN_BATCH=0), on the CPU oracle.

The oracle never merges launches, so this pins the host-side reordering
alone: the same tree, levels, coefficient terms, aligned powers and sums must
give the same residues whichever order issues them.  The knob is read once
per process, so each setting runs in a fresh child.
"""
import json
import os
import re
import subprocess
import sys

_CHILD = r"""
import hashlib, json
import sfhe
from oracle import slotsim

def digest(ct):
    return [int(ct.level), hashlib.sha256(ct.download().tobytes()).hexdigest()]

out = {}
v = [0.02, -0.02, 0.01, -0.01, 0.4, -0.6, 1, -1]
for cfg, depth in (((3, 2, 2), 12), ((4, 1, 1), 9)):
    e = sfhe.Engine("oracle", mult_depth=depth, ring_dim=1 << 12, batch_size=8, scaling_mod_size=50, seed=1234)
    out["sign%d%d%d" % cfg] = digest(e.sign(e.encrypt(v), *cfg))
N = 8
depth, rots = sfhe.direct_sort_params(N, "oracle")
e = sfhe.Engine("oracle", mult_depth=depth, ring_dim=1 << 12, batch_size=N, rotations=rots, seed=5)
e.set_quiet(True)
x = slotsim.input_vector(N).tolist()
out["sort8"] = digest(e.sorter(N).sort(e.encrypt(x), *slotsim.default_sign_config(N)))
out["ops"] = e.op_stats()
print("RESULT " + json.dumps(out))
"""


def _run(knob):
    env = dict(os.environ)
    env.pop("SFHE_SIGN_BATCH", None)
    if knob is not None:
        env["SFHE_SIGN_BATCH"] = knob
    env["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(re.search(r"RESULT (.*)", r.stdout).group(1))


def test_oracle_same_residues_knob_on_and_off(oracle_lib):
    on, off = _run(None), _run("0")
    print(on)
    assert on["sign322"][0] == 12 and on["sign411"][0] == 9
    for k in ("sign322", "sign411", "sort8"):
        assert on[k] == off[k], (k, on[k], off[k])
    # the same ops were counted: nothing added, nothing dropped
    assert on["ops"] == off["ops"]
