"""Batched encryption and the sample counters on the CPU oracle.

The oracle has no device sampler (oracle/prims_ref.c defines neither
sfp_sample_small nor sfp_encrypt_combine: weak declarations, the host layer
tests their addresses), so every small polynomial is sampled on the host and
encrypt_batch is a loop over the per-plaintext path: it must give, residue for
residue, what sequential encrypt calls give on an engine with the same seed --
the seeds are drawn in list order whatever the levels -- and sample_counts
reports (0, 3 * count)."""
import subprocess

import numpy as np

import sfhe

LOGN, DEPTH = 12, 2


def mixed_values(rng, count):
    """Negative entries and magnitudes from 1e-3 to 255."""
    mag = 10.0 ** rng.uniform(-3.0, np.log10(255.0), count)
    return [float(x) for x in mag * rng.choice([-1.0, 1.0], count)]


def test_encrypt_batch_equals_encrypt_oracle(oracle_lib):
    a, b = (sfhe.Engine("oracle", mult_depth=DEPTH, ring_dim=1 << LOGN, batch_size=8, seed=4242) for _ in range(2))
    rng = np.random.default_rng(11)
    levels = [0, DEPTH, 0, 1, DEPTH]
    inputs = [mixed_values(rng, 8) for _ in levels]
    a.op_stats(reset=True)
    batch = a.encrypt_batch(inputs, 8, levels)
    assert a.sample_counts() == (0, 3 * len(levels))
    single = [b.encrypt(v, 8, lv) for v, lv in zip(inputs, levels)]
    assert [c.level for c in batch] == levels
    assert [c.slots for c in batch] == [8] * len(levels)
    for k, (x, y) in enumerate(zip(batch, single)):
        assert np.array_equal(x.download(), y.download()), k
    # the seed counter stands where the sequential calls left it
    assert np.array_equal(a.encrypt(inputs[0], 8).download(), b.encrypt(inputs[0], 8).download())
    # levels=None is level 0 throughout; an empty list is an empty list
    more = a.encrypt_batch(inputs[:2], 8)
    assert [c.level for c in more] == [0, 0]
    for k, c in enumerate(more):
        assert np.array_equal(c.download(), b.encrypt(inputs[k], 8).download()), k
    assert a.encrypt_batch([]) == []
    got = a.decrypt(batch[1])
    assert np.allclose(got, inputs[1], rtol=0, atol=1e-4)


def test_oracle_has_no_sample_prim(oracle_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", sfhe.ORACLE_LIB], check=True, capture_output=True,
                         text=True).stdout
    assert "sfp_sample_small" not in out and "sfp_encrypt_combine" not in out
    assert "sfhe_encrypt_batch" in out and "sfhe_sample_counts" in out
