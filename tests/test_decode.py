"""Batched decryption and the decode counters on the CPU oracle.

The oracle has no device decoder (oracle/prims_ref.c defines no sfp_decode*
symbol: the prim is a weak declaration and the host layer tests its address),
so every decryption is decoded on the host: decrypt_batch loops over the
per-ciphertext path and must return exactly what decrypt returns, and
decode_counts reports (0, k).  The oracle_lib fixture also covers that the
oracle library still builds from the same context.cpp and loads (ctypes binds
with RTLD_NOW) without the prim."""
import subprocess

import numpy as np

import sfhe

LOGN, DEPTH = 12, 2


def mixed_values(rng, count):
    """Negative entries and magnitudes from 1e-3 to 255."""
    mag = 10.0 ** rng.uniform(-3.0, np.log10(255.0), count)
    return [float(x) for x in mag * rng.choice([-1.0, 1.0], count)]


def mixed_cts(e, half):
    rng = np.random.default_rng(7)
    cts = []
    for slots in (1, 8, half):
        for level in (0, DEPTH):
            cts.append(e.encrypt(mixed_values(rng, slots), slots, level))
    return cts


def test_decrypt_batch_equals_decrypt_oracle(oracle_lib):
    e = sfhe.Engine("oracle", mult_depth=DEPTH, ring_dim=1 << LOGN, batch_size=8, seed=4242)
    cts = mixed_cts(e, 1 << (LOGN - 1))
    assert sorted({c.info()["limbs"] for c in cts})[0] == 1  # the last level: one limb
    assert max(c.info()["limbs"] for c in cts) >= 2
    e.op_stats(reset=True)
    single = [e.decrypt(c) for c in cts]
    assert e.decode_counts() == (0, len(cts))
    batch = e.decrypt_batch(cts)
    assert e.decode_counts() == (0, 2 * len(cts))
    assert [len(v) for v in batch] == [c.slots for c in cts]
    for k, (a, b) in enumerate(zip(single, batch)):
        assert np.array_equal(np.array(a), np.array(b)), k
    assert e.decrypt_batch([]) == []
    # the values are the inputs' (sanity: the exact comparison above is the check)
    assert abs(single[0][0]) > 0


def test_decrypt_once(oracle_lib):
    """Engine.decrypt takes the slot count from sfhe_ct_info: one decryption per call."""
    e = sfhe.Engine("oracle", mult_depth=DEPTH, ring_dim=1 << LOGN, batch_size=8, seed=4242)
    ct = e.encrypt([0.5, -0.25, 3.0], 8)
    e.op_stats(reset=True)
    v = e.decrypt(ct)
    assert len(v) == 8 and np.allclose(v[:3], [0.5, -0.25, 3.0], atol=1e-6)
    assert e.decode_counts() == (0, 1)


def test_oracle_has_no_decode_prim(oracle_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", sfhe.ORACLE_LIB], check=True, capture_output=True,
                         text=True).stdout
    assert "sfp_decode" not in out
    assert "sfhe_decrypt_batch" in out and "sfhe_decode_counts" in out
