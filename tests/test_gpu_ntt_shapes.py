"""GPU parity of every branch of the NTT dispatch (nttRows in
csrc/hip/prims_hip.hip) that a default run takes, with no knob set: the same
operations on the `hip` and the `oracle` engine from the same seed, compared
bit for bit.  The smallest shapes that reach each branch:

  ring 2^11            one tile per row: the single-pass k_ntt_small
  ring 2^12            two passes over 1024-word tiles (at most 64 rows per
                       launch), LE = 2: the ModUp conversion in k_ntt's COL
                       prologue (CONV), the rescale's lift and epilogue, both
                       inverse passes
  ring 2^12, 24 limbs  key switching over more than 64 rows: the CONV prologue
                       and the forward passes over full 2048-word tiles
  ring 2^16, depth 4   k_modup_col (two targets per block: the launches of
                       this depth stay below the threshold of the wider
                       variant) and the fused key-switch pass k_ntt_ks
  ring 2^12, 40 x 2    decrypt_batch: one inverse launch over 80 rows, full
                       2048-word tiles, LE = 2

Launches of kNttSmallRows (4096) rows or more take the LE = 3 kernels.  No
call of the binding makes one: decrypt_batch works through its list in chunks
of 128 ciphertexts (context.cpp kDecryptChunk), 256 rows per launch, and the
binding has no batched forward entry point.
"""
import numpy as np
import pytest

import sfhe

pytestmark = pytest.mark.gpu

CASES = {
    "ring11": dict(mult_depth=3, ring_dim=1 << 11),
    "ring12": dict(mult_depth=3, ring_dim=1 << 12),
    "ring12_rows_gt64": dict(mult_depth=23, ring_dim=1 << 12),
    "ring16": dict(mult_depth=4, ring_dim=1 << 16),
}


def engines(**kw):
    kw = dict(batch_size=16, scaling_mod_size=40, secure=False, **kw)
    return sfhe.Engine("hip", **kw), sfhe.Engine("oracle", **kw)


@pytest.mark.parametrize("case", sorted(CASES))
def test_encrypt_mult_rotate_bitexact(hip_lib, oracle_lib, case):
    g, o = engines(seed=99, rotations=[1, -3], **CASES[case])
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-1, 1, 16).tolist(), rng.uniform(-1, 1, 16).tolist()
    outs = []
    for e in (g, o):
        x, y = e.encrypt(a), e.encrypt(b)
        m = e.mult(x, y)  # relinearise + rescale
        outs.append([x, m, e.rotate(m, 1), e.rotate(e.mult(m, x), -3)])
    for k, (cg, co) in enumerate(zip(*outs)):
        assert np.array_equal(cg.download(), co.download()), k
    got = np.array(g.decrypt(outs[0][1]))
    assert np.max(np.abs(got - np.array(a) * np.array(b))) < 1e-6
    g.close()
    o.close()


def test_decrypt_batch_over_64_rows(hip_lib, oracle_lib):
    count = 40
    g, o = engines(seed=4321, mult_depth=1, ring_dim=1 << 12)
    rng = np.random.default_rng(12)
    vals = [rng.uniform(-1, 1, 16).tolist() for _ in range(count)]
    cts = [g.encrypt(v) for v in vals]
    assert {c.info()["limbs"] for c in cts} == {2}  # count x limbs = 80 rows in one launch
    ref = [np.array(o.decrypt(o.encrypt(v))) for v in vals]
    g.op_stats(reset=True)
    batch = g.decrypt_batch(cts)
    assert g.decode_counts() == (count, 0)
    for k in range(count):
        assert np.array_equal(np.array(batch[k]), ref[k]), k
        assert np.allclose(ref[k], vals[k], rtol=0, atol=1e-6)
    g.close()
    o.close()
