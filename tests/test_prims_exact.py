"""The C oracle against exact integer arithmetic, primitive by primitive, on chosen residues.

Every GPU parity claim rests on the oracle; this is its own check, against the
definitions of prims.h restated in Python integers (tests/prims_harness.py) on
the prime sets and residue patterns of tests/prims_cases.py: primes of 30 (the
context's lower limit), 32, just below and just above 42, 50 and just below 60
bits; 0, 1, q-1, q/2, deltas at the tile borders, alternating rows, one seeded
uniform row.  The same cases run on the HIP library in test_gpu_prims_exact.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prims_cases as K  # noqa: E402
import prims_harness as H  # noqa: E402
from _prims_params import CONV, KINDS, MAPS, RESCALE_ELL, WSUM_NIN, WSUM_NOUT  # noqa: E402


@pytest.fixture(scope="module")
def devs(oracle_lib):
    return lambda primes, logn: [H.dev(oracle_lib, "oracle", primes, logn)]


def test_reference_ntt_is_the_definition():
    K.case_reference_ntt_definition()


@pytest.mark.parametrize("logn", [12, 16])
def test_forward_pass_model_rows_exceed_the_uniform_row(logn):
    """The sign-aligned rows fwd1 / fwd2 of the NTT cases drive their forward FP64 pass further
    than the uniform row does (figures: prims_cases.case_forward_pass_model)."""
    K.case_forward_pass_model(logn)


def test_forward_pass_model_is_the_transform():
    """The model's network, reduced, is the exact NTT: it models the transform the kernels run."""
    R = H.ring(H.prime_set(12), 12)
    for name in ("uniform", "fwd2"):
        a = K.ntt_reference(R, H.ident(9))[name][0][2]
        q, n, tw = R.primes[2], R.n, R.psi_rev(2)
        v = H.obj(a)
        for S in range(12):
            m, t = 1 << S, n >> (S + 1)
            v = v.reshape(m, 2, t)
            r = v[:, 1, :] * tw[m:2 * m].reshape(m, 1) % q
            v = np.stack([(v[:, 0, :] + r) % q, (v[:, 0, :] - r) % q], axis=1).reshape(n)
        assert np.array_equal(v, R.ntt(a, 2))


def test_reference_automorphism_is_the_substitution():
    K.case_reference_automorph()


def test_tables_match_the_engine(oracle_lib):
    """The Python tables for an engine context's own primes(): the library's NTT under them is
    the exact NTT (a wrong psi power, table order, Shoup companion or n^-1 breaks it), and the
    context's ciphertext rows are canonical residues of those primes.  (The engine exposes no
    plaintext NTT row, so its own choice of psi is not compared.)"""
    import sfhe
    e = sfhe.Engine("oracle", mult_depth=2, ring_dim=1 << 11, batch_size=8, seed=3)
    primes = [int(q) for q in e.primes()]
    R = H.ring(primes, 11)
    D = H.dev(oracle_lib, "oracle", primes, 11)
    m = H.ident(len(primes))
    a = H.pattern_polys(R, m)["uniform"]
    p = D.up(H.u64(a))
    D.call("sfp_ntt", p, m, 0)
    H.assert_eq(D.down(p, (m.count, R.n)), H.exact_rows(R, m, a, R.ntt), "ntt under the engine's primes")
    D.release()
    ct = e.encrypt([0.5] * 8)
    raw = np.asarray(ct.download()).reshape(2, -1, R.n)
    for i in range(raw.shape[1]):
        assert int(raw[:, i].max()) < primes[i]


@pytest.mark.parametrize("bits", [20, 28, 29])
def test_context_refuses_primes_below_the_reductions_range(bits):
    """modarith.h: a full word is outside sf_reduce128's 64 correction steps below 30 bits."""
    import sfhe
    with pytest.raises(Exception, match="scaling mod size"):
        sfhe.Engine("oracle", mult_depth=1, ring_dim=1 << 11, batch_size=8, scaling_mod_size=bits,
                    first_mod_size=60, seed=1)


def test_context_accepts_the_lower_limit():
    import sfhe
    e = sfhe.Engine("oracle", mult_depth=1, ring_dim=1 << 11, batch_size=8, scaling_mod_size=H.MIN_PRIME_BITS,
                    first_mod_size=60, seed=1)
    assert min(int(q) for q in e.primes()).bit_length() >= H.MIN_PRIME_BITS


def test_load_i64(devs):
    K.case_load_i64(devs)


def test_sample_uniform(devs):
    K.case_sample_uniform(devs)


@pytest.mark.parametrize("mapname", MAPS)
def test_elementwise_and_tensor(devs, mapname):
    K.case_elementwise(devs, mapname)


def test_ntt_one_tile_ring(devs):
    K.case_ntt(devs, "ident", logn=11)


@pytest.mark.parametrize("mapname", MAPS)
def test_ntt(devs, mapname):
    K.case_ntt(devs, mapname)


def test_ntt_batch_72_rows(devs):
    K.case_ntt_batch(devs, 8, 9)


@pytest.mark.parametrize("logn", [16, 17])
def test_ntt_large_rings(devs, logn):
    K.case_ntt_large(devs, logn, names=("uniform", "qm1", "fwd1") if logn == 17 else ("uniform", "qm1", "alt0", "fwd1", "fwd2"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nin", WSUM_NIN)
def test_lin_wsum(devs, nin, kind):
    K.case_lin_wsum(devs, nin, kind)


@pytest.mark.parametrize("nout", WSUM_NOUT)
@pytest.mark.parametrize("nin", WSUM_NIN)
def test_lin_wsum_multi(devs, nin, nout):
    K.case_lin_wsum_multi(devs, nin, nout, "qm1")


def test_lin_wsum_multi_half(devs):
    """80 terms of lazy magnitude q/2 and one sign: |sum| = 40 q, the largest a sum reaches."""
    K.case_lin_wsum_multi(devs, 80, 9, "half")


def test_lin_wsum_multi_uniform(devs):
    K.case_lin_wsum_multi(devs, 5, 9, "uniform")


@pytest.mark.parametrize("kind", KINDS)
def test_mac_plain_80(devs, kind):
    K.case_mac(devs, 7 if kind == "uniform" else 80, kind)


@pytest.mark.parametrize("kind", ["qm1", "half"])
def test_mac_plain2_multi_8x32(devs, kind):
    K.case_mac_multi(devs, 8, 32, kind)


def test_mac_plain2_multi_uniform(devs):
    K.case_mac_multi(devs, 3, 5, "uniform")


def test_mac_plain2_multi_refused(devs):
    K.case_mac_multi_refused(devs)


@pytest.mark.parametrize("mapname", MAPS)
def test_automorph(devs, mapname):
    K.case_automorph(devs, mapname)


@pytest.mark.parametrize("ell", RESCALE_ELL)
def test_rescale(devs, ell):
    K.case_rescale(devs, ell)


def test_rescale_ext(devs):
    K.case_rescale_ext(devs)


@pytest.mark.parametrize("mapname", ["stride", "split"])
def test_rescale_rows(devs, mapname):
    K.case_rescale_rows(devs, mapname)


@pytest.mark.parametrize("ns,nbig", CONV)
def test_conv(devs, ns, nbig):
    K.case_conv(devs, ns, nbig)


def test_ks_inner_family(devs):
    K.case_ks_inner(devs)


@pytest.mark.parametrize("kind", ["uniform", "qm1", "tie"])
@pytest.mark.parametrize("pset", ["mixed", "fp"])
def test_ks_chain(devs, pset, kind):
    """ModUp, inner product, ModDown (add both ways, P rows next to a centring tie) and
    ModDown + rescale at ell = 5, K = 2, alpha = 2 (a ragged last digit); the fused forms
    where the library has them."""
    assert K.case_ks_chain(devs, pset, kind) == 0


def test_ks_chain_at_2_16(devs):
    """The only ring with k_modup_col, k_moddown_col, k_ntt_ks, k_conv_mdrs, k_mdrsi, k_mdrsf."""
    assert K.case_ks_chain_large(devs) == 0
