"""The HIP kernels against exact integer arithmetic and against the oracle, primitive by
primitive, on chosen residues: the cases of test_prims_exact.py (tests/prims_cases.py) run on
the product library next to the oracle, plus what only the device has -- the launches of 4096
rows (the LE = 3 NTT kernels, which no binding call reaches), sfp_tie_tensor, sfp_sample_small,
sfp_mac_plain2_cols, the weak *_add forms, sfp_const_terms_rescale, the fused key-switch
forms -- and a part of the table once more in a fresh child process with SFHE_NTT_FP=0 (every
row on the integer path): the NTT at 2^11, at 2^12 on all three limb maps and with 72 rows, at
2^16 and 2^17 (uniform row), the widest sums, rescales, conversions and the key-switch chain.
The child leaves out the 4096-row launch (128 MiB twice over) and the remaining patterns at
2^16 / 2^17.

Stated bounds the cases drive ("Primitive-level tests"):
  forward FP64 NTT, "values stay below 19q": rows fwd1 / fwd2, derived from the twiddles with
      the model of one pass's lazy butterflies (prims_harness.Ring.fwd_pass_model); modelled
      max |v|/q in (pass 1, pass 2): n = 2^12 fwd1 2.984, fwd2 4.969 (uniform 2.358, 3.432);
      n = 2^16 fwd1 4.969, fwd2 4.969 (uniform 3.773, 3.842); n = 2^17 fwd1 5.465 (uniform
      4.252) -- the whole table is in prims_cases.case_forward_pass_model;
  inverse FP64 NTT, "values below 2^9 q": the all-(q-1) evaluation row makes the untwiddled
      sum leg of a d-stage pass exactly 2^d (q-1);
  k_lin_wsum_multi, "|sum| < nin * 2q < 2^50": nin = 80, every input and weight q-1, q just
      below 2^42;
  k_mac_plain2, "up to SFP_MAX_WSUM terms stay below 2^50": nin = 80, all q-1, the same prime;
  the same sums with every term's lazy residue q/2 in magnitude and of one sign ("half":
      inputs q-1, weights (q+1)/2): |sum| = 40 q, where all-(q-1) terms are 1 each;
  sf_reduce128's 64 steps: int64 values of magnitude 2^62, 2^63-1, 2^63 and the uniform
      sampler's full words, on the 30-bit prime (the smallest the context accepts).
"""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prims_cases as K  # noqa: E402
import prims_harness as H  # noqa: E402
from _prims_params import CONV, KINDS, MAPS, RESCALE_ELL, WSUM_NIN, WSUM_NOUT  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devs(hip_lib, oracle_lib):
    return lambda primes, logn: [H.dev(hip_lib, "hip", primes, logn), H.dev(oracle_lib, "oracle", primes, logn)]


def test_load_i64(devs):
    K.case_load_i64(devs)


def test_sample_uniform(devs):
    K.case_sample_uniform(devs)


def test_sample_small(devs):
    assert K.case_sample_small(devs) == 3


@pytest.mark.parametrize("mapname", MAPS)
def test_elementwise_and_tensor(devs, mapname):
    K.case_elementwise(devs, mapname)


def test_ntt_one_tile_ring(devs):
    K.case_ntt(devs, "ident", logn=11)


@pytest.mark.parametrize("mapname", MAPS)
def test_ntt_small_tiles(devs, mapname):
    """At most 64 rows: the 1024-word tiles."""
    K.case_ntt(devs, mapname)


def test_ntt_batch_72_rows(devs):
    """More than 64 rows: the 2048-word tiles."""
    K.case_ntt_batch(devs, 8, 9)


def test_ntt_batch_4096_rows(devs):
    """kNttSmallRows rows in one launch: nttRows takes the LE = 3 kernels (128 MiB of rows)."""
    K.case_ntt_batch(devs, 512, 8)


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


def test_mac_plain2_cols(devs):
    assert K.case_mac_cols(devs) == 1


def test_mac_plain2_cols_half_32(devs):
    """nin = SFP_MAC_MULTI_N terms of lazy magnitude q/2 and one sign: 16 q a sum."""
    assert K.case_mac_cols(devs, kind="half", nin=32) == 1


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
    assert K.case_ks_chain(devs, pset, kind) == (0 if kind == "tie" else 1)


def test_ks_chain_at_2_16(devs):
    """The only ring with k_modup_col, k_moddown_col, k_ntt_ks, k_conv_mdrs, k_mdrsi, k_mdrsf."""
    assert K.case_ks_chain_large(devs) == 1


def test_const_terms_rescale_merged(devs):
    assert K.case_const_terms(devs, merged=1) == 1


def test_const_terms_rescale_one_tile_ring(devs):
    """n = 2^11: the terms go out one by one (0)."""
    assert K.case_const_terms(devs, logn=11, merged=0) == 1


def test_create_refuses_a_prime_below_the_range(hip_lib):
    """sfp_create returns null for a prime below 30 bits (modarith.h)."""
    primes = H.prime_set(11)
    primes[1] = H.prime_below(1 << 28, 1 << 12)
    with pytest.raises(AssertionError, match="sfp_create failed"):
        H.Dev(hip_lib, primes, 11)


_CHILD = """
import sys
sys.path[:0] = [%r, %r, %r]
import sfhe, prims_cases as K, prims_harness as H
hip, orc = sfhe.load('hip'), sfhe.load('oracle')
devs = lambda primes, logn: [H.dev(hip, 'hip', primes, logn), H.dev(orc, 'oracle', primes, logn)]
K.case_ntt(devs, 'ident', logn=11)
for mapname in ('ident', 'stride', 'split'):
    K.case_ntt(devs, mapname)
K.case_ntt_batch(devs, 8, 9)
K.case_ntt_large(devs, 16, names=('uniform',))
K.case_ntt_large(devs, 17, names=('uniform',))
for nin in (1, 80):
    K.case_lin_wsum(devs, nin, 'qm1')
    K.case_lin_wsum_multi(devs, nin, 9, 'qm1')
K.case_mac(devs, 80, 'qm1')
for ell in (2, 3, 7):
    K.case_rescale(devs, ell)
for ns, nbig in ((2, 1), (13, 0), (13, 2)):
    K.case_conv(devs, ns, nbig)
K.case_ks_inner(devs)
K.case_ks_chain(devs, 'mixed', 'uniform')
K.case_ks_chain(devs, 'fp', 'tie')
print('integer-path cases passed')
"""


def test_integer_path_in_a_fresh_process():
    """SFHE_NTT_FP is read once per process: a fresh child runs with SFHE_NTT_FP=0."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, SFHE_NTT_FP="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (here, root, os.path.join(root, "sorting-fhe_amd", "python"))],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "integer-path cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
