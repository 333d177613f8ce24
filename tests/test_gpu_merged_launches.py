"""The code of prims_hip.hip that glues several launches into one ("Stacked launches":
issueSets, launchSets, argSel, issueY / YPay, stackMerge, mergeSets, stackFlush), on its own:
the cases of tests/merge_cases.py on the product library next to the oracle.  Every case
issues independent ops on their own buffers inside one sfp_batch_begin / sfp_stack_begin
region -- shapes the evaluators do not currently produce: unequal row counts, padded groups of
3, 5, 6, 7 sets, element-wise groups above four, conversions of different depth, ModDown
heads at different levels, both transform directions and both tile sizes in one region,
waits, a flush in the middle, a capture -- and asserts integer equality with the exact
reference on every row, the fill value past every op's rows, and the (merged, single) delta
of sfp_stack_stats, which merge_cases.flush_model derives from stackFlush's rule.

Cases 1 to 4 run once more in a fresh child process with SFHE_NTT_FP=0 (the integer-path
forms of the merged kernels; the knob is read once per process).  SFHE_BATCH and SFHE_STACK
are left at their defaults (on).
"""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_cases as M  # noqa: E402
import prims_harness as H  # noqa: E402

pytestmark = pytest.mark.gpu

EW_COUNTS = [2, 3, 4, 5, 8]
CHAIN_COUNTS = [2, 3, 4]


@pytest.fixture(scope="module")
def devs(hip_lib, oracle_lib):
    return lambda primes, logn: [H.dev(hip_lib, "hip", primes, logn), H.dev(oracle_lib, "oracle", primes, logn)]


@pytest.mark.parametrize("count", EW_COUNTS)
@pytest.mark.parametrize("prim", M.EW_PRIMS)
def test_elementwise_family_in_a_batch(devs, prim, count):
    """k_ew, k_automorph, k_lin_wsum, k_ks_inner as dim3(max grid.x, count) over argument sets of
    different maps, nin, Galois elements, beta / ell; 5 = 4 + 1 and 8 = 4 + 4."""
    M.case_ew_batch(devs, (prim,), count)


def test_two_prims_in_one_batch(devs):
    M.case_ew_batch(devs, ("add", "mul"), 4)


@pytest.mark.parametrize("count", [2, 3, 4, 5, 6, 7, 8])
def test_ntt_batch_equal_maps(devs, count):
    """2, 4, 8: interleaved rows; 3, 5, 6, 7: padded to ArgSet<T, 4 / 8> and concatenated."""
    M.case_ntt_batch(devs, "equal", count)


@pytest.mark.parametrize("count", [4, 7])
def test_ntt_batch_unequal_maps(devs, count):
    M.case_ntt_batch(devs, "unequal", count)


def test_ntt_batch_both_directions(devs):
    M.case_ntt_batch(devs, "directions", 4)


def test_ntt_batch_both_tile_sizes(devs):
    M.case_ntt_batch_tiles(devs)


@pytest.mark.parametrize("count", [2, 3, 8])
def test_conversions_in_a_batch(devs, count):
    M.case_conv_batch(devs, count)


@pytest.mark.parametrize("count", CHAIN_COUNTS)
@pytest.mark.parametrize("pset", ["mixed", "fp"])
def test_ks_chains_in_a_batch_equal_levels(devs, pset, count):
    M.case_chain_batch(devs, pset, [5] * count)


@pytest.mark.parametrize("count", CHAIN_COUNTS)
@pytest.mark.parametrize("pset", ["mixed", "fp"])
def test_ks_chains_in_a_batch_mixed_levels(devs, pset, count):
    M.case_chain_batch(devs, pset, [5, 4, 3, 5][:count])


@pytest.mark.parametrize("levels", [(0, 0), (0, 0, -1)])
def test_ks_chains_in_a_batch_at_2_16(devs, levels):
    """The only ring with k_modup_col, k_ntt_ks and the mdrs kernels; (0, 0, -1): the odd level's
    ModDown heads are refused and issue alone."""
    M.case_chain_batch_large(devs, levels)


@pytest.mark.parametrize("offset", [0, 1])
def test_stacked_region_over_four_lanes(devs, offset):
    M.case_stack_lanes(devs, offset)


def test_stacked_region_event_chain(devs):
    M.case_stack_events(devs)


def test_batch_inside_a_stacked_region_declines(devs):
    M.case_batch_inside_stack(devs)


def test_host_synchronisation_inside_a_batch(devs):
    M.case_sync_inside_batch(devs)


def test_batches_inside_a_capture(devs):
    assert M.case_batch_in_capture(devs) == 1


def test_declined_batches(devs):
    M.case_declines(devs)


_CHILD = """
import sys
sys.path[:0] = [%r, %r, %r]
import sfhe, merge_cases as M, prims_harness as H
hip, orc = sfhe.load('hip'), sfhe.load('oracle')
devs = lambda primes, logn: [H.dev(hip, 'hip', primes, logn), H.dev(orc, 'oracle', primes, logn)]
M.run_integer_path_cases(devs)
print('integer-path merged cases passed')
"""


def test_integer_path_in_a_fresh_process():
    """SFHE_NTT_FP is read once per process: a fresh child runs cases 1 to 4 with SFHE_NTT_FP=0."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, SFHE_NTT_FP="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (here, root, os.path.join(root, "sorting-fhe_amd", "python"))],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "integer-path merged cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
