"""The merged-launch cases (tests/merge_cases.py) on the C oracle alone.

The oracle's sfp_batch_begin returns 0 and its stacked-region, lane, event and graph calls
are no-ops, so the same call sequences run unmerged: this module checks the cases' call
sequences, strides and exact references without a GPU, keeps the oracle's no-op contract
under test (every region call accepted, the ops run as issued, the stats at zero), and
checks the restatement of stackFlush's grouping rule (merge_cases.flush_model) on shapes
whose grouping is worked out by hand.  The same cases run on the HIP library, stats included, in
test_gpu_merged_launches.py.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_cases as M  # noqa: E402
import prims_harness as H  # noqa: E402

EW_COUNTS = [2, 3, 4, 5, 8]
CHAIN_COUNTS = [2, 3, 4]


@pytest.fixture(scope="module")
def devs(oracle_lib):
    return lambda primes, logn: [H.dev(oracle_lib, "oracle", primes, logn)]


def test_flush_model_on_the_hand_derived_groupings():
    """stackFlush's rule by hand: element-wise sets merge four at most (5 = 4 + 1, 8 = 4 + 4);
    row-set kernels up to eight; unclassified launches never; forward and inverse transforms
    never with each other; a lane that waits issues after the record it names."""
    y = [M.L("Y", "add")]
    assert [M.flush_model([y] * c)[:2] for c in EW_COUNTS] == [(1, 0), (1, 0), (1, 0), (1, 1), (2, 0)]
    assert M.flush_model([[M.L(None, "tensor")]] * 5)[:2] == (0, 5)
    assert [M.flush_model([M.t_ntt(9, 0)] * c)[:2] for c in range(2, 9)] == [(2, 0)] * 7
    m, s, g = M.flush_model([M.t_ntt(9, 0), M.t_ntt(9, 1), M.t_ntt(9, 0), M.t_ntt(9, 1)])
    assert (m, s) == (4, 0) and [x[2] for x in g] == [(0, 2), (0, 2), (1, 3), (1, 3)]
    assert M.flush_model([M.t_ntt(72, 0), M.t_ntt(9, 0), M.t_ntt(9, 0)])[:2] == (2, 2)
    # the waiter has more items left, and still goes second
    m, s, g = M.flush_model([[M.L("Y", "a"), ("R", 1)], [("W", 1), M.L("Y", "b"), M.L("Y", "b"), M.L("Y", "b")]])
    assert (m, s) == (0, 4) and [x[2] for x in g] == [(0,), (1,), (1,), (1,)]
    # lanes offset by one op: the three leading adds go first, then four aligned lanes
    seq = M.t_ntt(9, 0) + [M.L("Y", "mul")] + M.t_ntt(9, 1)
    assert M.flush_model([seq] + [[M.L("Y", "add")] + seq] * 3)[:2] == (6, 0)
    # one lane behind by one op and no group: the lane with the most items left goes first
    m, s, g = M.flush_model([[M.L("Y", "mul")], [M.L("Y", "add"), M.L("Y", "mul")]])
    assert (m, s) == (1, 1) and [x[2] for x in g] == [(1,), (0, 1)]
    # ModDown heads of one key: levels 4, 4, 3 -- three refused, the first two merge; levels
    # 4, 3, 4 -- a refused group loses its last lane only, so the two of level 4 never meet
    md = lambda l: [M.L("MDRS", "m", l)]
    assert [x[2] for x in M.flush_model([md(4), md(4), md(3)])[2]] == [(0, 1), (2,)]
    assert M.flush_model([md(4), md(3), md(4)])[:2] == (0, 3)


@pytest.mark.parametrize("count", EW_COUNTS)
@pytest.mark.parametrize("prim", M.EW_PRIMS)
def test_elementwise_family_in_a_batch(devs, prim, count):
    M.case_ew_batch(devs, (prim,), count)


def test_two_prims_in_one_batch(devs):
    M.case_ew_batch(devs, ("add", "mul"), 4)


@pytest.mark.parametrize("count", [2, 3, 4, 5, 6, 7, 8])
def test_ntt_batch_equal_maps(devs, count):
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


def test_capture_is_declined_by_the_oracle(devs):
    """The oracle has no graphs: sfp_capture_begin returns -1 and the case runs nothing on it."""
    assert M.case_batch_in_capture(devs) == 0


def test_declined_batches(devs):
    M.case_declines(devs)
