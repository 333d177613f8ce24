"""What each relinearised product counts, on the HIP engine and on the oracle
(tests/test_product_counters.py, tests/product_cases.py): the same ops, one per case on fresh
counters.  The HIP library takes the fused launch chains -- the counters say which -- and every
result equals the oracle's composed form residue for residue; with each op's knob off it composes
on the device as well (the report's `ref`).
"""
import pytest

import product_cases as P
import sfhe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sizes(hip_lib):
    return P.key_sizes(sfhe.Engine("hip", mult_depth=P.DEPTH, ring_dim=P.N, batch_size=8, secure=False, seed=P.SEED))


@pytest.fixture(scope="module")
def reports(hip_lib, oracle_lib):
    return {(b, lazy): P.report(b, lazy) for b in ("hip", "oracle") for lazy in (False, True)}


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("name", P.NAMES)
def test_counts_and_values(reports, sizes, name, lazy):
    got = {b: P.check(reports[(b, lazy)], P.expected(b, lazy, *sizes), name) for b in ("hip", "oracle")}
    assert got["hip"] == got["oracle"], name
