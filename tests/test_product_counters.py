"""What each relinearised product counts, on the CPU oracle: EvalMult(ct, ct), EvalMultMany,
EvalMultAdd, EvalMultManyAdd, EvalMultSum2, EvalMultSum and EvalMultSumMany, one op per case on
fresh counters, eager (SFHE_LAZY=0) and with deferred products (tests/product_cases.py: the
expectations are written out from the engine's counting rules).  The oracle has no fused prim, so
every op runs its composed form; its values equal the separately formed ones residue for residue.
"""
import pytest

import product_cases as P
import sfhe


@pytest.fixture(scope="module")
def sizes(oracle_lib):
    return P.key_sizes(sfhe.Engine("oracle", mult_depth=P.DEPTH, ring_dim=P.N, batch_size=8, secure=False,
                                   seed=P.SEED))


@pytest.fixture(scope="module")
def reports(oracle_lib):
    return {lazy: P.report("oracle", lazy) for lazy in (False, True)}


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("name", P.NAMES)
def test_counts_and_values(reports, sizes, name, lazy):
    P.check(reports[lazy], P.expected("oracle", lazy, *sizes), name)


def test_deferred_products_give_the_eager_values(reports):
    for name in P.NAMES:
        assert reports[True][name]["hash"] == reports[False][name]["hash"], name
