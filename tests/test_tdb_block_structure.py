"""CPU: detection of replicated-block generators on TimeDependentBilinearIntegrators at dto_create (DTO_FLAG_BLOCK_GENERATORS,
the block search over every G_j and carrier matrix H_cj) on structure-only handles: what dto_integrator_blocks reports, which
integrators the structured path serves, and what is refused."""
import numpy as np
import pytest

import dto_amd
from helpers import to_engine
from tdb_block_cases import kron_family, kron_tdb_problem, problem_from_family


def blocks(po, flag=True):
    ev = dto_amd.Evaluator(to_engine(po), device=-1, block_generators=flag)
    try:
        return ev.integrator_blocks(0)
    finally:
        ev.close()


def dense_problem(n, m=1, n_mods=2):
    rng = np.random.default_rng(n)
    G = rng.standard_normal((m + 1, n, n))
    mods = [("cos", 1.7, rng.standard_normal((m + 1, n, n))), ("sin", 0.6, rng.standard_normal((m + 1, n, n)))][:n_mods]
    return problem_from_family(G, mods, m, 0, 2)


@pytest.mark.parametrize("b,r,want", [(16, 8, (16, 8, 1)), (34, 2, (34, 2, 1)), (64, 8, (64, 8, 1)), (66, 2, (66, 2, 0))])
def test_replicated_blocks_are_found_on_time_dependent_integrators(b, r, want):
    assert blocks(kron_tdb_problem(b, r, 1, 0, 2, 2)) == want


def test_dense_matrices_have_none():
    assert blocks(dense_problem(72)) == (72, 1, 0)


def test_flag_clear_reports_nothing():
    assert blocks(kron_tdb_problem(16, 8, 1, 0, 2, 2), flag=False) == (128, 1, 0)


def test_one_carrier_entry_breaks_the_structure():
    rng = np.random.default_rng(2)
    G, mods = kron_family(12, 6, 2, 2, rng)
    assert blocks(problem_from_family(G, mods, 2, 1, 2)) == (12, 6, 1)
    H = mods[1][2].copy()
    H[2, 5, 30] = 5e-324          # one off-diagonal-block entry of one carrier matrix, the smallest subnormal
    assert blocks(problem_from_family(G, [mods[0], ("sin", 0.6, H)], 2, 1, 2)) == (72, 1, 0)


def test_an_all_zero_carrier_matrix_conforms():
    rng = np.random.default_rng(3)
    G, mods = kron_family(12, 6, 1, 1, rng)
    H = mods[0][2].copy()
    H[1] = 0.0
    assert blocks(problem_from_family(G, [("cos", 1.7, H)], 1, 0, 2)) == (12, 6, 1)


def test_structure_is_that_of_the_unflagged_handle():
    p = to_engine(kron_tdb_problem(12, 6, 2, 1, 2, 2, with_derivative=True))
    evs = [dto_amd.Evaluator(p, device=-1, block_generators=f) for f in (False, True)]
    try:
        assert evs[1].integrator_blocks(0) == (12, 6, 1) and evs[1].integrator_blocks(1) == (2, 1, 0)
        assert evs[0].n_jacobian_entries == evs[1].n_jacobian_entries and evs[0].n_hessian_entries == evs[1].n_hessian_entries
        for a, b in zip(evs[0].jacobian_structure(), evs[1].jacobian_structure()):
            assert np.array_equal(a, b)
        for a, b in zip(evs[0].hessian_lagrangian_structure(), evs[1].hessian_lagrangian_structure()):
            assert np.array_equal(a, b)
    finally:
        for e in evs:
            e.close()


def test_the_cost_model_prices_the_structured_work():
    po = kron_tdb_problem(16, 8, 1, 0, 2, 2)
    p = to_engine(po)
    evs = [dto_amd.Evaluator(p, device=-1, block_generators=f) for f in (False, True)]
    try:
        dense, structured = (e.interval_costs(po.Z0).sum() for e in evs)
        assert 0.0 < structured < 0.2 * dense
    finally:
        for e in evs:
            e.close()


def test_more_than_512_states_are_refused_naming_the_limit():
    with pytest.raises(Exception, match="512 states"):
        dto_amd.Evaluator(to_engine(kron_tdb_problem(34, 16, 1, 0, 2, 0)), device=-1, block_generators=True).close()


def test_dense_272_states_on_a_flagged_handle_keep_todays_refusal():
    with pytest.raises(Exception, match="256 states"):
        dto_amd.Evaluator(to_engine(dense_problem(272, n_mods=0)), device=-1, block_generators=True).close()
