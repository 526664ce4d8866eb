"""CPU: detection of replicated-block generators G_j = I_r (x) B_j at dto_create (DTO_FLAG_BLOCK_GENERATORS) on structure-only
handles, and what dto_integrator_blocks reports."""
import numpy as np

import dto_amd
import dto_oracle as O
from helpers import to_engine


def problem(G, m, N=4, x_dim=None):
    n = G.shape[1]
    z = n + 2 * m + 1
    rng = np.random.default_rng(1)
    Z0 = rng.standard_normal(z * N)
    return O.Problem(N=N, z=z, dt_idx=z - 1,
                     integrators=[O.BilinearIntegrator(0, n, n, m, G), O.DerivativeIntegrator(n, m, n + m)],
                     objectives=[O.QuadraticRegularizer(n, m, np.ones(m))], Z0=Z0)


def blocks(G, m, flag=True):
    ev = dto_amd.Evaluator(to_engine(problem(G, m)), device=-1, block_generators=flag)
    try:
        return ev.integrator_blocks(0), ev
    finally:
        ev.close()


def kron_generators(b, r, m, seed=0, inner=1):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((m + 1, b, b))
    return np.stack([np.kron(np.eye(r), np.kron(np.eye(inner), Bj)) for Bj in B])


def test_replicated_blocks_are_found():
    assert blocks(kron_generators(16, 8, 2), 2)[0] == (16, 8, 1)


def test_the_finest_structure_is_reported():
    assert blocks(kron_generators(8, 4, 2, inner=2), 2)[0] == (8, 8, 1)


def test_dense_generators_have_none():
    G = np.random.default_rng(3).standard_normal((3, 48, 48))
    assert blocks(G, 2)[0] == (48, 1, 0)


def test_comparison_is_exact():
    G = kron_generators(16, 4, 2)
    G1 = G.copy(); G1[1, 3, 40] = 5e-324                      # one off-block entry, the smallest subnormal
    assert blocks(G1, 2)[0] == (64, 1, 0)
    G2 = G.copy(); G2[2, 16 + 5, 16 + 7] = np.nextafter(G2[2, 16 + 5, 16 + 7], np.inf)   # one diagonal block, last bit
    assert blocks(G2, 2)[0] == (64, 1, 0)
    G3 = G.copy(); G3[G3 == 0.0] = -0.0                       # -0.0 == 0.0
    assert blocks(G3, 2)[0] == (16, 4, 1)


def test_every_generator_must_share_the_structure():
    G = kron_generators(16, 4, 2)
    G[2] = np.random.default_rng(5).standard_normal((64, 64))   # drift structured, one drive dense
    assert blocks(G, 2)[0] == (64, 1, 0)


def test_blocks_above_64_keep_the_dense_path():
    assert blocks(kron_generators(96, 2, 1), 1)[0] == (96, 2, 0)


def test_the_small_state_range_keeps_its_kernel():
    assert blocks(kron_generators(16, 2, 2), 2)[0] == (16, 2, 0)   # x_dim = 32


def test_flag_clear_reports_nothing_and_structure_is_the_same():
    G = kron_generators(16, 8, 2)
    assert blocks(G, 2, flag=False)[0] == (128, 1, 0)
    evs = [dto_amd.Evaluator(to_engine(problem(G, 2)), device=-1, block_generators=f) for f in (False, True)]
    try:
        assert evs[0].n_jacobian_entries == evs[1].n_jacobian_entries and evs[0].n_hessian_entries == evs[1].n_hessian_entries
        for a, b in zip(evs[0].jacobian_structure(), evs[1].jacobian_structure()):
            assert np.array_equal(a, b)
        for a, b in zip(evs[0].hessian_lagrangian_structure(), evs[1].hessian_lagrangian_structure()):
            assert np.array_equal(a, b)
        # other integrator kinds report (x_dim, 1, 0)
        assert evs[1].integrator_blocks(1) == (2, 1, 0)
    finally:
        for e in evs:
            e.close()


def test_unitary_problem_is_recognised():
    prob = dto_amd.synthetic.unitary_problem(levels=8, drives=2, N=5)
    ev = dto_amd.Evaluator(prob, device=-1, block_generators=True)
    try:
        assert ev.integrator_blocks(0) == (16, 8, 1)
        # the cost model prices the structured work: far below the dense path's
        Z = prob.trajectory.vec()
        dense = dto_amd.Evaluator(prob, device=-1)
        try:
            assert 0.0 < ev.interval_costs(Z).sum() < 0.2 * dense.interval_costs(Z).sum()
        finally:
            dense.close()
    finally:
        ev.close()
