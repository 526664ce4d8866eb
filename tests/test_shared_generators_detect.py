"""CPU: grouping of bilinear integrators with equal generators and controls at dto_create (DTO_FLAG_SHARED_GENERATORS) on
structure-only handles, and what dto_integrator_share reports."""
import numpy as np

import dto_amd
import dto_oracle as O
from dto_amd import capi
from helpers import to_engine


def problem(Gs, n, m=2, N=4, u_offs=None, dims=None, tdb_last=False):
    """kets x_1 .. x_P (dims[i] states each, default n), then u[m], v[m] (a second control component), du[m], dt; integrator i has
    generators Gs[i] and reads the controls at u_offs[i] (default: u)."""
    P = len(Gs)
    dims = [n] * P if dims is None else dims
    x_offs = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    u0 = int(x_offs[-1])
    z = u0 + 3 * m + 2
    u_offs = [u0] * P if u_offs is None else u_offs
    integ = [O.BilinearIntegrator(int(x_offs[i]), dims[i], u_offs[i], m, Gs[i]) for i in range(P)]
    integ.append(O.DerivativeIntegrator(u0, m, u0 + 2 * m))
    if tdb_last:  # a time-dependent integrator with the first ket's generators, on the first ket's state and a time component
        integ.append(O.TimeDependentBilinearIntegrator(0, dims[0], u0, m, z - 2, Gs[0], [], spline_order=0, substeps=4))
    Z0 = np.random.default_rng(1).standard_normal(z * N)
    return O.Problem(N=N, z=z, dt_idx=z - 1, integrators=integ, objectives=[O.QuadraticRegularizer(u0, m, np.ones(m))], Z0=Z0), u0


def gens(n, m=2, seed=0):
    return np.random.default_rng(seed).standard_normal((m + 1, n, n))


def shares(prob, flag=True, **kw):
    ev = dto_amd.Evaluator(to_engine(prob), device=-1, shared_generators=flag, **kw)
    try:
        return [ev.integrator_share(i) for i in range(len(prob.integrators))]
    finally:
        ev.close()


def test_abi_version_and_flag_value():
    assert capi.DTO_ABI_VERSION == 8 and capi.FLAG_SHARED_GENERATORS == 4
    header = open(__file__.replace("tests/test_shared_generators_detect.py", "include/dto_engine.h")).read()
    assert "#define DTO_ABI_VERSION 8" in header and "#define DTO_FLAG_SHARED_GENERATORS 4" in header


def test_three_equal_integrators_form_one_group():
    G = gens(48)
    p, _ = problem([G, G.copy(), G.copy()], 48)
    assert shares(p) == [(0, 3, 1), (0, 3, 1), (0, 3, 1), (3, 1, 0)]


def test_flag_clear_reports_nothing():
    G = gens(48)
    p, _ = problem([G, G, G], 48)
    assert shares(p, flag=False) == [(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0)]


def test_comparison_is_exact():
    G = gens(48)
    G1 = G.copy(); G1[2, 17, 5] = np.nextafter(G1[2, 17, 5], np.inf)     # one entry of one drive, last bit
    p, _ = problem([G, G1], 48)
    assert shares(p)[:2] == [(0, 1, 0), (1, 1, 0)]
    G2 = G.copy(); G2[0, 3, 3] = 0.0
    G3 = G2.copy(); G3[0, 3, 3] = -0.0                                    # -0.0 == 0.0
    p, _ = problem([G2, G3], 48)
    assert shares(p)[:2] == [(0, 2, 1), (0, 2, 1)]


def test_a_different_control_component_is_not_grouped():
    G = gens(48)
    p, u0 = problem([G, G, G], 48)
    p2, _ = problem([G, G, G], 48, u_offs=[u0, u0 + 2, u0])
    assert shares(p2)[:3] == [(0, 2, 1), (1, 1, 0), (0, 2, 1)]


def test_a_different_x_dim_is_not_grouped():
    G = gens(48)
    p, _ = problem([G, G[:, :40, :40].copy()], 48, dims=[48, 40])
    assert shares(p)[:2] == [(0, 1, 0), (1, 1, 0)]


def test_two_pairs_give_two_groups():
    A, B = gens(48, seed=1), gens(48, seed=2)
    p, _ = problem([A, B, A, B], 48)
    assert shares(p)[:4] == [(0, 2, 1), (1, 2, 1), (0, 2, 1), (1, 2, 1)]


def test_small_states_are_grouped_but_inactive():
    G = gens(16)
    p, _ = problem([G, G], 16)
    assert shares(p)[:2] == [(0, 2, 0), (0, 2, 0)]
    # ... unless the general path serves them
    assert shares(p, general_path_only=True)[:2] == [(0, 2, 1), (0, 2, 1)]


def test_structured_integrators_are_grouped_but_inactive():
    B = np.random.default_rng(4).standard_normal((3, 16, 16))
    G = np.stack([np.kron(np.eye(4), Bj) for Bj in B])
    p, _ = problem([G, G], 64)
    assert shares(p, block_generators=True)[:2] == [(0, 2, 0), (0, 2, 0)]
    assert shares(p)[:2] == [(0, 2, 1), (0, 2, 1)]


def test_a_time_dependent_integrator_is_never_grouped():
    G = gens(8)
    p, _ = problem([G, G], 8, tdb_last=True)
    s = shares(p, general_path_only=True)
    assert s == [(0, 2, 1), (0, 2, 1), (2, 1, 0), (3, 1, 0)]


def test_structures_do_not_depend_on_the_flag():
    G = gens(48)
    p, _ = problem([G, G, G], 48)
    evs = [dto_amd.Evaluator(to_engine(p), device=-1, shared_generators=f) for f in (False, True)]
    try:
        assert evs[0].n_jacobian_entries == evs[1].n_jacobian_entries and evs[0].n_hessian_entries == evs[1].n_hessian_entries
        for a, b in zip(evs[0].jacobian_structure(), evs[1].jacobian_structure()):
            assert np.array_equal(a, b)
        for a, b in zip(evs[0].hessian_lagrangian_structure(), evs[1].hessian_lagrangian_structure()):
            assert np.array_equal(a, b)
    finally:
        for e in evs:
            e.close()


def test_a_follower_costs_its_sweep_not_a_chain():
    prob = dto_amd.synthetic.multi_ket_problem(64, 3, 2, 6)
    Z = prob.trajectory.vec()
    evs = [dto_amd.Evaluator(prob, device=-1, shared_generators=f) for f in (False, True)]
    one = dto_amd.Evaluator(dto_amd.synthetic.multi_ket_problem(64, 1, 2, 6), device=-1)
    try:
        assert [evs[1].integrator_share(i) for i in range(4)] == [(0, 3, 1), (0, 3, 1), (0, 3, 1), (3, 1, 0)]
        plain, shared, single = (e.interval_costs(Z if e is not one else one.trajectory.vec()).sum() for e in (evs[0], evs[1], one))
        assert single < shared < plain and shared < 0.75 * plain
    finally:
        for e in evs + [one]:
            e.close()
