"""CPU: grouping of TimeDependentBilinearIntegrators of one system at dto_create (DTO_FLAG_SHARED_GENERATORS on the time-dependent
kind) on structure-only handles: what dto_integrator_share reports, that structure does not depend on the flag, and how
dto_interval_costs prices a group."""
import numpy as np
import pytest

import dto_amd
import tdb_share_cases as S
from helpers import to_engine


def shares(prob, flag=True, **kw):
    ev = dto_amd.Evaluator(to_engine(prob), device=-1, shared_generators=flag, **kw)
    try:
        return [ev.integrator_share(i) for i in range(len(prob.integrators))]
    finally:
        ev.close()


def test_three_equal_families_form_one_active_group():
    p = S.problem(72, 3)
    assert shares(p) == [(0, 3, 1), (0, 3, 1), (0, 3, 1), (3, 1, 0)]
    assert shares(p, flag=False) == [(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0)]
    p = S.problem(72, 3, derivative_between=True)
    assert shares(p) == [(0, 3, 1), (1, 1, 0), (0, 3, 1), (0, 3, 1)]


def _differs(what):
    G, mods = S.family(72, 2, 2, seed=100 + 72)
    if what == "H last bit":
        H = mods[1][2].copy(); H[2, 17, 5] = np.nextafter(H[2, 17, 5], np.inf)
        return {"mods": [mods[0], (mods[1][0], mods[1][1], H)]}
    if what == "G last bit":
        G1 = G.copy(); G1[0, 3, 70] = np.nextafter(G1[0, 3, 70], -np.inf)
        return {"G": G1}
    if what == "omega":
        return {"mods": [(mods[0][0], np.nextafter(mods[0][1], 2.0), mods[0][2]), mods[1]]}
    if what == "modulation kind":
        return {"mods": [("sin", mods[0][1], mods[0][2]), mods[1]]}
    return {"substeps": {"substeps": 3}, "order": {"order": 0}, "control component": {"u": 1}, "time component": {"t": 1},
            "x_dim": {"dim": 70}}[what]


@pytest.mark.parametrize("what", ["H last bit", "G last bit", "omega", "modulation kind", "substeps", "order", "control component",
                                  "time component", "x_dim"])
def test_one_difference_keeps_an_integrator_out_of_the_group(what):
    p = S.problem(72, 3, members=[{}, _differs(what), {}])
    assert shares(p)[:3] == [(0, 2, 1), (1, 1, 0), (0, 2, 1)], what


def test_minus_zero_equals_zero():
    G, mods = S.family(72, 2, 2, seed=100 + 72)
    G2 = G.copy(); G2[1, 4, 4] = 0.0
    G3 = G2.copy(); G3[1, 4, 4] = -0.0
    assert shares(S.problem(72, 2, members=[{"G": G2}, {"G": G3}]))[:2] == [(0, 2, 1), (0, 2, 1)]


def test_two_pairs_give_two_groups():
    B = {"G": S.family(72, 2, 2, seed=5)[0]}
    p = S.problem(72, 4, members=[{}, B, {}, B])
    assert shares(p)[:4] == [(0, 2, 1), (1, 2, 1), (0, 2, 1), (1, 2, 1)]


def test_24_state_members_are_grouped_but_inactive():
    assert shares(S.problem(24, 2))[:2] == [(0, 2, 0), (0, 2, 0)]
    assert shares(S.problem(64, 2))[:2] == [(0, 2, 0), (0, 2, 0)]     # k_tdb's last size
    assert shares(S.problem(65, 2))[:2] == [(0, 2, 1), (0, 2, 1)]     # k_tdb_mfma's first


def test_structured_members_are_grouped_but_inactive():
    rng = np.random.default_rng(4)
    kron = lambda B: np.stack([np.kron(np.eye(6), Bj) for Bj in B])
    fam = {"G": kron(rng.standard_normal((3, 12, 12))), "mods": [("cos", 1.7, kron(rng.standard_normal((3, 12, 12))))]}
    p = S.problem(72, 2, members=[fam, fam])
    assert shares(p, block_generators=True)[:2] == [(0, 2, 0), (0, 2, 0)]
    assert shares(p)[:2] == [(0, 2, 1), (0, 2, 1)]


def test_a_bilinear_and_a_time_dependent_integrator_with_equal_G_are_not_grouped():
    p = S.problem(72, 1, n_mods=0, order=0, bilinear_first=True)
    assert shares(p) == [(0, 1, 0), (1, 1, 0), (2, 1, 0)]
    p = S.problem(72, 2, n_mods=0, order=0, bilinear_first=True)
    assert shares(p) == [(0, 1, 0), (1, 2, 1), (1, 2, 1), (3, 1, 0)]


def test_structures_do_not_depend_on_the_flag():
    p = to_engine(S.problem(72, 3, derivative_between=True))
    evs = [dto_amd.Evaluator(p, device=-1, shared_generators=f) for f in (False, True)]
    try:
        assert evs[0].n_jacobian_entries == evs[1].n_jacobian_entries and evs[0].n_hessian_entries == evs[1].n_hessian_entries
        for a, b in zip(evs[0].jacobian_structure(), evs[1].jacobian_structure()):
            assert np.array_equal(a, b)
        for a, b in zip(evs[0].hessian_lagrangian_structure(), evs[1].hessian_lagrangian_structure()):
            assert np.array_equal(a, b)
    finally:
        for e in evs:
            e.close()


def test_a_group_is_priced_by_its_one_launch():
    """single < shared < plain for three kets at 72 states; one launch per member (tdb_share_members = 1) costs what the unflagged
    handle does."""
    p3, p1 = S.problem(72, 3), S.problem(72, 1)
    evs = [dto_amd.Evaluator(to_engine(p3), device=-1, shared_generators=f) for f in (False, True)]
    one = dto_amd.Evaluator(to_engine(p1), device=-1)
    try:
        plain, shared, single = evs[0].interval_costs(p3.Z0).sum(), evs[1].interval_costs(p3.Z0).sum(), one.interval_costs(p1.Z0).sum()
        assert single < shared < plain, (single, shared, plain)
        evs[1].set_option("tdb_share_members", 1)
        assert evs[1].interval_costs(p3.Z0).sum() == plain
        evs[1].set_option("tdb_share_members", 3)
        assert evs[1].interval_costs(p3.Z0).sum() == shared
        for bad in (0, 4):
            with pytest.raises(Exception, match="tdb_share_members"):
                evs[1].set_option("tdb_share_members", bad)
    finally:
        for e in evs + [one]:
            e.close()


def test_synthetic_multi_ket_modulated_problem_is_grouped():
    prob = dto_amd.synthetic.multi_ket_modulated_problem(72, 3, 2, 4, substeps=2)
    ev = dto_amd.Evaluator(prob, device=-1, shared_generators=True)
    try:
        assert [ev.integrator_share(i) for i in range(4)] == [(0, 3, 1), (0, 3, 1), (0, 3, 1), (3, 1, 0)]
    finally:
        ev.close()
    prob = dto_amd.synthetic.multi_ket_modulated_problem(72, 2, 1, 4, order=0, n_mods=1, derivative_between=True)
    ev = dto_amd.Evaluator(prob, device=-1, shared_generators=True)
    try:
        assert [ev.integrator_share(i) for i in range(3)] == [(0, 2, 1), (1, 1, 0), (0, 2, 1)]
    finally:
        ev.close()
