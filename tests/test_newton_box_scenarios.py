"""CPU: the scenarios of newton_box_cases.py run with the ORACLE's dense reduced Hessian and gradient alone, through the NumPy loop.  What
is asserted here are the conditions that make the GPU comparison (test_gpu_newton_box.py) meaningful, and they are met by the reference
alone: the half-box is hit and restarted, the held scenario holds exactly its four entries, the indefinite box takes a
negative-curvature step to a face and goes on, no active set hangs on a rounding, and the model value never increases."""
import numpy as np
import pytest

import newton_box_cases as B
import reduced_cases as R
from test_newton_plan_header import BOUNDARY, CONTINUE, CONVERGED, MAX_ITER, NEG_CURVATURE

CASES = ["scaled_12x9", "scaled_12x9+con", "tdb_order1"]      # of the GPU test's shapes, what a CPU run affords (reduced_cases.SMALL_CASES)
GAP = 1e-6


def run(name, scenario):
    c, sc = R.case(name), B.small_scenarios(name)
    ref = c["ref"]
    out = B.box_loop(B.oracle_product(name), np.array(ref["r_ref"]), B.nonfixed_of(c["p"]), c["Z"], **sc[scenario])
    return c, sc, out


def model_values(c, kw, out):
    """g'p + p'Ap / 2 per iteration with the oracle's dense matrix, A = Hr + shift I on the independent entries"""
    ref, Cidx = c["ref"], c["ref"]["C"]
    A = ref["Hr"] + kw["shift"] * np.eye(Cidx.size)
    g = ref["r_ref"][Cidx]
    return np.array([g @ x[Cidx] + 0.5 * x[Cidx] @ (A @ x[Cidx]) for x in out["xs"]])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("scenario", B.SCENARIOS)
def test_the_scenarios_are_what_they_are_meant_to_be(name, scenario):
    c, sc, out = run(name, scenario)
    kw, info, tr, states = sc[scenario], out["info"], out["trace"], out["states"]
    Cidx, S = c["ref"]["C"], c["ref"]["S"]
    status, it, held, hit, restarts = int(info[0]), int(info[1]), int(info[8]), int(info[9]), int(info[10])
    print(name, scenario, "status", status, "iterations", it, "held", held, "hit", hit, "restarts", restarts, "|F|", int(info[11]), "shift", kw["shift"])
    assert np.all(states[S] == B.FIXED) and np.all(out["p"][S] == 0.0)
    # no active set hangs on a rounding: where an entry was hit, the runner-up breakpoint is further by 1e-6 relative at least -- unless
    # it lies beyond the step taken and was never in question
    for (t1, t2), row in zip(out["gaps"], tr):
        if row[5] > 0:
            assert row[5] == 1 and t1 == row[4], "one entry per hit"
            assert t2 > t1 and t2 - t1 >= GAP * t1, (name, scenario, t1, t2)
    # the model value never increases (the clamps and the recurrence round: one part in 1e12 of its size is allowed)
    m = np.concatenate([[0.0], model_values(c, kw, out)])
    assert np.all(np.diff(m) <= 1e-12 * np.max(np.abs(m))), (name, scenario, m)
    lo, hi = kw.get("lo"), kw.get("hi")
    if lo is not None:
        assert np.all(out["Zp"][Cidx] >= lo[Cidx]) and np.all(out["Zp"][Cidx] <= hi[Cidx])
    if scenario == "inf":
        assert status == CONVERGED and held == hit == restarts == 0 and np.all(tr[:, 4] == np.inf) and np.all(tr[:, 0] > 0)
        err = np.linalg.norm(out["p"][Cidx] - sc["pstar"]) / np.linalg.norm(sc["pstar"])
        print(name, "||p - p*|| / ||p*||", err)
        assert err <= 1e-6
    if scenario == "half_box":
        assert status == CONVERGED and hit >= 3 and restarts >= 2 and held == 0
    if scenario == "held":
        four, two = sc["held_entries"]
        assert held == 4 and np.all((states[four] == B.HELD_LO) | (states[four] == B.HELD_HI)) and np.all(out["p"][four] == 0.0)
        assert np.all(states[two] == B.FREE) and np.all(out["p"][two] != 0.0), "on a bound with the gradient pointing inward: free, and they move"
        assert status == CONVERGED
        others = np.setdiff1d(Cidx, np.concatenate([four, two]))
        assert not np.any((states[others] == B.HELD_LO) | (states[others] == B.HELD_HI))
    if scenario == "indefinite_box":
        assert sc["lam"][0] < 0 < sc["lam"][-1], "indefinite"
        to_face = (tr[:, 0] <= 0) & (tr[:, 5] > 0) & (tr[:, 2] == tr[:, 4])
        assert np.any(to_face[:-1]) or (to_face[-1] and status in (CONVERGED, MAX_ITER)), "a negative-curvature step to a face, and the solve goes on"
        assert it > int(np.flatnonzero(to_face)[0]) + 1 or status == CONVERGED
        assert hit >= 1      # (Zp is inside the box exactly, above; p = bound - Z is rounded)
    if scenario == "indefinite_box_radius":
        assert np.sqrt(out["p"] @ out["p"]) <= 2.0 * (1 + 1e-12)
        assert status in (BOUNDARY, NEG_CURVATURE, CONVERGED, MAX_ITER)


def test_the_scenarios_differ_from_the_unbounded_step():
    c, sc, a = run("scaled_12x9", "inf")
    for scenario in ("half_box", "held"):
        b = run("scaled_12x9", scenario)[2]
        assert not np.array_equal(a["p"], b["p"]), scenario


def test_the_states_can_be_passed_back_as_the_next_mask():
    """every non-zero code is free to be decided again: the held scenario run again with its own states as the mask gives the same step"""
    c, sc, a = run("scaled_12x9", "held")
    ref = c["ref"]
    b = B.box_loop(B.oracle_product("scaled_12x9"), np.array(ref["r_ref"]), B.nonfixed_of(c["p"], free=a["states"]), c["Z"], **sc["held"])
    assert np.array_equal(a["p"], b["p"]) and np.array_equal(a["info"], b["info"])
