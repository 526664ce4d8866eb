"""CPU, oracle only: with its stops disabled (gtol = ctol = radius_min = 0, the defaults) minimize_cases.minimize_loop -- the NumPy
restatement of csrc/dto_minimize_plan.h -- makes, on the oracle's dense operators, the decisions of the two loops the project already
holds to its bars: newton_box_cases.trust_region_loop (the README's trust-region loop, here in a box) and auglag_cases.outer_loop (the
README's outer loop).  This ties the new rules to those loops; the engine's one-call run is compared with the same oracle runs in
test_gpu_minimize.py."""
import numpy as np

import auglag_cases as A
import minimize_cases as M


def test_the_outer_loop_is_auglag_cases_outer_loop_on_the_oracles_operators():
    want, got = A.oracle_outer_run("al_12x9"), M.oracle_minimize_run("al_12x9")
    print("accepted", got["accepted"])
    print("grew", got["grew"], "max viol", got["viol0"], got["viol"])
    assert got["accepted"] == want["accepted"] and got["grew"] == want["grew"]
    assert got["viol0"] == want["viol0"] and got["viol"] == want["viol"], "one algorithm on one set of operators: the same numbers"
    # the run itself, as the oracle gives it
    assert [t + 1 for t, ok in enumerate(got["accepted"][0]) if not ok] == [1, 7], "the first outer iteration rejects trials 1 and 7"
    assert got["accepted"][2][:4] == [False] * 4 and all(got["accepted"][2][4:]), "the third rejects its first four"
    assert got["grew"] == [False, False, True, True, False]
    assert abs(got["viol0"] - 0.191) < 1e-3 and 1.7e-6 < got["viol"][-1] < 1.9e-6
    info = got["info"]
    assert info[0] == M.M_MAX_OUTER and info[1] == 5 and info[2] == 50 and info[3] == sum(sum(a) for a in got["accepted"])
    assert info[8] == got["viol0"] and info[9] == got["viol"][-1] and info[10] == 2
    assert got["history"].shape == (50, 8) and got["outer_history"].shape == (5, 4)
    assert np.array_equal(got["history"][:, 1], np.array([ok for a in got["accepted"] for ok in a], dtype=float))
    rho = got["rho"][A.case("al_12x9", dense=False)["n_dyn"]:]
    assert np.all(rho == A.RHO * 100.0), "two increases on every row"


def test_the_inner_loop_is_newton_box_cases_trust_region_loop_on_the_oracles_operators():
    run, (iterates, values, accepted), (lo, hi) = M.oracle_box_run("scaled_12x9+con", 0.3)
    print("accepted", accepted, "phi", values)
    assert run["accepted"] == [accepted]
    assert np.array_equal(run["Z"], iterates[-1]) and run["info"][5] == values[-1] and run["info"][4] == values[0]
    assert run["info"][0] == M.M_MAX_TRIALS and run["info"][2] == 10 and run["info"][3] == sum(accepted)
    assert run["merits"] == 11, "one merit per trial and the one in front"
    # delta follows the loop's rule: the history's column is what trust_region_loop would pass
    delta = 1.0
    for row in run["history"]:
        assert row[2] == delta
        if row[0] < 0.25:
            delta /= 4.0
        elif row[0] > 0.75 and row[5] != M.CONVERGED:
            delta *= 2.0
    assert run["info"][6] == delta
