"""GPU: the contract the four KEPT POINTS of the host driver share (csrc/dto_kept_point.h; DESIGN, "Kept points"), stated once through
the public Evaluator and the profile counters alone, on ONE handle of the case scaled_12x9+con (reduced_cases.py: 12 states, two
integrators, a constraint so that mu matters -- the smallest case on which all four points exist).

    operator                                    its point                      rebuilt                 at the kept point
    dynamics_solve (integrator 0)               integrator, Z                  dynsolve_tree > 0       dynsolve_tree == 0
    dynamics_solve_all                          Z                              dynsolve_tree > 0       dynsolve_tree == 0
    eval_hessian_lagrangian_product (H v)       Z, sigma, mu                   hess_product == 2       hess_product == 1
    reduced_hessian_product                     Z, sigma, mu or "no mu"        reduced_pack > 6        reduced_pack == 6
    reduced_lagrangian_gradient                 (the reduced point)            all > 0                 all == 0

Every point also holds the handle's generation: dto_set_option and every failed call start all of them anew.  The reduced product runs
a whole-dynamics solve at its Z and an H v at its own multipliers, so it moves those two points; each test below primes what it reads
in an order that allows for that."""
import numpy as np
import pytest

import dto_amd
import reduced_cases as R

pytestmark = pytest.mark.gpu

CASE = "scaled_12x9+con"


@pytest.fixture(scope="module")
def ev():
    c = R.case(CASE)
    e = dto_amd.Evaluator(c["pe"], **c["kw"])
    e.profile_enable(True)
    yield e
    e.close()


class Operator:
    def __init__(self, name, call, counter, rebuilt, hit):
        self.name, self.call, self.counter, self.rebuilt, self.hit = name, call, counter, rebuilt, hit


def operators(ev):
    c = R.case(CASE)
    p, v = c["p"], c["vs"][0]
    D = sum(it.x_dim for it in p.integrators)
    rng = np.random.default_rng(8)
    B1, BD = rng.standard_normal((p.N, 1, p.integrators[0].x_dim)), rng.standard_normal((p.N, 1, D))

    def hv(Z, sigma, mu):
        y = np.full(ev.n_variables, np.nan)
        ev.eval_hessian_lagrangian_product(y, Z, v, sigma, mu)
        return y

    ops = [Operator("dynamics_solve", lambda Z, sigma, mu: ev.dynamics_solve(Z, B1, integrator=0), "dynsolve_tree", lambda n: n > 0, lambda n: n == 0),
           Operator("dynamics_solve_all", lambda Z, sigma, mu: ev.dynamics_solve_all(Z, BD), "dynsolve_tree", lambda n: n > 0, lambda n: n == 0),
           Operator("hessian_product", hv, "hess_product", lambda n: n == 2, lambda n: n == 1),
           Operator("reduced_hessian_product", lambda Z, sigma, mu: ev.reduced_hessian_product(Z, v, sigma, mu), "reduced_pack",
                    lambda n: n > 6, lambda n: n == 6)]
    return {o.name: o for o in ops}


OPERATORS = ["dynamics_solve", "dynamics_solve_all", "hessian_product", "reduced_hessian_product"]


def measure(ev, op, Z, sigma, mu):
    """the operator's counter over one call, and the call's result"""
    ev.profile_reset()
    out = op.call(Z, sigma, mu)
    n = ev.profile_get(op.counter)[1]
    print(op.name, op.counter, n)
    assert not np.isnan(out).any()
    return n, out


def gradient_launches(ev, Z, sigma, mu):
    ev.profile_reset()
    r = ev.reduced_lagrangian_gradient(Z, sigma, mu)
    n = ev.profile_get("all")[1]
    print("reduced_lagrangian_gradient all", n)
    return n, r


def one_ulp_in_a_timestep(Z):
    p = R.case(CASE)["p"]
    Zt = np.array(Z)
    i = 2 * p.z + p.dt_idx
    Zt[i] = np.nextafter(Zt[i], np.inf)
    return Zt


def refused_call(ev, Z):
    with pytest.raises(dto_amd.EngineError, match="n_cols = 0"):
        ev.rollout(Z, X0=np.empty((0, R.case(CASE)["p"].integrators[0].x_dim)))


@pytest.mark.parametrize("name", OPERATORS)
def test_the_shared_contract(ev, name):
    c, op = R.case(CASE), operators(ev)[name]
    Z, mu = c["Z"], c["mu"]
    _, first = measure(ev, op, Z, R.SIGMA, mu)                      # (whatever the tests before left: this call makes the point)
    # 1. a second call at the same point hits, with the same bits
    n, again = measure(ev, op, Z, R.SIGMA, mu)
    assert op.hit(n) and np.array_equal(again, first)
    # 2. one ulp in a timestep is another point
    Zt = one_ulp_in_a_timestep(Z)
    n, _ = measure(ev, op, Zt, R.SIGMA, mu)
    assert op.rebuilt(n)
    n, _ = measure(ev, op, Zt, R.SIGMA, mu)
    assert op.hit(n), "the new point is the kept one now"
    n, back = measure(ev, op, Z, R.SIGMA, mu)
    assert op.rebuilt(n) and np.array_equal(back, first)
    # 3. dto_set_option starts every point anew; the rebuilt result has the bits of the kept one
    for value in (0, 1):
        ev.set_option("overlap_sweep", value)
        n, out = measure(ev, op, Z, R.SIGMA, mu)
        assert op.rebuilt(n) and np.array_equal(out, first), value
        n, out = measure(ev, op, Z, R.SIGMA, mu)
        assert op.hit(n) and np.array_equal(out, first), value
    # 4. so does a call refused with text on its arguments, and the handle stays usable
    refused_call(ev, Z)
    n, out = measure(ev, op, Z, R.SIGMA, mu)
    assert op.rebuilt(n) and np.array_equal(out, first)
    n, out = measure(ev, op, Z, R.SIGMA, mu)
    assert op.hit(n) and np.array_equal(out, first)


def prime_all(ev, ops, Z, sigma, mu):
    """every point made (Z, sigma, mu): the reduced product before H v, whose point it moves to its own multipliers"""
    for name in ("dynamics_solve", "dynamics_solve_all", "reduced_hessian_product", "hessian_product"):
        measure(ev, ops[name], Z, sigma, mu)


def test_a_rollout_takes_the_single_integrator_solves_tree_alone(ev):
    c, ops = R.case(CASE), operators(ev)
    Z, mu = c["Z"], c["mu"]
    prime_all(ev, ops, Z, R.SIGMA, mu)
    ev.rollout(Z)
    n, _ = measure(ev, ops["dynamics_solve"], Z, R.SIGMA, mu)
    assert ops["dynamics_solve"].rebuilt(n)
    for name in ("dynamics_solve_all", "hessian_product", "reduced_hessian_product"):    # H v before the reduced product moves its point
        n, _ = measure(ev, ops[name], Z, R.SIGMA, mu)
        assert ops[name].hit(n), name
    n, _ = gradient_launches(ev, Z, R.SIGMA, mu)
    assert n == 0, "a reduced gradient at the kept point copies its result"


def test_sigma_and_mu_are_part_of_the_products_points(ev):
    c, ops = R.case(CASE), operators(ev)
    Z, mu = c["Z"], c["mu"]
    sigma2 = np.nextafter(R.SIGMA, 1.0)
    mu2 = np.array(mu)
    mu2[-1] = np.nextafter(mu2[-1], np.inf)                          # the last row: a non-dynamics one
    assert c["n_cons"] > c["n_dyn"] and mu2[-1] != mu[-1]
    for name in ("hessian_product", "reduced_hessian_product"):
        op = ops[name]
        measure(ev, op, Z, R.SIGMA, mu)
        for what, (s, m) in dict(sigma=(sigma2, mu), mu=(R.SIGMA, mu2)).items():
            n, _ = measure(ev, op, Z, s, m)
            assert op.rebuilt(n), (name, what)
            n, _ = measure(ev, op, Z, s, m)
            assert op.hit(n), (name, what)
            n, _ = measure(ev, op, Z, R.SIGMA, mu)
            assert op.rebuilt(n), (name, what, "and back")
    # the reduced gradient: mu given against mu absent
    gradient_launches(ev, Z, R.SIGMA, mu)
    n, with_mu = gradient_launches(ev, Z, R.SIGMA, mu)
    assert n == 0
    n, without = gradient_launches(ev, Z, R.SIGMA, None)
    assert n > 0
    n, again = gradient_launches(ev, Z, R.SIGMA, None)
    assert n == 0 and np.array_equal(again, without)
    n, back = gradient_launches(ev, Z, R.SIGMA, mu)
    assert n > 0 and np.array_equal(back, with_mu)


def test_a_whole_dynamics_solve_elsewhere_leaves_the_reduced_and_the_hessian_points(ev):
    c, ops = R.case(CASE), operators(ev)
    Z, mu = c["Z"], c["mu"]
    prime_all(ev, ops, Z, R.SIGMA, mu)
    solve = ops["dynamics_solve_all"]
    n, _ = measure(ev, solve, one_ulp_in_a_timestep(Z), R.SIGMA, mu)
    assert solve.rebuilt(n)
    n, _ = measure(ev, ops["hessian_product"], Z, R.SIGMA, mu)
    assert ops["hessian_product"].hit(n)
    n, _ = gradient_launches(ev, Z, R.SIGMA, mu)
    assert n == 0, "the reduced point is its own"
    n, _ = measure(ev, solve, Z, R.SIGMA, mu)
    assert solve.rebuilt(n), "the solves' point went to the other Z"
    n, _ = measure(ev, solve, Z, R.SIGMA, mu)
    assert solve.hit(n), "one rebuild"
    ev.profile_reset()
    ops["reduced_hessian_product"].call(Z, R.SIGMA, mu)
    assert ev.profile_get("reduced_pack")[1] == 6 and ev.profile_get("dynsolve_tree")[1] == 0
