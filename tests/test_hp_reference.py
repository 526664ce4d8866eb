"""CPU: the 320-bit reference (tests/hp_reference.py) is pinned, the accuracy-budget fixtures (tests/golden/hp_*.npz) come out of
their generator, and the fp64 oracle sits within 1e-13 of every fixture in the normwise metric per interval and quantity class
(tests/hp_cases.py).  The oracle's Hessian error is printed per interval; DESIGN section 2 records it."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import hp_cases as C
import hp_reference as HP


def _mp_err(E, ref, mp):
    n = E.shape[0]
    return max(abs(mp.mpf(int(E[i, j])) / mp.mpf(HP.ONE) - ref[i, j]) for i in range(n) for j in range(n))


@pytest.mark.parametrize("kind", ["skew", "non_normal"])
def test_exponential_agrees_with_mpmath_at_50_digits(kind):
    import mpmath as mp
    rng = np.random.default_rng(6)
    M = 3.0 * rng.standard_normal((6, 6))
    if kind == "skew":
        M = M - M.T
    with mp.workdps(50):
        ref = mp.expm(mp.matrix(M.tolist()), method="taylor")
        assert _mp_err(HP.expm(HP.fx(M)), ref, mp) <= mp.mpf("1e-40")
        # the action, summed with no scaling, gives the same vector
        v = rng.standard_normal(6)
        got = HP.expm_action(HP.fx(M), HP.fx(v))
        want = ref * mp.matrix(v.tolist())
        assert max(abs(mp.mpf(int(got[i])) / mp.mpf(HP.ONE) - want[i]) for i in range(6)) <= mp.mpf("1e-40")


@pytest.mark.parametrize("kind", ["skew", "non_normal"])
def test_block_form_frechet_derivative_is_the_central_difference_of_exp(kind):
    rng = np.random.default_rng(7)
    A, B = 2.0 * rng.standard_normal((6, 6)), rng.standard_normal((6, 6))
    if kind == "skew":
        A, B = A - A.T, B - B.T
    x = rng.standard_normal(6)
    Af, Bf, xf = HP.fx(A), HP.fx(B), HP.fx(x)
    L, Ex = HP.frechet_action(Af, Bf, xf)
    h = 80
    Bh = (Bf + 0) >> h   # 2^-80 B, exact but for the floor at 2^-320
    diff = (HP.mul(HP.expm(Af + Bh), xf) - HP.mul(HP.expm(Af - Bh), xf)) << (h - 1)
    # truncation ~ 2^-160 ||B||^3, the shift amplifies 2^-320 roundings to 2^-240: 1e-40 holds with room
    assert max(abs(int(v)) for v in (L.reshape(-1) - diff)) / HP.ONE <= 1e-40
    assert max(abs(int(v)) for v in (Ex.reshape(-1) - HP.mul(HP.expm(Af), xf))) / HP.ONE <= 1e-80


def test_differenced_hessian_is_symmetric_and_matches_the_gradient_in_x():
    """The (u_i, u_j) entries come out of two independent differencings; the (x, u) entries, differenced along u from the x
    gradient, equal the x gradient of the u column (the defect is linear in x): d/dx [-mu' L_j x] = -L_j' mu."""
    rng = np.random.default_rng(8)
    n, m = 5, 2
    G = rng.standard_normal((m + 1, n, n))
    G = G - G.transpose(0, 2, 1)
    x, xn, mu, u = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(m)
    R = HP.interval(G, x, u, 0.7, xn, mu=mu)
    H = R["H"]
    assert all(int(H[i, j]) == int(H[j, i]) for i in range(n + m + 1) for j in range(n + m + 1))
    assert all(int(H[i, j]) == 0 for i in range(n) for j in range(n))
    for j in range(m):   # -L_j' mu through the transposed block form
        LT, _ = HP.frechet_action(R["A"].T.copy(), HP.scale(int(HP.fx(0.7)), HP.fx(G[1 + j])).T.copy(), HP.fx(mu))
        assert max(abs(int(a) + int(b)) for a, b in zip(H[:n, n + j], LT.reshape(-1))) / HP.ONE <= 1e-40


def _generator():
    spec = importlib.util.spec_from_file_location("make_hp_golden", os.path.join(C.GOLDEN, "make_hp_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_fixture_regenerates_bit_for_bit():
    fresh, stored = _generator().build("hp_small"), C.load("hp_small")
    assert sorted(fresh) == sorted(stored)
    for k in stored:
        assert np.array_equal(np.asarray(fresh[k]), stored[k]), k


@pytest.mark.parametrize("name", list(C.CASES))
def test_fixture_inputs_are_the_seeds_and_the_ladder(name):
    fix = C.load(name)
    d = C.inputs(name)
    assert C.input_hash(d) == str(fix["input_hash"]) == C.input_hash(fix)
    assert os.path.getsize(os.path.join(C.GOLDEN, name + ".npz")) < 512 * 1024
    # every rung of the ladder once, to the rounding of the 2-norm
    assert np.allclose(np.sort(fix["norm2"]), C.CASES[name].get("ladder", C.LADDER), rtol=1e-12, atol=0)
    assert all(np.all(np.isfinite(fix[k])) for k in ("cons", "jac", "Jw", "JTw", "hess"))


@functools.lru_cache(maxsize=None)
def oracle_errors(name):
    fix = C.load(name)
    p, ev_o = C.at_point(name, fix["Z"])
    Z = fix["Z"]
    got = dict(cons=ev_o.eval_constraint(Z), jac=ev_o.eval_constraint_jacobian(Z),
               Jw=ev_o.eval_constraint_jacobian_product(Z, fix["w"]),
               JTw=ev_o.eval_constraint_jacobian_transpose_product(Z, fix["wt"]),
               hess=ev_o.eval_hessian_lagrangian(Z, 0.0, fix["mu"]))
    errs = C.errors(name, fix, got)
    print(C.report(name, fix, errs, "oracle vs fixture"))
    return errs


@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_is_within_its_cap_of_the_fixture(name):
    errs = oracle_errors(name)
    worst = {}
    for (cls, k), v in errs.items():
        if cls != "hess":
            worst[cls] = max(worst.get(cls, 0.0), v)
            assert v <= (0.0 if cls in ("const", "hess_outside_blocks") else C.ORACLE_CAP), (name, cls, k, v)
    print(name, "oracle, worst per class:", {c: f"{v:.1e}" for c, v in worst.items()})


@pytest.mark.parametrize("name", list(C.CASES))
def test_oracle_hessian_error_is_measured(name):
    """Not known in advance: printed per interval for DESIGN section 2.  What must hold whatever it is: it is finite, and the
    oracle writes nothing outside the interval blocks."""
    errs = oracle_errors(name)
    h = {k: v for (cls, k), v in errs.items() if cls == "hess"}
    print(name, "oracle Hessian, normwise per interval block:", {k: f"{v:.1e}" for k, v in sorted(h.items())})
    assert len(h) == C.N_KNOTS - 1 and all(np.isfinite(v) for v in h.values())
    assert errs[("hess_outside_blocks", 0)] == 0.0
