"""CPU: the 320-bit reference (tests/hp_reference.py) is pinned, the accuracy-budget fixtures (tests/golden/hp_*.npz) come out of
their generator, and the fp64 oracle sits within 1e-13 of every fixture in the normwise metric per interval and quantity class
(tests/hp_cases.py).  The oracle's Hessian error is printed per interval; DESIGN section 2 records it.  From 130 states on a
fixture's Jacobian knows 16 sampled columns of each E_k block (`jac_known`); the cap holds there as well, measured: worst class
4.2e-14 (J' w of hp_ring256)."""
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


@pytest.mark.parametrize("n", [6, 12])
@pytest.mark.parametrize("kind", ["skew", "general"])
def test_sampled_propagator_columns_are_the_columns_of_the_exponential(n, kind):
    """interval(E_cols=...) forms the columns as actions of exp(A) on unit vectors and calls no expm: they equal the same columns
    of expm(A) to 1e-80, the bar the action is held to against expm above."""
    rng = np.random.default_rng(9 + n)
    m = 2
    G = rng.standard_normal((m + 1, n, n))
    if kind == "skew":
        G = G - G.transpose(0, 2, 1)
    x, xn, u = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(m)
    cols = [0, n - 1, 3, 2]      # unsorted on purpose: column j of the result is column cols[j] of E
    R = HP.interval(G, x, u, 0.6, xn, want_E=False, E_cols=cols)
    assert R["E"] is None and R["E_cols"].shape == (n, len(cols))
    E = HP.expm(R["A"])
    assert max(abs(int(v)) for v in (R["E_cols"] - E[:, cols]).reshape(-1)) / HP.ONE <= 1e-80
    # and a whole E beside them is the one interval() always returned
    R2 = HP.interval(G, x, u, 0.6, xn, E_cols=cols[:1])
    assert all(int(a) == int(b) for a, b in zip(R2["E"].reshape(-1), E.reshape(-1)))


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
    assert all(np.all(np.isfinite(fix[k])) for k in ("cons", "Jw", "JTw", "hess"))
    if "jac_known" not in fix:
        assert np.all(np.isfinite(fix["jac"]))
        return
    # sampled E_k: the Jacobian is finite exactly where it is known, and what is unknown lies in the E_k blocks' other columns
    assert fix["jac_known"].dtype == bool and np.array_equal(np.isfinite(fix["jac"]), fix["jac_known"])
    cols = C.E_columns(name)
    assert np.array_equal(fix["E_cols"], cols) and len(cols) == 16
    n = C.CASES[name]["n"]
    assert {0, 15, 16, 63, 64, n - 1} | {b + s for b in range(128, n, 128) for s in (-1, 0)} <= set(cols.tolist())
    p, ev_o = C.at_point(name, fix["Z"])
    it = p.integrators[0]
    unknown_cols = np.unique((ev_o.jac_cols[~fix["jac_known"]] % p.z) - it.x_off)
    assert np.array_equal(unknown_cols, np.setdiff1d(np.arange(n), cols))
    assert np.count_nonzero(~fix["jac_known"]) == p.K * n * (n - 16)


def test_sampled_metric_reads_known_entries_and_lets_no_nan_through():
    """Under `jac_known` the E class compares the sampled columns alone, but an entry nobody wrote (NaN) anywhere in the block
    still fails it."""
    name = "hp_tile192"
    fix = C.load(name)
    unknown = np.flatnonzero(~fix["jac_known"])
    got = np.where(fix["jac_known"], fix["jac"], 123.0)           # exact where known, anything finite elsewhere
    errs = C.errors(name, fix, dict(jac=got))
    assert all(v == 0.0 for (cls, k), v in errs.items())
    got[unknown[len(unknown) // 2]] = np.nan
    errs = C.errors(name, fix, dict(jac=got))
    assert sorted(v for (cls, k), v in errs.items() if cls == "E")[-2:] == [0.0, np.inf]
    known_E = np.flatnonzero(fix["jac_known"] & (np.abs(fix["jac"]) < 0.9) & (fix["jac"] != 0.0))
    got = np.where(fix["jac_known"], fix["jac"], 123.0)
    got[known_E[0]] += 1e-9                                       # a sampled entry off by 1e-9 shows
    assert max(v for (cls, k), v in C.errors(name, fix, dict(jac=got)).items() if cls in ("E", "u0", "dt")) > 1e-10


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
