"""GPU: the reduced-space stack at long horizons and past the flat launches' grid caps -- the whole-dynamics solves (csrc/dto_elim.hip),
the reduced gradient and Hessian products on both routes (csrc/dto_reduced.hip, option "reduced_input_store"), the block products
(k_hess_spmm and the *_block kernels) and the rollout's compaction (csrc/dto_rollout.hip).

C1, C2 -- horizon length.  K = 1, 2, 64, 65, 257 and a three-level layout at 12 states, 40 x 258 on the one-launch chain: VALUES against the
sparse reference of long_cases.py (the oracle alone, no dense N D matrix) under the unchanged bars of reduced_cases and
test_gpu_rollout.bar(K) x levels, on smoothed directions whose kappa is asserted; BITS against reduced_cases.compose_* (default route),
against the NumPy restatement of reduced_input_cases (store route), and of the block call against the single products.

C3 -- past the caps.  flat_grid / red_grid cap a launch at 4096 workgroups of 256 threads; past 1 048 576 entries a grid-stride loop
takes over.  At scaled_64x320 with 64 columns k_elim_couple, k_elim_collect, k_rollout_compact and every block packer cross that count
(the totals are asserted from the handle's sizes), while the single-vector and single-column forms stay below it: an independent path
the block results must reproduce bit for bit.  No oracle Hessian is evaluated at this shape.

C4 -- k_hess_gather caps at 8192 workgroups, 2 097 152 entries of the row-major Hessian copy.  The 256-state problem of
test_gpu_hessian_product.py has 360 198 of them at 200 knots (measured), about 1 810 per interval (both triangles of the (x, u), (x, dt)
and small blocks, the odd rows padded): N = 1200 crosses the cap, which the test asserts from the bytes a kept-point product books.

Outputs are pre-filled with NaN by the mirror; every comparison also asserts that none is left.  The largest errors seen are in
DESIGN 4.30."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import long_cases as L
import reduced_cases as R
import reduced_input_cases as RI
from helpers import rel_err, to_engine
from test_gpu_hessian_product import _product, _sym_product
from test_gpu_reduced_input import evaluator, launches
from test_gpu_rollout import bar

pytestmark = pytest.mark.gpu

OPERATOR_CASES = L.C1_OPERATOR_CASES + [L.C2_CASE]
SOLVE_CASES = L.C1_CASES + [L.C2_CASE]
ROUTES = {"store": 1, "default": 0}
FLAT_CAP = 4096 * 256          # entries one pass of a capped flat launch covers
PROBED = [0, 17, 63]           # the columns of a 64-column call that are run alone


def block_columns(name):
    """13 columns at 12 states (the column limit, 12, makes two chunks), 40 at 40 states"""
    return 40 if name == L.C2_CASE else 13


@functools.lru_cache(maxsize=None)
def vectors(name):
    c = L.case(name)
    V = np.random.default_rng(1000 + len(name)).standard_normal((block_columns(name), c["p"].n_vars))
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def route(name, store):
    """one handle per case and route: the products of the case's two smoothed directions, the gradient with its costates, the single
    product of every random column and the block call on them"""
    c, V = L.case(name), vectors(name)
    Z, mu = c["Z"], c["mu"]
    ev = evaluator(c, store)
    try:
        ys = [ev.reduced_hessian_product(Z, v, R.SIGMA, mu) for v in c["vs"]]     # a product first: it computes the point itself
        r, lam = ev.reduced_lagrangian_gradient(Z, R.SIGMA, mu, costates=True)
        singles = np.stack([ev.reduced_hessian_product(Z, v, R.SIGMA, mu) for v in V])
        block = ev.reduced_hessian_products(Z, V, R.SIGMA, mu)
    finally:
        ev.close()
    return dict(ys=ys, r=r, lam=lam, singles=singles, block=block)


@functools.lru_cache(maxsize=None)
def composed(name):
    """both compositions on one fresh handle (public methods alone): the default route's with the engine's J w / J' w, the store route's
    with the sums over entries cut from the engine's public Jacobian values; gradient and the first two random columns"""
    c, V = L.case(name), vectors(name)
    p, Z, mu = c["p"], c["Z"], c["mu"]
    ev = evaluator(c, None)
    try:
        r, lam, mut = R.compose_gradient(ev, p, Z, R.SIGMA, mu)
        ys = [R.compose_product(ev, p, Z, R.SIGMA, mu, v, mut=mut) for v in V[:2]]
        S = RI.store_from_jacobian(ev, p, Z)
        rs, lams, muts = RI.compose_gradient(ev, p, Z, R.SIGMA, mu, S)
        yss = [RI.compose_product(ev, p, Z, R.SIGMA, mu, v, S, muts) for v in V[:2]]
    finally:
        ev.close()
    return {0: dict(r=r, lam=lam, ys=ys), 1: dict(r=rs, lam=lams, ys=yss)}


# ------------------------------------------------------------------------------------------------ C1, C2: the solves' values
@pytest.mark.parametrize("name", SOLVE_CASES)
def test_whole_dynamics_solves_against_the_sparse_solve(name):
    c = L.jac_case(name)
    K, limit = c["p"].N - 1, bar(c["p"].N - 1) * c["levels"]
    ev = evaluator(c, None)
    try:
        assert ev.dynamics_layout()[:2] == (c["D"], c["levels"])
        Y = ev.dynamics_solve_all(c["Z"], c["B"])
        Lam = ev.dynamics_solve_all(c["Z"], c["B"], adjoint=True)
    finally:
        ev.close()
    assert Y.shape == Lam.shape == c["B"].shape and not np.isnan(Y).any() and not np.isnan(Lam).any()
    errs = dict(forward=rel_err(Y, c["ref_solve"][0]), adjoint=rel_err(Lam, c["ref_solve"][1]))
    print(name, "K", K, "levels", c["levels"], errs, "bar", limit, "max |y|", float(np.max(np.abs(c["ref_solve"][0]))),
          float(np.max(np.abs(c["ref_solve"][1]))))
    for what, e in errs.items():
        assert e <= limit, (name, what, e)


# ---------------------------------------------------------------------------------------------- C1, C2: the operators' values
@pytest.mark.parametrize("which", list(ROUTES))
@pytest.mark.parametrize("name", OPERATOR_CASES)
def test_operators_against_the_sparse_reference(name, which):
    c, g = L.case(name), route(name, ROUTES[which])
    ref = c["ref"]
    assert not np.isnan(g["r"]).any() and not np.isnan(g["lam"]).any()
    eg, bg = float(np.linalg.norm(g["r"] - ref["r_ref"])), L.gradient_bar(ref, c["levels"])
    print(name, which, "gradient error", eg, "bar", bg, "ratio", eg / bg, "||T||", ref["nT"], "||H||", ref["nH"], "||g||", ref["ng"])
    assert eg <= bg
    assert np.all(g["r"][ref["S"]] == 0.0)
    for v, y, yr in zip(c["vs"], g["ys"], c["ys"]):
        assert not np.isnan(y).any()
        e, b, k = float(np.linalg.norm(y - yr)), L.product_bar(ref, v), L.kappa(ref, v, yr)
        print(name, which, "product error", e, "bar", b, "ratio", e / b, "relative", e / float(np.linalg.norm(yr)), "kappa", k)
        assert k <= L.KAPPA_CAP, "the direction is too ill-conditioned for its bar"
        assert e <= b
        assert np.all(y[ref["S"]] == 0.0)


# ------------------------------------------------------------------------------------------------------ C1, C2: the bits
@pytest.mark.parametrize("which", list(ROUTES))
@pytest.mark.parametrize("name", OPERATOR_CASES)
def test_operators_bit_for_bit_against_their_composition(name, which):
    g, want = route(name, ROUTES[which]), composed(name)[ROUTES[which]]
    assert not np.isnan(g["r"]).any() and not np.isnan(g["lam"]).any()
    print(name, which, "gradient entries that differ", int(np.sum(g["r"] != want["r"])), "costates", int(np.sum(g["lam"] != want["lam"])))
    assert np.array_equal(g["lam"], want["lam"]) and np.array_equal(g["r"], want["r"])
    for y, yc in zip(g["singles"][:2], want["ys"]):
        print(name, which, "product entries that differ", int(np.sum(y != yc)), "largest", float(np.max(np.abs(y - yc))))
        assert not np.isnan(y).any() and np.array_equal(y, yc)


@pytest.mark.parametrize("which", list(ROUTES))
@pytest.mark.parametrize("name", OPERATOR_CASES)
def test_the_block_call_has_the_bits_of_the_single_products(name, which):
    g = route(name, ROUTES[which])
    Y, want = g["block"], g["singles"]
    print(name, which, "columns", Y.shape[0], "entries that differ", int(np.sum(Y != want)))
    assert Y.shape == want.shape == vectors(name).shape and not np.isnan(want).any() and not np.isnan(Y).any()
    assert np.array_equal(Y, want)


# ---------------------------------------------------------------------------------------------------- C3: past the caps
def c3_evaluator(store=None):
    return evaluator(L.jac_case(L.C3_CASE), store)


@functools.lru_cache(maxsize=None)
def c3_inputs():
    c = L.jac_case(L.C3_CASE)
    p = c["p"]
    rng = np.random.default_rng(64320)
    B = rng.standard_normal((p.N, 64, c["D"]))
    B[:, PROBED, :] = c["B"]                                      # the three columns with a sparse solution
    X0 = rng.standard_normal((64, p.integrators[0].x_dim))
    V = rng.standard_normal((64, p.n_vars))
    mu = rng.standard_normal(c["n_cons"])
    for a in (B, X0, V, mu):
        a.setflags(write=False)
    return dict(B=B, X0=X0, V=V, mu=mu)


def test_past_the_caps_the_launch_totals_exceed_one_pass():
    c = L.jac_case(L.C3_CASE)
    ev = c3_evaluator()
    try:
        N, n_vars, n_cons, (D, _, offset, level) = ev.trajectory.N, ev.n_variables, ev.n_constraints, ev.dynamics_layout()
    finally:
        ev.close()
    n, w = c["p"].integrators[0].x_dim, 64
    totals = {"k_elim_couple, k_elim_collect, k_rollout_compact: N n_cols n": N * w * n, "block packers over n_vars w": n_vars * w,
              "block packers over N w D": N * w * D, "block packers over n_cons w": n_cons * w}
    print(L.C3_CASE, "N", N, "D", D, "n", n, "n_vars", n_vars, "n_cons", n_cons, "one pass", FLAT_CAP, totals)
    assert (N, D, n, n_vars) == (c["p"].N, c["D"], 64, c["p"].n_vars) and level[0] == 1, "the 64-state integrator has coupling blocks"
    for what, total in totals.items():
        assert total > FLAT_CAP, (what, total)
    assert max(n_vars, n_cons, N * D) < FLAT_CAP, "the single-vector forms stay in one pass: an independent path"
    assert N * n * 1 < FLAT_CAP, "and so do the single-column solves and rollouts"


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
def test_past_the_caps_whole_dynamics_solves_with_64_columns(adjoint):
    c, B = L.jac_case(L.C3_CASE), c3_inputs()["B"]
    K, limit = c["p"].N - 1, bar(c["p"].N - 1) * c["levels"]
    ev = c3_evaluator()
    try:
        Y = ev.dynamics_solve_all(c["Z"], B, adjoint=adjoint)
        alone = [ev.dynamics_solve_all(c["Z"], B[:, j:j + 1], adjoint=adjoint) for j in PROBED]
    finally:
        ev.close()
    assert Y.shape == B.shape and not np.isnan(Y).any()
    for j, Yj in zip(PROBED, alone):
        print("column", j, "entries that differ from its run alone", int(np.sum(Y[:, j] != Yj[:, 0])))
        assert not np.isnan(Yj).any() and np.array_equal(Y[:, j], Yj[:, 0]), j
    e = rel_err(Y[:, PROBED], c["ref_solve"][1 if adjoint else 0])
    print(L.C3_CASE, "adjoint" if adjoint else "forward", "K", K, "error against the sparse solve", e, "bar", limit)
    assert e <= limit


def test_past_the_caps_rollout_with_64_columns():
    c, X0 = L.jac_case(L.C3_CASE), c3_inputs()["X0"]
    ev = c3_evaluator()
    try:
        X = ev.rollout(c["Z"], integrator=0, X0=X0)
        alone = [ev.rollout(c["Z"], integrator=0, X0=X0[j]) for j in PROBED]
    finally:
        ev.close()
    assert X.shape == (c["p"].N, 64, 64) and not np.isnan(X).any() and np.array_equal(X[0], X0)
    for j, Xj in zip(PROBED, alone):
        print("column", j, "entries that differ from its run alone", int(np.sum(X[:, j] != Xj[:, 0])))
        assert not np.isnan(Xj).any() and np.array_equal(X[:, j], Xj[:, 0]), j
    norms = np.linalg.norm(X, axis=2)
    assert np.max(np.abs(norms - norms[0])) <= 1e-9 * np.max(norms[0]), "skew generators: every propagator is orthogonal"


@pytest.mark.parametrize("which", list(ROUTES))
def test_past_the_caps_reduced_block_products_with_64_columns(which):
    c, V = L.jac_case(L.C3_CASE), c3_inputs()["V"]
    Z = c["Z"]
    ev = c3_evaluator(ROUTES[which])
    try:
        want = np.stack([ev.reduced_hessian_product(Z, v, R.SIGMA) for v in V])        # the singles; they compute and keep the point
        ev.profile_enable(True)
        ev.profile_reset()
        Y = ev.reduced_hessian_products(Z, V, R.SIGMA)
        chunks, trees = launches(ev, "hess_product", "dynsolve_tree")
        ev.profile_enable(False)
    finally:
        ev.close()
    print(L.C3_CASE, which, "hess_product launches", chunks, "entries that differ", int(np.sum(Y != want)), "columns that differ",
          int(np.sum(np.any(Y != want, axis=1))))
    assert (chunks, trees) == (1, 0), "one chunk of 64 columns at the kept point"
    assert Y.shape == want.shape and not np.isnan(want).any() and not np.isnan(Y).any()
    assert np.array_equal(Y, want)
    S = R.index_sets(c["p"])[0]
    assert np.all(Y[:, S] == 0.0) and np.any(Y != 0.0)


def test_past_the_caps_hessian_block_products_with_64_columns():
    c, q = L.jac_case(L.C3_CASE), c3_inputs()
    Z, V, mu = c["Z"], q["V"], q["mu"]
    ev = c3_evaluator()
    try:
        want = np.full(V.shape, np.nan)
        for j in range(V.shape[0]):
            ev.eval_hessian_lagrangian_product(want[j], Z, V[j], R.SIGMA, mu)
        Y = np.full(V.shape, np.nan)
        ev.eval_hessian_lagrangian_products(Y, Z, V, R.SIGMA, mu)
        h = np.full(ev.n_hessian_entries, np.nan)
        ev.eval_hessian_lagrangian(h, Z, R.SIGMA, mu)
        rows, cols = ev.hessian_lagrangian_structure()
    finally:
        ev.close()
    assert not np.isnan(want).any() and not np.isnan(Y).any() and not np.isnan(h).any()
    print(L.C3_CASE, "H V: entries that differ", int(np.sum(Y != want)))
    assert np.array_equal(Y, want)
    e = rel_err(Y[17], _sym_product(rows, cols, h, V[17]))
    print(L.C3_CASE, "column 17 against NumPy's product of the engine's own Hessian", e)
    assert e <= 1e-13


# ------------------------------------------------------------------------------- C4: k_hess_gather past 8192 workgroups
HESS_GATHER_CAP = 8192 * 256
HESS_GATHER_N = 1200           # 256 states: 360 198 entries at N = 200, about 1 810 more per interval


def test_hessian_gather_past_its_cap_matches_the_engines_own_hessian():
    """the 256-state problem of test_product_matches_the_engines_own_hessian_and_the_device_form with N raised until the row-major copy
    (hp_nnz entries) no longer fits one pass of k_hess_gather; a product at the kept point books 12 hp_nnz + 32 n_vars bytes.

    The bar of that test, rel_err <= 1e-13, cannot be met at this length by ANY float64 summation and is not asserted here.  Measured:
    3.6e-13 against NumPy's float64 product, 1.5e-13 against the np.longdouble product, and NumPy's float64 product itself is 2.1e-13
    from the np.longdouble one -- all three at the timestep row of knot 755, whose 260 terms of total magnitude 1.3e4 cancel to 4.7
    (at N = 200 the worst row cancels 1.2e4 to 44 and the figure is 1.7e-14).  The engine's absolute error there is 0.25 eps
    sum_j |h_ij v_j|.  rel_err floors the denominator at 1 and takes the worst of N z rows, so it grows with the number of rows drawn.
    What is asserted instead, row by row against the np.longdouble product: |y_i - ref_i| <= 2 z eps sum_j |h_ij v_j|, four times the
    a-priori bound n u sum |terms| of a sum of n <= z products in any order (u = eps / 2).  An entry the gather misses or misplaces
    shows as an error of the order of a whole term, 1e12 times that."""
    p = O.make_scaled_problem(HESS_GATHER_N, 256, 2, seed=4, with_constraint=True)
    ev = dto_amd.Evaluator(to_engine(p))
    try:
        rng = np.random.default_rng(2)
        Z = p.Z0 + 0.01 * rng.standard_normal(p.n_vars)
        mu = rng.standard_normal(ev.n_constraints)
        v = rng.standard_normal(ev.n_variables)
        y = _product(ev, Z, v, 0.7, mu)                               # a new point: the assembly, the gather, the product
        ev.profile_enable(True)
        ev.profile_reset()
        assert np.array_equal(_product(ev, Z, v, 0.7, mu), y)         # the kept point: the product launch alone
        _, n_launches, n_bytes = ev.profile_get("hess_product")
        ev.profile_enable(False)
        hp_nnz = (n_bytes - 32.0 * ev.n_variables) / 12.0
        print("256 x", HESS_GATHER_N, "hp_nnz", hp_nnz, "one pass of k_hess_gather", HESS_GATHER_CAP)
        assert n_launches == 1 and hp_nnz == int(hp_nnz) and hp_nnz > HESS_GATHER_CAP
        h = np.full(ev.n_hessian_entries, np.nan)
        ev.eval_hessian_lagrangian(h, Z, 0.7, mu)
        r, c = ev.hessian_lagrangian_structure()
    finally:
        ev.close()
    assert not np.isnan(y).any() and not np.isnan(h).any()
    # NumPy's symmetric product of the engine's own Hessian, in np.longdouble, with sum_j |h_ij v_j| beside it.  (The structure lists
    # whole blocks: all but about a hundredth of the stored values are zero and are left out of the sums.)
    ld = np.longdouble
    nz = np.flatnonzero(h)
    r0, c0, hl, vl = np.asarray(r)[nz] - 1, np.asarray(c)[nz] - 1, h[nz].astype(ld), v.astype(ld)
    del r, c
    ref, mag = np.zeros(v.size, dtype=ld), np.zeros(v.size, dtype=ld)
    t = hl * vl[c0]
    np.add.at(ref, r0, t), np.add.at(mag, r0, np.abs(t))
    off = r0 != c0
    t = hl[off] * vl[r0[off]]
    np.add.at(ref, c0[off], t), np.add.at(mag, c0[off], np.abs(t))
    err = np.abs(y.astype(ld) - ref)
    bound = 2 * p.z * np.finfo(np.float64).eps * mag
    i = int(np.argmax(err / np.maximum(bound, np.finfo(np.float64).tiny)))
    e = rel_err(y, ref.astype(np.float64))
    print("256 x", HESS_GATHER_N, "largest error / rounding bound", float(err[i] / bound[i]), "at row", i, "knot", i // p.z, "component", i % p.z,
          "|ref|", float(abs(ref[i])), "sum |h v|", float(mag[i]), "; rel_err (not asserted, see the docstring)", e)
    assert np.all(err <= bound)
