"""CPU: the references and bars of the scan accuracy tests (tests/scan_cases.py, tests/golden/*_scan_*.npz).

The fixtures extend the accuracy-budget fixtures they name by hash; the small ones come out of their generator bit for bit, the
large ones (66 states and more) are held by that hash, by their seeds and by the sequential fp64 recurrence on SciPy expm or the
oracle's map, which must stay within hp_cases.ORACLE_CAP = 1e-13 of every stored knot.  The yardstick of layer A -- rho, the error
of the NumPy restatement of the tree scan against exact arithmetic on the same matrices -- must stay under its a-priori bound, and
every stored bar is the rule of tests/scan_cases.py applied to what the fixture stores.

Then the bars are shown to discriminate: the restatement with one defect at a time (scan_cases.DEFECTS) on hp_s64 and tdbhp_n16_o0
against layer A's bar (exact arithmetic on the same E_k) and layer B's stored bars, beside the 1e-10 the rollout and solve tests
held before."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import hp_cases as HC
import hp_reference as HP
import scan_cases as S
import tdb_hp_reference as T

NAMES = list(S.CASES)


def _generator(case):
    name = "make_hp_golden" if S.CASES[case]["kind"] != "tdb" else "make_tdbhp_golden"
    spec = importlib.util.spec_from_file_location(name, os.path.join(S.GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def at(case):
    """(fixture, problem at its point, the oracle's fp64 E_k)"""
    fix = S.load(case)
    p, _ = S.point_of(case, fix)
    E = S.oracle_propagators(p)
    for a in list(fix.values()) + [E]:
        a.setflags(write=False)
    return fix, p, E


# ---- the references ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["tdbhp_n4", "tdbhp_n16_o0"])
def test_reversed_flow_on_the_negated_transposed_family_is_the_transpose_of_the_map(case):
    """flow_transposed against the columns of the whole Phi, where Phi is affordable: to 300 bits.  And `flow` on the transposed
    family at the same times is NOT Phi' where the stages do not commute (tdbhp_n4: order 1, carriers)."""
    fix, p, _ = at(case)
    it = p.integrators[0]
    n = it.x_dim
    fam = T.family(it.G, it.mods)
    fam_t = S.transposed_family(fam)
    plain_t = ([np.transpose(Bc, (0, 2, 1)) for Bc in fam[0]], fam[1], fam[2])
    tol = 1 << (T.FRAC_BITS - 300)
    for k in range(p.K):
        a = S.tdb_interval_args(p, k)
        Phi = T.flow(fam, it.spline_order, it.substeps, *a, HP.eye(n))
        back = S.flow_transposed(fam_t, it.spline_order, it.substeps, *a, HP.eye(n))
        assert max(abs(int(v)) for v in (Phi.T - back).flat) <= tol, k
        if case == "tdbhp_n4":
            same_times = T.flow(plain_t, it.spline_order, it.substeps, *a, HP.eye(n))
            assert max(abs(int(v)) for v in (Phi.T - same_times).flat) > 1 << (T.FRAC_BITS - 40), k


def test_exact_recurrences_are_the_recurrences():
    """On matrices of small integers over 8 every product is exact in fp64 too: `exact` and the fp64 recurrence agree bit for bit."""
    rng = np.random.default_rng(3)
    E = rng.integers(-3, 4, (3, 5, 5)) / 8.0
    X0, B = rng.integers(-3, 4, (2, 5)) / 4.0, rng.integers(-3, 4, (4, 2, 5)) / 4.0
    ex, seq = S.exact(E, X0, B), S.sequential(E, X0, B)
    for q in S.QUANTITIES:
        assert np.array_equal(ex[q], seq[q]), q


def test_the_metric_scales_a_knot_by_the_knots_behind_it():
    b = np.array([[[4.0]], [[1.0]], [[0.25]]])
    a = b + np.array([[[0.0]], [[0.5]], [[0.5]]])
    assert np.array_equal(S.knot_errors(a, b, False), [0.0, 0.125, 0.125])     # forward: max|b| over knots 0 .. t
    assert np.array_equal(S.knot_errors(a, b, True), [0.0, 0.5, 2.0])          # adjoint: over knots t .. K
    a[1] = np.nan
    assert S.knot_errors(a, b, False)[1] == np.inf


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", NAMES)
def test_fixture_extends_the_fixture_it_names_and_its_columns_are_the_seeds(case):
    fix, p, E = at(case)
    Z, h = S.base_inputs(case)
    assert str(fix["input_hash"]) == h
    n, N = p.integrators[0].x_dim, p.N
    assert N == (4 if S.CASES[case]["kind"] == "tdb" else 7)
    X0, B = S.columns(case, N)
    assert X0.shape == (3, n) and B.shape == (N, 3, n)
    assert np.array_equal(fix["X0"], X0) and np.array_equal(fix["B"], B)
    for q in S.QUANTITIES:
        assert fix[q].shape == (N, 3, n) and np.all(np.isfinite(fix[q])), q
    assert np.array_equal(fix["X"][0], X0) and np.array_equal(fix["Y"][0], B[0]) and np.array_equal(fix["Lam"][-1], B[-1])
    assert os.path.getsize(os.path.join(S.GOLDEN, S.fixture_name(case) + ".npz")) < 256 * 1024
    if S.CASES[case]["kind"] == "damped":       # contractive: the rolled states decay by more than an order over the ladder
        G0 = p.integrators[0].G[0]
        assert np.linalg.eigvalsh(G0 + G0.T).max() <= 1e-12 and np.abs(G0 + G0.T).max() > 0.1
        size = np.abs(fix["X"]).reshape(N, -1).max(axis=1)
        assert size[-1] < size[0] / 20.0, size
    elif S.CASES[case]["kind"] == "hp":
        assert np.abs(p.integrators[0].G + p.integrators[0].G.transpose(0, 2, 1)).max() < 1e-15


@pytest.mark.parametrize("case", S.REGENERATED)
def test_small_fixture_regenerates_bit_for_bit(case):
    """The 320-bit parts bit for bit; what a BLAS sums (yard, rho, the bars built on them) to its own accuracy."""
    fresh, stored = _generator(case).build_scan(case), S.load(case)
    assert sorted(fresh) == sorted(stored)
    for k in ("input_hash", "X0", "B", "X", "Y", "Lam") + (("Z",) if "Z" in stored else ()):
        assert np.array_equal(fresh[k], stored[k]), k
    assert np.allclose(fresh["bars"], stored["bars"], rtol=0.5, atol=0.0)
    if S.CASES[case]["kind"] != "damped":
        assert np.array_equal(fresh["b_fwd"], stored["b_fwd"]) and np.array_equal(fresh["b_adj"], stored["b_adj"])


@pytest.mark.parametrize("case", NAMES)
def test_sequential_fp64_recurrence_stays_within_its_cap_of_the_320_bit_values(case):
    fix, p, E = at(case)
    yard = S.errors(S.sequential(E, fix["X0"], fix["B"]), fix)
    print(case, "sequential fp64 recurrence, worst per quantity:", {q: f"{v.max():.2e}" for q, v in yard.items()})
    for i, q in enumerate(S.QUANTITIES):
        assert np.all(yard[q] <= HC.ORACLE_CAP), (case, q, yard[q])
        assert np.all(fix["yard"][i] <= HC.ORACLE_CAP), (case, q, fix["yard"][i])


@pytest.mark.parametrize("case", NAMES)
def test_rho_stays_under_its_a_priori_bound_and_the_bars_are_the_rule(case):
    fix, p, E = at(case)
    rho = S.rho(E, fix["X0"], fix["B"])
    bound = S.rho_bound(E)
    print(case, "rho", {q: f"{v:.2e}" for q, v in rho.items()}, "a-priori bound", f"{bound:.2e}", "kappa", S.kappa(E))
    assert np.isclose(bound, float(fix["rho_bound"]), rtol=1e-6)
    for i, q in enumerate(S.QUANTITIES):
        assert rho[q] <= bound and fix["rho"][i] <= float(fix["rho_bound"]), (case, q)
        assert rho[q] <= S.bar_a(fix["rho"][i])       # measured again (another BLAS sums in another order) it stays under its own bar
    # the stored bars: the rule applied to the stored interval bars and the stored rho
    K = p.K
    kind = S.CASES[case]["kind"]
    if kind != "damped":
        b_fwd, b_adj = S.interval_bars(case, E, None, None)
        assert np.array_equal(b_fwd, fix["b_fwd"]) and np.array_equal(b_adj, fix["b_adj"])
    if kind == "hp":
        assert sorted(fix["b_fwd"]) == [HC.BAR_NO_SQUARING] + [HC.BAR] * (K - 1)
    assert fix["b_fwd"].shape == fix["b_adj"].shape == (K,) and fix["b_fwd"].min() >= S.FLOOR and fix["b_adj"].min() >= S.FLOOR
    rule = S.layer_b_bars(E, fix, fix["b_fwd"], fix["b_adj"], dict(zip(S.QUANTITIES, fix["rho"])))
    assert fix["bars"].shape == (3, K + 1) and np.allclose(rule, fix["bars"], rtol=1e-6, atol=0.0)
    assert fix["bars"].min() >= S.FLOOR and fix["bars"].max() < S.OLD_BAR / 10.0
    if kind == "hp":     # orthogonal propagation: alpha <= 1, no bar passes the sum of the interval bars and layer A's term
        assert np.all(fix["bars"] <= fix["b_fwd"].sum() * (1.0 + 1e-9) + S.bar_a(fix["rho"].max()))


# ---- the bars discriminate ----------------------------------------------------------------------------------------------------------

DEFECT_CASES = ["hp_s64", "tdbhp_n16_o0"]


@functools.lru_cache(maxsize=None)
def defective(case, defect):
    """({quantity: worst error / bar} for layer A, the same for layer B, worst error against the 320-bit values) of the restatement
    with `defect` (None: none) on the oracle's E_k.  The fp32 leaf is the interval of the smallest step norm."""
    fix, p, E = at(case)
    leaf = int(np.argmin([np.linalg.norm(Ek - np.eye(E.shape[1]), 2) for Ek in E]))
    got = S.restated(E, fix["X0"], fix["B"], defect, leaf)
    ea, eb = S.errors(got, S.exact(E, fix["X0"], fix["B"])), S.errors(got, fix)
    a = {q: float(np.max(ea[q] / S.bar_a(fix["rho"][i]))) for i, q in enumerate(S.QUANTITIES)}
    b = {q: float(np.max(eb[q] / fix["bars"][i])) for i, q in enumerate(S.QUANTITIES)}
    worst = {q: float(eb[q].max()) for q in S.QUANTITIES}
    print(f"{case} defect={defect}: error / bar, layer A {a}, layer B {b}; worst error against the 320-bit values {worst}")
    return a, b, worst


@pytest.mark.parametrize("case", DEFECT_CASES)
def test_a_defect_free_restatement_stays_under_every_bar(case):
    a, b, _ = defective(case, None)
    assert max(a.values()) <= 1.0 and max(b.values()) <= 1.0, (a, b)


@pytest.mark.parametrize("case", DEFECT_CASES)
def test_a_tree_node_off_by_a_relative_1e_11_lands_over_both_layers_and_under_the_old_bar(case):
    a, b, worst = defective(case, "node")
    assert max(a.values()) > 1.0 and max(b.values()) > 1.0, (a, b)
    assert min(a.values()) > 1.0          # every quantity reads the tree
    assert max(worst.values()) < S.OLD_BAR, worst


@pytest.mark.parametrize("case", DEFECT_CASES)
def test_a_leaf_rounded_to_fp32_lands_over_both_layers(case):
    """The leaf of the smallest step.  Layer A sees it by orders; so does layer B.  Against the old bar: an fp32 rounding of a
    matrix with entries near 1 is an error of 2^-25 ~ 3e-8 in the state, which 1e-10 catches too -- measured and asserted here as
    it is, not as hoped."""
    a, b, worst = defective(case, "leaf32")
    assert min(a.values()) > 100.0 and min(b.values()) > 100.0, (a, b)
    assert max(worst.values()) > S.OLD_BAR, worst


@pytest.mark.parametrize("case", DEFECT_CASES)
def test_the_left_childs_offset_in_the_adjoints_up_sweep_lands_over_the_bar(case):
    a, b, _ = defective(case, "left_offset")
    assert a["Lam"] > 100.0 and b["Lam"] > 100.0, (a, b)
    clean = defective(case, None)[0]
    assert a["X"] == clean["X"] and a["Y"] == clean["Y"]          # the forward scans do not read it


@pytest.mark.parametrize("case", DEFECT_CASES)
def test_another_order_of_the_same_sum_stays_under_the_bar(case):
    """The addend joined to the product's first k block: the same value in exact arithmetic.  A control that the bar is no bit
    comparison."""
    fix, p, E = at(case)
    a, b, _ = defective(case, "addend_first")
    assert max(a.values()) <= 1.0 and max(b.values()) <= 1.0, (a, b)
    clean, other = S.restated(E, fix["X0"], fix["B"]), S.restated(E, fix["X0"], fix["B"], "addend_first")
    assert any(not np.array_equal(clean[q], other[q]) for q in S.QUANTITIES), "the control changed no bit"


@pytest.mark.parametrize("case", DEFECT_CASES)
def test_a_propagator_where_an_identity_leaf_belongs_reaches_no_live_knot(case):
    """The last E_k in the leaves beyond K.  The plan keeps those leaves away from every live knot: a forward item whose node
    holds one writes a knot past K (dead), and the adjoint reads such a node only against the zero offsets behind knot K, which
    the plan marks `src_zero` and copies without a product (tests/test_dynamics_solve_plan_header.py asserts the marking).  So
    this defect cannot show in X, Y or Lam -- in the adjoint either -- and what is asserted is that it changes no bit; the node
    products themselves differ."""
    fix, p, E = at(case)
    clean, other = S.restated(E, fix["X0"], fix["B"]), S.restated(E, fix["X0"], fix["B"], "leaf_beyond")
    for q in S.QUANTITIES:
        assert np.array_equal(clean[q], other[q]), q
    fw = S.plans(p.K)[0]
    trees = [S.tree_products(fw, S.matrix_tree(fw, list(E), d)) for d in (None, "leaf_beyond")]
    assert len(fw["leaf"]) > p.K and not np.array_equal(trees[0], trees[1])
    assert defective(case, "leaf_beyond")[0] == defective(case, None)[0]
