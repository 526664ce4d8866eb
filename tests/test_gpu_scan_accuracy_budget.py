"""GPU: the rollout and both solves with the dynamics block (dto_rollout, dto_dynamics_solve; csrc/dto_rollout.hip,
csrc/dto_dynsolve.hip) held to the 320-bit references, in the metric and under the bars of tests/scan_cases.py.

Layer A, the scan alone: the handle's Jacobian at the fixture's point (into NaN) gives the engine's own E_k -- the same do_jacobian
a rollout runs, whose bits the determinism suite holds -- and the three recurrences are carried out on those matrices in exact
arithmetic (2^-320 per product, one rounding at the end).  What is left is the scan's own fp64 arithmetic: tree products, descent,
offsets, the transposed operand.  Bar: 16 rho floored at 64 2^-53, rho the error of the NumPy restatement of the same tree scan on
the same matrices; rho must stay under its a-priori bound (2L + 1) n 2^-53 kappa.  Nothing the scan under test returns sets a bar.

Layer B, end to end: against the fixtures tests/golden/*_scan_*.npz -- 320-bit values of the true propagators -- under the bars the
fixture's generator wrote (the budget of every interval's E_k, amplified by what follows it, plus layer A's term).

One handle per case (`run`), every entry point once into NaN-filled outputs; the tables print per case and quantity the engine's
error at every knot beside its bar.  DESIGN 4.23 and 4.25 record them."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import scan_cases as S
import tdbhp_cases as TC
from helpers import to_engine

pytestmark = pytest.mark.gpu

NAMES = list(S.CASES)
BITS = [c for c in NAMES if "bits" in S.CASES[c]]
COUNTERS = ("rollout", "rollout_tree", "dynsolve", "dynsolve_tree", "tdb_mfma", "tdb_kron")


def open_case(case):
    """(handle, Z, integrator, problem the handle was made of, fixture): the case's handle at its fixture's point.  tdbhp_n72 is
    the group of two, and the integrator is its follower."""
    fix = S.load(case)
    p, Z = S.point_of(case, fix)
    integrator, kw = 0, S.engine_kw(case)
    if S.CASES[case].get("group"):
        p, d = TC.group_problem(case, TC.load(case))
        Z, integrator, kw = d["Z"], 1, dict(kw, shared_generators=True)
    return dto_amd.Evaluator(to_engine(p), **kw), Z, integrator, p, fix


def engine_propagators(ev, Z, p, q):
    """(K, n, n): the -E_k blocks of integrator q cut out of the handle's Jacobian (into NaN) and negated."""
    ev_o = O.OracleEvaluator(p)
    jac = np.full(ev.shard.jac_len, np.nan)
    ev.eval_constraint_jacobian(jac, Z)
    its = p.integrators
    n, K, z = its[q].x_dim, p.K, p.z
    row0 = sum(it.x_dim for it in its[:q]) * K
    rows, cols = np.asarray(ev_o.jac_rows), np.asarray(ev_o.jac_cols)
    E = np.zeros((K, n, n))
    for k in range(K):
        r0, c0 = row0 + k * n, k * z + its[q].x_off
        sel = (rows >= r0) & (rows < r0 + n) & (cols >= c0) & (cols < c0 + n)
        assert sel.sum() >= n, (k, int(sel.sum()))
        E[k][rows[sel] - r0, cols[sel] - c0] = -jac[sel]
    assert np.all(np.isfinite(E)), "the Jacobian left an entry of an E_k block unwritten"
    return E


def _three(ev, Z, q, X0, B):
    return dict(X=ev.rollout(Z, integrator=q, X0=X0), Y=ev.dynamics_solve(Z, B, integrator=q),
                Lam=ev.dynamics_solve(Z, B, integrator=q, adjoint=True))


@functools.lru_cache(maxsize=None)
def run(case):
    """Everything the tests of a case read, from one handle: per column count the engine's X, Y, Lam and layer A's exact values,
    rho and bound; the bit comparisons of the ring cases; the group's checks."""
    ev, Z, q, p, fix = open_case(case)
    out = dict(fix=fix, runs={})
    try:
        ev.profile_enable(True)
        ev.profile_reset()
        if S.CASES[case].get("group"):
            out["share"] = [ev.integrator_share(i) for i in range(2)]
        E = engine_propagators(ev, Z, p, q)
        n = E.shape[1]
        out["E"] = E
        if S.CASES[case].get("group"):
            out["leader_blocks_equal"] = np.array_equal(E, engine_propagators(ev, Z, p, 0))
            out["leader_rollout"] = ev.rollout(Z, integrator=0, X0=fix["X0"])
        for n_cols in (S.N_COLS,) + tuple(S.CASES[case].get("wide", ())):
            X0, B = (fix["X0"], fix["B"]) if n_cols == S.N_COLS else S.more_columns(case, n_cols, fix["X0"], fix["B"])
            got = _three(ev, Z, q, X0, B)
            out["runs"][n_cols] = dict(X0=X0, B=B, got=got)
        if "bits" in S.CASES[case]:
            X0, B = S.more_columns(case, n, fix["X0"], fix["B"])
            picks = (0, 48, n - 1)
            alone = {c: _three(ev, Z, q, X0[c:c + 1], B[:, c:c + 1]) for c in picks}
            out["bits"] = {}
            for n_cols in S.CASES[case]["bits"]:
                among = _three(ev, Z, q, X0[:n_cols], B[:, :n_cols])
                for c in picks:
                    if c < n_cols:
                        for quantity in S.QUANTITIES:
                            out["bits"][(n_cols, c, quantity)] = (not np.isnan(among[quantity]).any()
                                                                  and np.array_equal(among[quantity][:, c], alone[c][quantity][:, 0]))
        out["launches"] = {k: ev.profile_get(k)[1] for k in COUNTERS}
    finally:
        ev.close()
    bound = S.rho_bound(E)
    for n_cols, r in out["runs"].items():
        ex = S.exact(E, r["X0"], r["B"])
        rho = S.rho(E, r["X0"], r["B"], ex)
        r.update(exact=ex, rho=rho, bound=bound, errs_a=S.errors(r["got"], ex), bars_a={k: S.bar_a(v) for k, v in rho.items()})
        print(S.report(case, f"layer A, {n_cols} columns (error/bar per knot)", r["errs_a"], r["bars_a"],
                       f"rho={ {k: f'{v:.2e}' for k, v in rho.items()} } a-priori bound {bound:.2e}"))
    three = {k: v[:, :S.N_COLS] for k, v in fix.items() if k in S.QUANTITIES}
    for n_cols, r in out["runs"].items():
        r["errs_b"] = S.errors({k: v[:, :S.N_COLS] for k, v in r["got"].items()}, three)
        r["bars_b"] = {quantity: fix["bars"][i] for i, quantity in enumerate(S.QUANTITIES)}
        print(S.report(case, f"layer B, the fixture's columns among {n_cols} (error/bar per knot)", r["errs_b"], r["bars_b"]))
    return out


def _over(errs, bars):
    return [(quantity, t, float(e), float(np.broadcast_to(bars[quantity], errs[quantity].shape)[t]))
            for quantity in errs for t, e in enumerate(errs[quantity]) if not e <= np.broadcast_to(bars[quantity], errs[quantity].shape)[t]]


@pytest.mark.parametrize("case", NAMES)
def test_the_scan_alone_stays_within_16_rho_of_exact_arithmetic_on_its_own_propagators(case):
    out = run(case)
    assert set(out["runs"]) == {S.N_COLS} | set(S.CASES[case].get("wide", ()))
    for n_cols, r in out["runs"].items():
        for quantity, v in r["rho"].items():       # the yardstick is honest: under its a-priori bound
            assert v <= r["bound"], (case, n_cols, quantity, v, r["bound"])
        bad = _over(r["errs_a"], r["bars_a"])
        assert not bad, f"{case}, {n_cols} columns, layer A: over the bar (quantity, knot, error, bar): {bad}"
        assert np.array_equal(r["got"]["X"][0], r["X0"]) and np.array_equal(r["got"]["Y"][0], r["B"][0]) \
            and np.array_equal(r["got"]["Lam"][-1], r["B"][-1]), "the start knots are copies"


@pytest.mark.parametrize("case", NAMES)
def test_rollout_and_solves_stay_within_the_interval_budgets_of_the_320_bit_values(case):
    out = run(case)
    for n_cols, r in out["runs"].items():
        bad = _over(r["errs_b"], r["bars_b"])
        assert not bad, f"{case}, {n_cols} columns, layer B: over the bar (quantity, knot, error, bar): {bad}"


@pytest.mark.parametrize("case", BITS)
def test_ring_tree_columns_have_the_same_bits_alone_and_among_others(case):
    """49 columns and all n of them (the 64-column tile, dead columns in its last tile) against columns 0, 48 and n - 1 alone."""
    bits = run(case)["bits"]
    n = run(case)["E"].shape[1]
    assert set(bits) == {(n_cols, c, quantity) for n_cols in S.CASES[case]["bits"] for c in (0, 48, n - 1) if c < n_cols for quantity in S.QUANTITIES}
    assert all(bits.values()), sorted(k for k, v in bits.items() if not v)


@pytest.mark.parametrize("case", NAMES)
def test_each_case_ran_the_scans_and_the_kernel_it_is_there_for(case):
    out = run(case)
    L = out["launches"]
    print(case, L)
    assert L["rollout"] > 0 and L["rollout_tree"] > 0 and L["dynsolve"] > 0 and L["dynsolve_tree"] > 0, L
    n = out["E"].shape[1]
    if case == "tdbhp_kron":
        assert L["tdb_kron"] >= 1 and L["tdb_mfma"] == 0, L
    elif case in ("tdbhp_n72", "tdbhp_n128"):
        assert n > 64 and L["tdb_mfma"] >= 1 and L["tdb_kron"] == 0, L
    else:
        assert L["tdb_mfma"] == 0 and L["tdb_kron"] == 0, L


def test_follower_of_the_time_dependent_group_scans_its_own_blocks():
    """tdbhp_n72 as the group of two: integrator 1 (pre, x_off != 0).  Its E_k are cut from its own rows and its own x block;
    members share Phi, so those blocks and, with equal X0, the two members' rollouts are bit-equal."""
    out = run("tdbhp_n72")
    assert out["share"] == [(0, 2, 1), (0, 2, 1)], out["share"]
    assert out["leader_blocks_equal"]
    assert np.array_equal(out["leader_rollout"], out["runs"][S.N_COLS]["got"]["X"])
