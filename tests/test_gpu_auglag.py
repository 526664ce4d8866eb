"""GPU: the augmented-Lagrangian terms of the reduced-space stack (dto_auglag_rows / _merit / _gradient / _hessian_products /
_newton_step and their _dev forms; csrc/dto_auglag.hip, csrc/dto_auglag_plan.h).

References.  BITS: the rules of csrc/dto_auglag_plan.h restated in NumPy (auglag_cases.rows_restated, which test_auglag_plan_header.py
holds the header to) on the handle's own eval_constraint; reduced_lagrangian_gradient(mu_eff); the composition of public methods
auglag_cases.compose_product (J w, the scaling, J' w around reduced_cases' / reduced_input_cases' composition); newton_box_cases.box_loop
around that product -- equal, not close.  EQUIVALENCE: with rho = None the existing calls, bits and launch counts.  VALUES: the oracle's
dense Phi, gradient and Hr_AL (auglag_cases.dense_reference; test_auglag_reference.py judges it).  Outputs are pre-filled with NaN.

Shapes: 4 .. 299 non-dynamics rows (the lane loop of the sums wraps at 64), 60 .. 3900 entries (1 .. 16 chunks of the step's dots), both
"reduced_input_store" routes on al_12x9 and al_8x70.  The loop's product is the composition on the small cases and the engine's
auglag_hessian_product (held to the composition on two directions) on al_8x70 and al_8x300, where a composed product costs seconds."""
import functools

import numpy as np
import pytest

import auglag_cases as A
import dto_amd
import newton_box_cases as B
import reduced_cases as R
import reduced_input_cases as RI
from test_gpu_newton_step import PRODUCT_NAMES, REBUILD_NAMES, dense_bar, device_arrays, launches, run_id
from test_gpu_rollout import bar as rollout_bar
from test_newton_plan_header import CONVERGED, MAX_ITER

pytestmark = pytest.mark.gpu

SIGMA = A.SIGMA
RUNS = [(n, 0) for n in A.CASES] + [("al_12x9", 1), ("al_8x70", 1)]
COMPOSED_LOOP = ("al_12x9", "tdb_order1", "structured_16x4", "quadform_6x6")
KINDS = ("half_box", "indefinite_box", "max_iter_3")
EXISTING = ("hess_product", "reduced_pack", "reduced_input", "dynsolve_scan", "dynsolve_couple", "dynsolve_deriv", "jac_product", "expmv", "all",
            "bgemm", "chain64", "dynsolve_tree", "assembly", "rollout_tree", "rollout", "feasible", "newton", "newton_box")


def case_of(name):
    return A.case(name, dense=False) if name == "al_8x300" else A.case(name)


def evaluator(c, store):
    ev = dto_amd.Evaluator(c["pe"], **c["kw"])
    if store:
        ev.set_option("reduced_input_store", 1)
    return ev


def scenarios_of(name):
    sc = dict(A.scenarios(name))
    sc["max_iter_3"] = dict(sc["half_box"], max_iter=3)
    return sc


def engine_step(ev, c, kw, rho="case", mu="case"):
    x, info, tr, es, zp = ev.auglag_newton_step(c["Z"], SIGMA, c["mu"] if isinstance(mu, str) else mu, c["rho"] if isinstance(rho, str) else rho,
                                                trace=True, states=True, trajectory=True, **kw)
    return dict(p=x, info=info["raw"], trace=tr, states=es, Zp=zp, named=info)


def same_bits(got, want, what):
    assert not np.isnan(got["p"]).any() and not np.isnan(got["info"][:7]).any(), what
    for key in ("p", "info", "states", "Zp"):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert got["trace"].shape == want["trace"].shape and np.array_equal(got["trace"], want["trace"]), (what, "trace", got["trace"], want["trace"])


@functools.lru_cache(maxsize=None)
def results(name, store):
    """every run of one (case, route) on ONE handle, each beside its restatement: computed once, shared, never written"""
    import torch
    c = case_of(name)
    p, Z, mu, rho = c["p"], c["Z"], c["mu"], c["rho"]
    n, m, n_dyn = Z.size, c["n_cons"], c["n_dyn"]
    sc = scenarios_of(name)
    out = dict(c=c, sc=sc)
    ev = evaluator(c, store)
    try:
        # ---- the row pass
        g = np.full(m, np.nan)
        ev.eval_constraint(g, Z)
        out["g"] = g
        out["rows"] = ev.auglag_rows(Z, mu, rho)
        out["rows_mu_none"] = ev.auglag_rows(Z, None, rho)
        out["rows_rho_none"] = ev.auglag_rows(Z, mu, None)
        mu_eff, weight, _ = out["rows"]
        # ---- the merit
        out["merit"] = ev.auglag_merit(Z, SIGMA, mu, rho, trajectory=True, constraints=True, info=True)
        out["merit_bare"] = ev.auglag_merit(Z, SIGMA, mu, rho)
        out["feasible"] = ev.feasible_merit(Z, SIGMA, mu, trajectory=True, constraints=True)
        out["sf"] = ev.feasible_merit(Z, SIGMA, None)
        out["merit_rho_none"] = ev.auglag_merit(Z, SIGMA, mu, None, trajectory=True, constraints=True)
        out["merit_rho_zero"] = ev.auglag_merit(Z, SIGMA, mu, np.zeros(m), info=True)
        # ---- the gradient
        out["grad"] = ev.auglag_gradient(Z, SIGMA, mu, rho, costates=True, multipliers=True)
        out["grad_ref"] = ev.reduced_lagrangian_gradient(Z, SIGMA, mu_eff, costates=True)
        out["grad_rho_none"] = ev.auglag_gradient(Z, SIGMA, mu, None, multipliers=True)
        out["grad_plain"] = ev.reduced_lagrangian_gradient(Z, SIGMA, mu)
        out["grad_rho_zero"] = ev.auglag_gradient(Z, SIGMA, mu, np.zeros(m))
        # ---- products: two directions beside the composition, blocks of 1, 3 and 9 columns
        rng = np.random.default_rng(len(name))
        V = rng.standard_normal((9, n))
        out["V"] = V
        S = RI.store_from_jacobian(ev, p, Z) if store else None
        mut = R.compose_gradient(ev, p, Z, SIGMA, mu_eff)[2]
        composed = lambda v: A.compose_product(ev, p, Z, SIGMA, mu_eff, weight, v, S=S, mut=mut)
        out["composed"] = [composed(V[j]) for j in range(2)]
        out["singles"] = np.array([ev.auglag_hessian_product(Z, V[j], SIGMA, mu, rho) for j in range(9)])
        out["block3"] = ev.auglag_hessian_products(Z, V[:3], SIGMA, mu, rho)
        out["block9"] = ev.auglag_hessian_products(Z, V, SIGMA, mu, rho)
        out["plain9"] = ev.reduced_hessian_products(Z, V, SIGMA, mu)
        out["rho_none9"] = ev.auglag_hessian_products(Z, V, SIGMA, mu, None)
        out["rho_zero9"] = ev.auglag_hessian_products(Z, V, SIGMA, mu, np.zeros(m))
        out["at_mu_eff9"] = ev.reduced_hessian_products(Z, V, SIGMA, mu_eff)
        # ---- the step beside the NumPy loop
        product = composed if name in COMPOSED_LOOP else (lambda d: ev.auglag_hessian_product(Z, d, SIGMA, mu, rho))
        gradient = out["grad"][0]
        nonfixed = B.nonfixed_of(p)
        for kind in KINDS:
            out[kind] = (engine_step(ev, c, sc[kind]), B.box_loop(product, gradient, nonfixed, Z, **sc[kind]))
        out["box_plain"] = ev.reduced_newton_step_box(Z, SIGMA, mu, trace=True, states=True, trajectory=True, **sc["max_iter_3"])
        out["step_rho_none"] = engine_step(ev, c, sc["max_iter_3"], rho=None)
        out["step_rho_zero"] = engine_step(ev, c, sc["max_iter_3"], rho=np.zeros(m))
        if name in A.VALUE_CASES:
            tight = dict(sc["half_box"], rtol=1e-10)
            out["tight"] = engine_step(ev, c, tight)
        # ---- the other entry-point family, a repeated call and a call after a merit value elsewhere
        kw = sc["half_box"]
        (dZ, dmu, drho, dlo, dhi, dV), st = device_arrays(Z, mu, rho, kw["lo"], kw["hi"], V)
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dZ.device)
        dme, dw, di8, dphi, dZf, dg, dgr, dlam, dY = nan(m), nan(m), nan(8), nan(1), nan(n), nan(m), nan(n), nan(*out["grad"][1].shape), nan(9, n)
        dp, dinfo, dtrace, des, dzp = nan(n), nan(12), nan(kw["max_iter"], 6), nan(n), nan(n)
        P = lambda t: t.data_ptr()
        ev.auglag_rows_dev(P(dZ), P(dmu), P(drho), P(dme), P(dw), P(di8), stream=st)
        torch.cuda.synchronize()
        out["dev_rows"] = (dme.cpu().numpy(), dw.cpu().numpy(), di8.cpu().numpy())
        di8.fill_(float("nan"))
        ev.auglag_merit_dev(P(dZ), SIGMA, P(dmu), P(drho), P(dphi), P(dZf), P(dg), P(di8), stream=st)
        torch.cuda.synchronize()
        out["dev_merit"] = (float(dphi.cpu()[0]), dZf.cpu().numpy(), dg.cpu().numpy(), di8.cpu().numpy())
        dme.fill_(float("nan"))
        ev.auglag_gradient_dev(P(dZ), SIGMA, P(dmu), P(drho), P(dgr), P(dlam), P(dme), stream=st)
        ev.auglag_hessian_products_dev(P(dZ), SIGMA, P(dmu), P(drho), 9, P(dV), P(dY), stream=st)
        ev.auglag_newton_step_dev(P(dZ), SIGMA, P(dmu), P(drho), 0, P(dlo), P(dhi), 0.0, kw["shift"], kw["rtol"], 0.0, kw["max_iter"], P(dp),
                                  P(dinfo), P(dtrace), P(des), P(dzp), stream=st)
        torch.cuda.synchronize()
        out["dev_grad"] = (dgr.cpu().numpy(), dlam.cpu().numpy(), dme.cpu().numpy())
        out["dev_Y"] = dY.cpu().numpy()
        out["dev_step"] = dict(p=dp.cpu().numpy(), info=dinfo.cpu().numpy(), trace=dtrace.cpu().numpy(), states=des.cpu().numpy(),
                               Zp=dzp.cpu().numpy())
        out["again"] = engine_step(ev, c, kw)
        Z2 = np.array(Z)
        Z2[p.dt_idx] *= 1.25
        assert np.isfinite(ev.auglag_merit(Z2, SIGMA, mu, rho))
        out["after_merit"] = engine_step(ev, c, kw)
        out["after_merit_product"] = ev.auglag_hessian_product(Z, V[0], SIGMA, mu, rho)
    finally:
        ev.close()
    return out


# ------------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_row_pass_and_the_merit_are_the_restated_rules_bit_for_bit(run):
    s = results(*run)
    c = s["c"]
    n_dyn, is_eq, mu, rho = c["n_dyn"], c["is_eq"], c["mu"], c["rho"]
    for key, m_, r_ in (("rows", mu, rho), ("rows_mu_none", np.zeros(mu.size), rho), ("rows_rho_none", mu, np.zeros(rho.size))):
        mu_eff, weight, info = s[key]
        psi, mult, w, viol = A.rows_restated(is_eq, s["g"][n_dyn:], m_[n_dyn:], r_[n_dyn:])
        assert np.array_equal(mu_eff, A.full(n_dyn, mult)) and np.array_equal(weight, A.full(n_dyn, w)), key
        want = A.info_restated(is_eq, s["g"][n_dyn:], m_[n_dyn:], r_[n_dyn:])
        assert np.array_equal(info["raw"], want), (key, info["raw"], want)
    info = s["rows"][2]
    print(run_id(run), "rows", is_eq.size, "active", info["active"], "max viol", info["max_viol"], "P", info["P"])
    assert 0 < info["active"] < is_eq.size and info["penalised"] == is_eq.size and s["rows_rho_none"][2]["penalised"] == 0
    # the merit: Zf and g are feasible_merit's, Phi = sigma f + P with P in the stated order over g(Zf)
    phi, Zf, g, minfo = s["merit"]
    phi_f, Zf_f, g_f = s["feasible"]
    assert np.array_equal(Zf, Zf_f) and np.array_equal(g, g_f)
    want = A.info_restated(is_eq, g[n_dyn:], mu[n_dyn:], rho[n_dyn:])
    assert np.array_equal(minfo["raw"], want) and phi == s["sf"] + want[0], (phi, s["sf"], want[0])
    assert s["merit_bare"] == phi and phi != phi_f, "the optional outputs change nothing; the penalty takes part"
    assert np.array_equal(s["dev_rows"][0], s["rows"][0]) and np.array_equal(s["dev_rows"][1], s["rows"][1])
    assert np.array_equal(s["dev_rows"][2], s["rows"][2]["raw"])
    assert s["dev_merit"][0] == phi and np.array_equal(s["dev_merit"][1], Zf) and np.array_equal(s["dev_merit"][2], g)
    assert np.array_equal(s["dev_merit"][3], minfo["raw"])


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_gradient_is_the_reduced_gradient_at_mu_eff_bit_for_bit(run):
    s = results(*run)
    grad, lam, mu_eff = s["grad"]
    assert not np.isnan(grad).any()
    assert np.array_equal(grad, s["grad_ref"][0]) and np.array_equal(lam, s["grad_ref"][1]) and np.array_equal(mu_eff, s["rows"][0])
    assert not np.array_equal(grad, s["grad_plain"]), "the penalty takes part"
    for got, want in zip(s["dev_grad"], s["grad"]):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_a_product_is_the_composition_of_public_methods_bit_for_bit(run):
    s = results(*run)
    for j, want in enumerate(s["composed"]):
        got = s["singles"][j]
        print(run_id(run), "entries that differ", int(np.sum(got != want)), "largest", float(np.max(np.abs(got - want))))
        assert not np.isnan(got).any() and np.array_equal(got, want)
    assert not np.array_equal(s["singles"], s["at_mu_eff9"]), "the Gauss-Newton term takes part"
    assert np.array_equal(s["after_merit_product"], s["singles"][0])


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_every_column_of_a_block_has_the_single_calls_bits(run):
    s = results(*run)
    assert np.array_equal(s["block3"], s["singles"][:3]) and np.array_equal(s["block9"], s["singles"]) and np.array_equal(s["dev_Y"], s["singles"])


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_step_is_the_numpy_loop_bit_for_bit(run):
    s = results(*run)
    for kind in KINDS:
        got, want = s[kind]
        i = got["named"]
        print(run_id(run), kind, "status", i["status"], "iterations", i["iterations"], "held", i["held"], "hit", i["hit"], "restarts", i["restarts"],
              "|F|", i["n_free"], "|r|/|g|", i["rnorm"] / i["gnorm"])
        same_bits(got, want, kind)
    assert s["max_iter_3"][0]["named"]["status"] == MAX_ITER and s["max_iter_3"][0]["named"]["iterations"] == 3
    assert s["half_box"][0]["named"]["hit"] >= 1


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_both_families_a_repeated_call_and_a_call_after_a_merit_value_return_the_same_bits(run):
    s = results(*run)
    first = s["half_box"][0]
    k = first["named"]["iterations"]
    dev = s["dev_step"]
    for key in ("p", "info", "states", "Zp"):
        assert np.array_equal(dev[key], first[key]), key
    assert np.array_equal(dev["trace"][:k], first["trace"]) and np.isnan(dev["trace"][k:]).all(), "rows past the last iteration stay NaN"
    for form in ("again", "after_merit"):
        same_bits(s[form], first, form)


# ----------------------------------------------------------------------------------------------------------- equivalence
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_without_penalties_every_call_is_the_call_it_extends(run):
    s = results(*run)
    c = s["c"]
    n_dyn = c["n_dyn"]
    phi_f, Zf_f, g_f = s["feasible"]
    # rho = None: the bits
    phi, Zf, g = s["merit_rho_none"]
    assert phi == phi_f and np.array_equal(Zf, Zf_f) and np.array_equal(g, g_f)
    grad, mu_eff = s["grad_rho_none"]
    assert np.array_equal(grad, s["grad_plain"]) and np.array_equal(mu_eff, A.full(n_dyn, c["mu"][n_dyn:]))
    assert np.array_equal(s["rho_none9"], s["plain9"])
    x, info, tr, es, zp = s["box_plain"]
    same_bits(s["step_rho_none"], dict(p=x, info=info["raw"], trace=tr, states=es, Zp=zp), "rho = None")
    # rho = 0 on every row: equal values
    phi0, info0 = s["merit_rho_zero"]
    assert phi0 == phi_f and info0["penalised"] == 0 and info0["active"] == 0
    assert np.array_equal(s["grad_rho_zero"], s["grad_plain"])
    assert np.array_equal(s["rho_zero9"], s["plain9"])
    same_bits(s["step_rho_zero"], s["step_rho_none"], "rho = 0")


@pytest.mark.parametrize("run", [("al_12x70", 1), ("al_12x70", 0), ("quadform_6x6", 0)], ids=run_id)
def test_launch_counts(run):
    """rho = None: the launch counts of the existing calls under every existing name, none under "auglag".  With penalties: a 9-column
    chunk counts what a 1-column chunk counts under "auglag" where every constraint is a norm or a squared norm without repeats; a
    step of k iterations at a kept point counts k times one product's launches and no chain, tree-build, assembly or sweep launch."""
    name, store = run
    # al_12x70: a norm and a squared-norm constraint without repeats, and 12 states, so that nine columns are ONE chunk (the solves'
    # column limit is the smallest state dimension); no dense matrix is needed here
    c = A.case(name, dense=False) if name == "al_12x70" else case_of(name)
    Z, mu, rho = c["Z"], c["mu"], c["rho"]
    V = np.random.default_rng(1).standard_normal((9, Z.size))
    if name == "al_12x70":
        lo, hi = B.loop_box(Z, R.index_sets(c["p"])[1], 1.0)
        kw = dict(lo=lo, hi=hi, max_iter=4, rtol=1e-12)
    else:
        kw = scenarios_of(name)["half_box"]
    ev = evaluator(c, store)
    try:
        ev.profile_enable(True)

        def counted(call, names=EXISTING + ("auglag",)):
            ev.profile_reset()
            call()
            return launches(ev, names)

        pairs = ((lambda: ev.feasible_merit(Z, SIGMA, mu), lambda: ev.auglag_merit(Z, SIGMA, mu, None)),
                 (lambda: ev.reduced_lagrangian_gradient(Z, SIGMA, mu), lambda: ev.auglag_gradient(Z, SIGMA, mu, None)),
                 (lambda: ev.reduced_hessian_products(Z, V, SIGMA, mu), lambda: ev.auglag_hessian_products(Z, V, SIGMA, mu, None)),
                 (lambda: ev.reduced_newton_step_box(Z, SIGMA, mu, **kw), lambda: ev.auglag_newton_step(Z, SIGMA, mu, None, **kw)))
        for old, new in pairs:
            old()                                   # both counted at the kept points the first call leaves
            a, b = counted(old), counted(new)
            assert a == b and b[-1] == 0, (a, b)
        # with penalties
        ev.auglag_hessian_products(Z, V[:1], SIGMA, mu, rho)
        one = counted(lambda: ev.auglag_hessian_products(Z, V[:1], SIGMA, mu, rho))
        nine = counted(lambda: ev.auglag_hessian_products(Z, V, SIGMA, mu, rho))
        at = lambda counts, key: dict(zip(EXISTING + ("auglag",), counts))[key]
        n_al, chunks = at(one, "auglag"), at(nine, "hess_product") // at(one, "hess_product")
        print(run_id(run), "auglag launches: 1 column", n_al, "9 columns", nine[-1], "in", chunks, "chunk(s); bytes", ev.profile_get("auglag")[2])
        assert n_al >= 3 and ev.profile_get("auglag")[2] > 0, "the row pass, a constraint's launch, the addition; bytes as executed"
        if name.startswith("al_"):
            assert nine[-1] == 1 + chunks * (n_al - 1), "per chunk what a 1-column chunk counts: no launch per column"
            assert chunks == 1 and nine[-1] == n_al, "a 9-column chunk counts what a 1-column chunk counts"
        else:
            assert nine[-1] > 1 + chunks * (n_al - 1), "the quadratic form goes through the single-column launchers"
        rebuild = dict(zip(EXISTING, one))
        assert all(rebuild[k] == 0 for k in REBUILD_NAMES), "a second call at the same (Z, sigma, mu, rho) rebuilds nothing"
        product_one = tuple(dict(zip(EXISTING + ("auglag",), one))[k] for k in PRODUCT_NAMES)
        ev.profile_reset()
        x, info = ev.auglag_newton_step(Z, SIGMA, mu, rho, **kw)
        k = info["iterations"]
        assert k >= 2
        assert launches(ev, PRODUCT_NAMES) == tuple(k * v for v in product_one), "k kept-point single products"
        assert launches(ev, REBUILD_NAMES) == (0,) * len(REBUILD_NAMES), "no chain, tree-build, assembly or rollout launch"
        assert launches(ev, ("auglag", "newton_box", "newton")) == (1 + k * (n_al - 1), 2 + 3 * k, 0), "one row pass per call"
        ev.profile_enable(False)
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", A.VALUE_CASES)
def test_values_against_the_oracle(name):
    """gradient: reduced_cases.gradient_bar; products: reduced_cases.product_bar with ||H_AL||; the step on its final face:
    test_gpu_newton_box.py's bar; Phi: the trajectory's bar of test_gpu_feasible.py (levels x test_gpu_rollout.bar(K) per entry, relative
    to max(1, |Zf_i|)) carried to Phi through its gradient, |dPhi| <= sum |dPhi/dZ_i| bar max(1, |Zf_i|), plus the values' own 1e-10 |Phi|.
    Each ratio to its bar is printed; DESIGN 4.34 records the largest."""
    s, c = results(name, 0), A.case(name)
    ref, Cidx, p = c["ref"], c["ref"]["C"], c["p"]
    err, b = float(np.linalg.norm(s["grad"][0] - ref["r_ref"])), R.gradient_bar(ref, c["levels"])
    print(name, "gradient: error", err, "bar", b, "ratio", err / b)
    assert err <= b
    for j in range(2):
        v = s["V"][j]
        err, b = float(np.linalg.norm(s["singles"][j] - R.product_ref(ref, v))), R.product_bar(ref, v)
        print(name, "product", j, "error", err, "bar", b, "ratio", err / b)
        assert err <= b
    phi = s["merit"][0]
    phi_o = A.phi_ref(p, c["Z"], SIGMA, c["mu"], c["rho"])
    b = c["levels"] * rollout_bar(p.N - 1) * float(np.abs(ref["g"]) @ np.maximum(1.0, np.abs(c["Z"]))) + 1e-10 * abs(phi_o)
    print(name, "Phi", phi, "oracle", phi_o, "error", abs(phi - phi_o), "bar", b, "ratio", abs(phi - phi_o) / b)
    assert abs(phi - phi_o) <= b
    # the step on the final face
    kw = dict(s["sc"]["half_box"], rtol=1e-10)
    got = s["tight"]
    want = B.box_loop(lambda d: R.product_ref(ref, d), np.array(ref["r_ref"]), B.nonfixed_of(p), c["Z"], **kw)
    assert got["named"]["status"] == CONVERGED and int(want["info"][0]) == CONVERGED
    assert np.array_equal(got["states"], want["states"]), "the engine ends on the oracle's face"
    es, x = got["states"][Cidx], got["p"][Cidx]
    F, Bd = es == B.FREE, es >= B.HIT_LO
    Am = ref["Hr"] + s["sc"]["shift"] * np.eye(Cidx.size)
    gC = ref["r_ref"][Cidx]
    pF = np.linalg.solve(Am[np.ix_(F, F)], -(gC[F] + Am[np.ix_(F, Bd)] @ x[Bd]))
    err = float(np.linalg.norm(x[F] - pF))
    b = dense_bar(ref, c["levels"], 1e-10, Am[np.ix_(F, F)], got["p"], got["named"]["gnorm"])
    print(name, "face: free", int(F.sum()), "hit", int(Bd.sum()), "||p_F - p_F*||", err, "bar", b, "ratio", err / b)
    assert err <= b


# ------------------------------------------------------------------------------------------------------------ the outer loop
def test_the_outer_loop_follows_the_oracles_run():
    """The README's outer loop on al_12x9 with the engine: the accept and reject decisions and the rho increases of the oracle's run
    (test_auglag_reference.py holds that run to its bar), max viol behind every outer iteration within a factor of 2 of the oracle's.
    Both runs are one algorithm and differ by rounding unless a decision flips: the factor is a loose margin, nothing was measured to
    set it."""
    c = A.case("al_12x9", dense=False)
    want = A.oracle_outer_run("al_12x9")
    ev = evaluator(c, 0)
    try:
        def step(Z, delta, mu, rho):
            x, info, Zp = ev.auglag_newton_step(Z, SIGMA, mu, rho, radius=delta, trajectory=True, **A.STEP_KW)
            return info["predicted"], info["status"], Zp

        def merit(Zp, mu, rho):
            return ev.auglag_merit(Zp, SIGMA, mu, rho, trajectory=True)

        def rows(Z, mu, rho):
            mu_eff, _, info = ev.auglag_rows(Z, mu, rho)
            return mu_eff, info["max_viol"]

        got = A.outer_loop(step, merit, rows, c["Z"], c["n_dyn"], c["n_cons"] - c["n_dyn"])
    finally:
        ev.close()
    print("engine: max viol", got["viol0"], got["viol"], "rho grew", got["grew"])
    print("oracle: max viol", want["viol0"], want["viol"], "rho grew", want["grew"])
    print("engine accepted", got["accepted"])
    print("oracle accepted", want["accepted"])
    assert got["accepted"] == want["accepted"] and got["grew"] == want["grew"]
    for a, b in zip(got["viol"], want["viol"]):
        assert b / 2.0 <= a <= 2.0 * b, (a, b)
    assert got["viol0"] >= 0.1 and got["viol"][-1] < 1e-4


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_device_handle_leave_nothing_written_and_the_handle_usable():
    c = A.case("al_12x9")
    Z, mu, rho = c["Z"], c["mu"], c["rho"]
    ev = dto_amd.Evaluator(c["pe"], k_lo=1, k_hi=3)                # a sharded handle: what the extended calls refuse
    try:
        for call, who in ((lambda: ev.auglag_rows(Z, mu, rho), "dto_auglag_rows"), (lambda: ev.auglag_merit(Z, SIGMA, mu, rho), "dto_auglag_merit"),
                          (lambda: ev.auglag_gradient(Z, SIGMA, mu, rho), "dto_auglag_gradient"),
                          (lambda: ev.auglag_newton_step(Z, SIGMA, mu, rho), "dto_auglag_newton_step")):
            with pytest.raises(dto_amd.EngineError, match=who + ".* unsharded handle"):
                call()
    finally:
        ev.close()
    ev = evaluator(c, 0)
    try:
        ev.profile_enable(True)
        bad = np.array(rho)
        bad[c["n_dyn"] + 1] = -2.0
        with pytest.raises(dto_amd.EngineError, match=rf"rho\[{c['n_dyn'] + 1}\]"):
            ev.auglag_newton_step(Z, SIGMA, mu, bad)
        with pytest.raises(dto_amd.EngineError, match="max_iter"):
            ev.auglag_newton_step(Z, SIGMA, mu, rho, max_iter=0)
        assert ev.profile_get("auglag")[1] == 0 and ev.profile_get("all")[1] == 0, "nothing was enqueued"
        ev.profile_enable(False)
        s = results("al_12x9", 0)
        same_bits(engine_step(ev, c, s["sc"]["half_box"]), s["half_box"][0], "after the refusals")
    finally:
        ev.close()
