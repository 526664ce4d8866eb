"""GPU: the L-BFGS-preconditioned truncated-Newton step (dto_preconditioned_newton_step, dto_newton_precondition, dto_newton_pairs_* and
their _dev forms, csrc/dto_precond.hip, csrc/dto_precond_plan.h).

References.  BITS: csrc/dto_precond_plan.h restated in NumPy (precond_cases.py, which test_precond_plan_header.py holds the plain-C++
header to) around the same handle's reduced_hessian_product (auglag_hessian_product with rho) and gradient -- p, info, trace,
entry_state and Zp must be equal, not close.  EQUIVALENCE: with an empty store, reduced_newton_step_box and auglag_newton_step on the
same handle.  VALUES: the oracle's dense reduced Hessian and gradient.  Outputs are pre-filled with NaN.

The store cannot be read back, so what a harvest left is judged through dto_newton_precondition on random vectors and through the next
step, both of which must have the bits of the restatement run with the restated loop's own (d, w).

Shapes: those of test_gpu_newton_box.py -- 41 .. 250 entries (1 - 2 chunks) and 40 x 258 (11610 entries: 46 chunks, the last ragged);
both "reduced_input_store" routes on scaled_40x6 and on the long case."""
import functools

import numpy as np
import pytest

import auglag_cases as A
import dto_amd
import dto_oracle as O
import newton_box_cases as B
import precond_cases as PC
import reduced_cases as R
from test_gpu_newton_box import KINDS, LONG, RUNS, SMALL, scenarios_of
from test_gpu_newton_step import PRODUCT_NAMES, REBUILD_NAMES, dense_bar, device_arrays, evaluator, launches, problem_of, run_id
from test_newton_plan_header import CONVERGED, MAX_ITER

pytestmark = pytest.mark.gpu

SIGMA = R.SIGMA
M = 8


def engine_step(ev, c, kw, harvest=False, rho=None):
    x, info, tr, es, zp = ev.preconditioned_newton_step(c["Z"], SIGMA, c["mu"], rho, trace=True, states=True, trajectory=True, harvest=harvest, **kw)
    return dict(p=x, info=info["raw"], trace=tr, states=es, Zp=zp, named=info)


def box_step(ev, c, kw):
    x, info, tr, es, zp = ev.reduced_newton_step_box(c["Z"], SIGMA, c["mu"], trace=True, states=True, trajectory=True, **kw)
    return dict(p=x, info=info["raw"], trace=tr, states=es, Zp=zp)


def numpy_step(ev, c, kw, store, harvest=False):
    Z, mu = c["Z"], c["mu"]
    return PC.precond_loop(lambda d: ev.reduced_hessian_product(Z, d, SIGMA, mu), ev.reduced_lagrangian_gradient(Z, SIGMA, mu), B.nonfixed_of(c["p"]),
                           Z, store.S, store.Y, harvest=harvest, **kw)


def same_bits(got, want, what, upto=None):
    assert not np.isnan(got["p"]).any() and not np.isnan(got["info"][:7]).any(), what
    for key in ("p", "states", "Zp"):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert np.array_equal(got["info"][:upto], want["info"][:upto]), (what, "info", got["info"], want["info"])
    cols = 6 if upto else 8
    assert got["trace"].shape[0] == want["trace"].shape[0] and np.array_equal(got["trace"][:, :cols], want["trace"][:, :cols]), (what, "trace")


@functools.lru_cache(maxsize=None)
def steps(name, store_route):
    """every run of one (case, route) on ONE handle, each beside its restatement: computed once, shared, never written"""
    import torch
    c = problem_of(name)
    Z, mu = c["Z"], c["mu"]
    n = Z.size
    sc = scenarios_of(name)
    out = dict(c=c, sc=sc)
    ev = evaluator(c, store_route)
    try:
        ev.set_option("newton_pairs", M)
        out["info_empty"] = ev.newton_pairs_info()
        # ---- an empty store: the box step
        for kind in KINDS:
            out["empty", kind] = (engine_step(ev, c, sc[kind]), box_step(ev, c, sc[kind]))
        # ---- a harvest from the empty store, beside the restated loop
        store = PC.Store(M)
        want = numpy_step(ev, c, sc["inf"], store, harvest=True)
        out["harvest"] = (engine_step(ev, c, sc["inf"], harvest=True), want)
        store.harvested(want["pairs"])
        out["info_harvested"] = ev.newton_pairs_info()
        out["store_count"] = store.count
        rng = np.random.default_rng(11)
        Rv = rng.standard_normal((5, n))
        out["applied"] = (ev.newton_precondition(Rv), PC.precondition_restated(store.S, store.Y, Rv, B.nonfixed_of(c["p"])))
        # ---- with the harvested pairs: every scenario beside the restated loop; the last one harvests again (the other bank)
        for kind in KINDS:
            again = kind == KINDS[-1]
            want = numpy_step(ev, c, sc[kind], store, harvest=again)
            out["harvested", kind] = (engine_step(ev, c, sc[kind], harvest=again), want)
            if again:
                store.harvested(want["pairs"])
        out["info_second"] = (ev.newton_pairs_info(), store.count)
        out["applied_second"] = (ev.newton_precondition(Rv[0]), PC.precondition_restated(store.S, store.Y, Rv[0], B.nonfixed_of(c["p"])))
        # ---- the same pairs pushed: host family, then the device family; a repeated call; a call after a merit value at another Z
        kw = sc["half_box"]
        first = numpy_step(ev, c, kw, store)
        out["want_half_box"] = first
        pairs = list(zip(store.S, store.Y))
        ev.newton_pairs_clear()
        out["info_cleared"] = ev.newton_pairs_info()
        for s, y in pairs:
            ev.newton_pairs_push(s, y)
        out["pushed"] = engine_step(ev, c, kw)
        out["again"] = engine_step(ev, c, kw)
        Z2 = np.array(Z)
        Z2[c["p"].dt_idx] *= 1.25
        assert np.isfinite(ev.feasible_merit(Z2, SIGMA, mu))
        out["after_merit"] = engine_step(ev, c, kw)
        x_bare, info_bare = ev.preconditioned_newton_step(Z, SIGMA, mu, **kw)
        out["bare"] = (x_bare, info_bare["raw"])
        ev.newton_pairs_clear()
        (dZ, dlo, dhi), st = device_arrays(Z, kw["lo"], kw["hi"])
        dmu = 0 if mu is None else device_arrays(mu)[0][0]
        for s, y in pairs:
            (ds, dy), _ = device_arrays(s, y)
            ev.newton_pairs_push_dev(ds.data_ptr(), dy.data_ptr(), stream=st)
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dZ.device)
        dp, dinfo, dtrace, des, dzp = nan(n), nan(16), nan(kw["max_iter"], 8), nan(n), nan(n)
        ev.preconditioned_newton_step_dev(dZ.data_ptr(), SIGMA, 0 if mu is None else dmu.data_ptr(), 0, 0, dlo.data_ptr(), dhi.data_ptr(), 0.0,
                                          kw["shift"], kw["rtol"], 0.0, kw["max_iter"], False, dp.data_ptr(), dinfo.data_ptr(), dtrace.data_ptr(),
                                          des.data_ptr(), dzp.data_ptr(), stream=st)
        torch.cuda.synchronize()
        out["dev"] = dict(p=dp.cpu().numpy(), info=dinfo.cpu().numpy(), trace=dtrace.cpu().numpy(), states=des.cpu().numpy(), Zp=dzp.cpu().numpy())
        if name != LONG:
            tight = {k: dict(sc[k], rtol=1e-10) for k in B.CONVEX}
            out["tight"] = {k: engine_step(ev, c, tight[k]) for k in B.CONVEX}
    finally:
        ev.close()
    return out


# ------------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_with_an_empty_store_the_step_is_the_box_step_bit_for_bit(run):
    s = steps(*run)
    assert s["info_empty"] == (0, M)
    for kind in KINDS:
        got, box = s["empty", kind]
        same_bits(got, box, kind, upto=12)
        k = got["named"]["iterations"]
        assert np.array_equal(got["trace"][:k, 6], got["trace"][:k, 3]) and np.all(got["trace"][:k, 7] == 0.0), "rz = rr bit for bit"
        assert np.array_equal(got["info"][12:15], [0.0, 0.0, 0.0]) and got["info"][15] == got["info"][2]


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_step_is_the_numpy_loop_bit_for_bit(run):
    s = steps(*run)
    got, want = s["harvest"]
    same_bits(got, want, "harvest from an empty store")
    for kind in KINDS:
        got, want = s["harvested", kind]
        i = got["named"]
        print(run_id(run), kind, "status", i["status"], "iterations", i["iterations"], "box iterations", int(s["empty", kind][0]["info"][1]), "admitted",
              i["admitted"], "harvested", i["harvested"], "fallbacks", i["fallbacks"], "hit", i["hit"], "restarts", i["restarts"])
        same_bits(got, want, kind)
        assert 1 <= i["admitted"] <= s["store_count"] and i["fallbacks"] == 0
    assert s["harvested", "inf"][0]["named"]["admitted"] == s["store_count"], "at the harvest's own F0 every pair is admitted"
    assert s["harvested", "max_iter_3"][0]["named"]["status"] == MAX_ITER and s["harvested", "max_iter_3"][0]["named"]["harvested"] == 3
    assert s["harvested", "half_box"][0]["named"]["hit"] >= 3 and s["harvested", "held"][0]["named"]["held"] == 4


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_a_harvest_leaves_the_loops_pairs(run):
    s = steps(*run)
    taken = len(s["harvest"][1]["pairs"])
    assert taken >= 2 and s["harvest"][0]["info"][13] == taken and s["info_harvested"] == (min(M, taken), M) and s["store_count"] == min(M, taken)
    got, want = s["applied"]
    assert got.shape == want.shape and np.array_equal(got, want), "five columns through the harvested store"
    assert s["info_second"][0] == (s["info_second"][1], M) and s["info_second"][1] == 3, "the second harvest took three pairs into the other bank"
    assert np.array_equal(*s["applied_second"])
    assert s["info_cleared"] == (0, M)


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_pushed_pairs_both_families_a_repeated_call_and_a_call_after_a_merit_value_return_the_same_bits(run):
    s = steps(*run)
    want = s["want_half_box"]
    same_bits(s["pushed"], want, "pushed")
    for form in ("again", "after_merit"):
        same_bits(s[form], want, form)
    assert np.array_equal(s["bare"][0], want["p"]) and np.array_equal(s["bare"][1], want["info"]), "the optional outputs change nothing"
    dev, k = s["dev"], int(want["info"][1])
    for key in ("p", "info", "states", "Zp"):
        assert np.array_equal(dev[key], want[key]), key
    assert np.array_equal(dev["trace"][:k], want["trace"]) and np.isnan(dev["trace"][k:]).all(), "rows past the last iteration stay NaN"


# --------------------------------------------------------------------------------------------------------- the application
def random_pairs(n, count, seed, bad=()):
    """pairs with positive curvature entry by entry (y = w .* s, w in 0.5 .. 2); the pairs in `bad` have y negated"""
    rng = np.random.default_rng(seed)
    S = [rng.standard_normal(n) for _ in range(count)]
    Y = [(-1.0 if k in bad else 1.0) * rng.uniform(0.5, 2.0, n) * s for k, s in enumerate(S)]
    return S, Y


@pytest.mark.parametrize("run", [("scaled_40x6", 0), (LONG, 1)], ids=run_id)
def test_newton_precondition_is_the_restatement_bit_for_bit(run):
    """m = 1, 3, 8, 16, a wrapped ring (m + 3 pushes), a rejected pair in the middle, all pairs rejected, a free mask, 1 and 5 columns,
    both entry-point families"""
    import torch
    name, store_route = run
    c = problem_of(name)
    n = c["Z"].size
    nonfixed = B.nonfixed_of(c["p"])
    rng = np.random.default_rng(3)
    Rv = rng.standard_normal((5, n))
    mask = (rng.random(n) < 0.7).astype(np.float64)
    ev = evaluator(c, store_route)
    try:
        for m, pushes, bad in ((1, 1, ()), (3, 3, ()), (8, 8, ()), (16, 16, ()), (8, 11, ()), (3, 6, ()), (8, 5, (2,)), (8, 4, (0, 1, 2, 3)), (8, 0, ())):
            ev.set_option("newton_pairs", m)
            S, Y = random_pairs(n, pushes, 100 * m + pushes, bad)
            store = PC.Store(m)
            for s, y in zip(S, Y):
                ev.newton_pairs_push(s, y)
                store.push(s, y)
            assert ev.newton_pairs_info() == (store.count, m) and store.count == min(m, pushes)
            P = PC.prepare_restated(store.S, store.Y, nonfixed)
            print(run_id(run), "m", m, "pushes", pushes, "admitted", len(P["idx"]), "gamma", P["gamma"])
            assert len(P["idx"]) == store.count - len([k for k in bad if k >= pushes - store.count])
            got5 = ev.newton_precondition(Rv)
            assert np.array_equal(got5, PC.precondition_restated(store.S, store.Y, Rv, nonfixed)), (m, pushes, "five columns")
            assert np.array_equal(ev.newton_precondition(Rv[3]), got5[3]), "column c is the single application"
            assert np.all(got5[:, ~nonfixed] == 0.0)
            if not store.count or len(bad) == pushes:
                assert np.array_equal(got5, np.where(nonfixed, Rv, 0.0)), "no admitted pair: the identity on the free entries"
            free = nonfixed & (mask != 0.0)
            assert np.array_equal(ev.newton_precondition(Rv[:2], free=mask), PC.precondition_restated(store.S, store.Y, Rv[:2], free)), (m, "mask")
            (dR, dmask), st = device_arrays(Rv, mask)
            dz = torch.full((5, n), float("nan"), dtype=torch.float64, device=dR.device)
            ev.newton_precondition_dev(0, 5, dR.data_ptr(), dz.data_ptr(), stream=st)
            torch.cuda.synchronize()
            assert np.array_equal(dz.cpu().numpy(), got5), "the device family"
            ev.newton_precondition_dev(dmask.data_ptr(), 1, dR.data_ptr(), dz.data_ptr(), stream=st)
            torch.cuda.synchronize()
            assert np.array_equal(dz.cpu().numpy()[0], PC.precondition_restated(store.S, store.Y, Rv[0], free))
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------- the augmented Lagrangian
def test_with_rho_it_is_the_auglag_step():
    """an empty store: dto_auglag_newton_step bit for bit; with harvested pairs: the restated loop around auglag_hessian_product"""
    name = "al_12x9"
    c = A.case(name)
    Z, mu, rho = c["Z"], c["mu"], c["rho"]
    kw = dict(A.scenarios(name)["half_box"])
    ev = dto_amd.Evaluator(c["pe"], **c["kw"])
    try:
        ev.set_option("newton_pairs", M)
        x, info, tr, es, zp = ev.auglag_newton_step(Z, SIGMA, mu, rho, trace=True, states=True, trajectory=True, **kw)
        got = engine_step(ev, c, kw, harvest=True, rho=rho)
        same_bits(got, dict(p=x, info=info["raw"], trace=tr, states=es, Zp=zp), "empty store, rho", upto=12)
        product = lambda d: ev.auglag_hessian_product(Z, d, SIGMA, mu, rho)
        gradient, nonfixed = ev.auglag_gradient(Z, SIGMA, mu, rho), B.nonfixed_of(c["p"])
        store = PC.Store(M)
        first = PC.precond_loop(product, gradient, nonfixed, Z, harvest=True, **kw)
        same_bits(got, first, "the harvesting call")
        store.harvested(first["pairs"])
        assert ev.newton_pairs_info() == (store.count, M) and store.count >= 2
        second = engine_step(ev, c, kw, rho=rho)
        same_bits(second, PC.precond_loop(product, gradient, nonfixed, Z, store.S, store.Y, **kw), "harvested pairs, rho")
        print("al_12x9 half_box: iterations", got["named"]["iterations"], "->", second["named"]["iterations"], "admitted", second["named"]["admitted"])
        same_bits(engine_step(ev, c, kw, rho=None), PC.precond_loop(lambda d: ev.reduced_hessian_product(Z, d, SIGMA, mu),
                                                                    ev.reduced_lagrangian_gradient(Z, SIGMA, mu), nonfixed, Z, store.S, store.Y, **kw),
                  "rho = None dispatches to the box operator")
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("kind", B.CONVEX)
def test_values_against_the_oracle(name, kind):
    """On the final face ||p_F - solve(A_FF, -(g_F + A_FB p_B))|| <= (2 rtol ||g|| + gradient_bar + product_bar(p)) / lambda_min(A_FF): the bar of
    test_gpu_newton_box.test_values_against_the_oracle; the convergence test is the Euclidean one there and here."""
    s, c = steps(name, 0), R.case(name)
    ref, Cidx = c["ref"], c["ref"]["C"]
    got = s["tight"][kind]
    assert got["named"]["status"] == CONVERGED and got["named"]["admitted"] >= 1
    es, x = got["states"][Cidx], got["p"][Cidx]
    F, Bd = es == B.FREE, es >= B.HIT_LO
    Aref = ref["Hr"] + s["sc"]["shift"] * np.eye(Cidx.size)
    g = ref["r_ref"][Cidx]
    pF = np.linalg.solve(Aref[np.ix_(F, F)], -(g[F] + Aref[np.ix_(F, Bd)] @ x[Bd]))
    err = float(np.linalg.norm(x[F] - pF))
    b = dense_bar(ref, c["levels"], 1e-10, Aref[np.ix_(F, F)], got["p"], got["named"]["gnorm"])
    print(name, kind, "iterations", got["named"]["iterations"], "face: free", int(F.sum()), "hit", int(Bd.sum()), "||p_F - p_F*||", err, "bar", b,
          "ratio", err / b)
    assert err <= b
    kw = s["sc"][kind]
    assert np.all(got["Zp"][Cidx] >= kw["lo"][Cidx]) and np.all(got["Zp"][Cidx] <= kw["hi"][Cidx]), "inside the box, exactly"


@pytest.mark.parametrize("name", ["scaled_12x9", "scaled_40x6"])
def test_harvested_pairs_save_iterations_at_the_same_point(name):
    s = steps(name, 0)
    plain, pre = s["harvest"][0]["named"], s["harvested", "inf"][0]["named"]
    print(name, "plain", plain["iterations"], "with the harvested pairs", pre["iterations"], "admitted", pre["admitted"])
    assert plain["status"] == pre["status"] == CONVERGED and pre["admitted"] == M
    assert pre["iterations"] < plain["iterations"], "strictly fewer iterations"


# --------------------------------------------------------------------------------------------------- kept points, launches
@pytest.mark.parametrize("run", [("scaled_40x6", 1), ("scaled_40x6", 0)], ids=run_id)
def test_a_step_is_k_kept_point_products_and_the_precond_launches(run):
    """per call: the start, the first combination and the first direction, and with pairs the Gram pass, the preparation and the first
    multi-dot pass; per iteration four launches -- curvature, step (with the multi-dot pass), combination, direction -- so an
    application is two launches behind an update and at most three anywhere"""
    name, store_route = run
    c = problem_of(name)
    p, Z, mu = c["p"], c["Z"], c["mu"]
    kw = scenarios_of(name)["half_box"]
    v = R.free_direction(p, np.random.default_rng(8))
    ev = evaluator(c, store_route)
    try:
        ev.set_option("newton_pairs", M)
        ev.reduced_lagrangian_gradient(Z, SIGMA, mu)
        first = ev.reduced_hessian_product(Z, v, SIGMA, mu)
        ev.profile_enable(True)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, v, SIGMA, mu), first)
        one, none = launches(ev, PRODUCT_NAMES), launches(ev, REBUILD_NAMES)
        assert none == (0,) * len(REBUILD_NAMES) and launches(ev, ("newton", "newton_box", "precond")) == (0, 0, 0)
        for pairs, fixed in ((False, 3), (True, 6)):
            ev.profile_reset()
            x, info = ev.preconditioned_newton_step(Z, SIGMA, mu, harvest=not pairs, **kw)
            k = info["iterations"]
            ms, n_pre, nbytes = ev.profile_get("precond")
            print(run_id(run), "pairs", info["admitted"], "iterations", k, "precond launches", n_pre, "bytes", nbytes, "bytes per iteration",
                  nbytes / max(k, 1), "ms", ms)
            assert info["status"] == CONVERGED and k >= 2 and (info["admitted"] == M) == pairs
            assert launches(ev, PRODUCT_NAMES) == tuple(k * n for n in one), "k kept-point single products"
            assert launches(ev, REBUILD_NAMES) == none, "no chain, tree-build, assembly or rollout launch"
            assert n_pre == fixed + 4 * k and nbytes > 0
            assert launches(ev, ("newton", "newton_box")) == (0, 0) and ev.profile_get("all")[1] >= 0
        ev.profile_reset()
        ev.newton_precondition(np.ones((3, Z.size)))
        assert launches(ev, ("precond",)) == (1 + 2 + 3 * 2,), "states, Gram, preparation, then two launches per column"
        ev.profile_enable(False)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------------- use
@functools.lru_cache(maxsize=None)
def oracle_trust_region_run(name, width, shift):
    """the README's loop with harvest on every step, run by the oracle alone: test_gpu_newton_box.oracle_trust_region_run with the
    restated preconditioned loop and its own store"""
    c = R.case(name)
    p, mu, n_dyn = c["p"], c["mu"], c["n_dyn"]
    ev_o = O.OracleEvaluator(p)
    nonfixed = B.nonfixed_of(p)
    store = PC.Store(M)
    log = []

    def merit(Zp):
        Zf = R.oracle_feasible(p, Zp)
        phi = SIGMA * ev_o.eval_objective(Zf)
        if mu is not None:
            phi += float(mu[n_dyn:] @ ev_o.eval_constraint(Zf)[n_dyn:])
        return phi, Zf

    phi0, Z0 = merit(c["Z"])
    lo, hi = B.loop_box(Z0, c["ref"]["C"], width)

    def step(Z, delta):
        ref = R.dense_reference(p, Z, SIGMA, mu)
        out = PC.precond_loop(lambda d: R.product_ref(ref, d), ref["r_ref"], nonfixed, Z, store.S, store.Y, lo, hi, radius=delta, shift=shift,
                              rtol=1e-6, harvest=True)
        store.harvested(out["pairs"])
        log.append((int(out["info"][0]), int(out["info"][1]), int(out["info"][12]), int(out["info"][13]), int(out["info"][14])))
        return out["info"][6], int(out["info"][0]), out["Zp"]

    return B.trust_region_loop(step, merit, Z0, phi0), (lo, hi), log


def test_a_trust_region_loop_with_a_box_and_a_harvest_on_every_step():
    """test_gpu_newton_box.test_a_trust_region_loop_with_a_box with harvest=True on every step: ten trials on scaled_12x9+con inside
    Z0 -+ 0.3; every accepted iterate is inside the box exactly, phi does not increase, and the restated loop around the oracle's product,
    carrying its own store, accepts the same trials."""
    name, width, shift = "scaled_12x9+con", 0.3, 0.0
    c = R.case(name)
    mu, Cidx = c["mu"], c["ref"]["C"]
    ev = evaluator(c, 0)
    try:
        ev.set_option("newton_pairs", M)
        Z0 = ev.feasible_trajectory_engine(c["Z"])
        lo, hi = B.loop_box(Z0, Cidx, width)
        log = []

        def step(Z, delta):
            x, info, Zp = ev.preconditioned_newton_step(Z, SIGMA, mu, None, lo, hi, radius=delta, shift=shift, rtol=1e-6, harvest=True, trajectory=True)
            log.append((info["status"], info["iterations"], info["admitted"], info["harvested"], info["fallbacks"]))
            return info["predicted"], info["status"], Zp

        def merit(Zp):
            return ev.feasible_merit(Zp, SIGMA, mu, trajectory=True)

        iterates, values, accepted = B.trust_region_loop(step, merit, Z0, ev.feasible_merit(Z0, SIGMA, mu))
    finally:
        ev.close()
    (o_iterates, o_values, o_accepted), _, o_log = oracle_trust_region_run(name, width, shift)
    print("engine: accepted", accepted, "phi", values, "(status, iterations, admitted, harvested, fallbacks) per trial", log)
    print("oracle: accepted", o_accepted, "phi", o_values, "per trial", o_log)
    for Zk in iterates:
        assert np.all(Zk[Cidx] >= lo[Cidx]) and np.all(Zk[Cidx] <= hi[Cidx]), "inside the box, exactly"
    assert np.all(np.diff(values) <= 0.0) and len(values) >= 2, "phi does not increase over the accepted trials"
    assert any(t[2] > 0 for t in log), "the pairs of an earlier step take part"
    assert accepted == o_accepted


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_device_handle_leave_nothing_written_and_the_handle_usable():
    c = R.case("scaled_12x9")
    Z = c["Z"]
    n = Z.size
    ev = dto_amd.Evaluator(c["pe"], k_lo=1, k_hi=3)                # a sharded handle: what the single product refuses
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_preconditioned_newton_step needs an unsharded handle"):
            ev.preconditioned_newton_step(Z)
    finally:
        ev.close()
    ev = evaluator(c, 0)
    try:
        ev.profile_enable(True)
        with pytest.raises(dto_amd.EngineError, match="newton_pairs"):
            ev.preconditioned_newton_step(Z, SIGMA, harvest=True)
        with pytest.raises(dto_amd.EngineError, match="newton_pairs"):
            ev.newton_pairs_push(np.ones(n), np.ones(n))
        for bad in (17, -1):
            with pytest.raises(dto_amd.EngineError, match="newton_pairs takes 0"):
                ev.set_option("newton_pairs", bad)
        ev.set_option("newton_pairs", M)
        s_bad = np.ones(n)
        s_bad[7] = np.inf
        with pytest.raises(dto_amd.EngineError, match=r"s\[7\] is not finite"):
            ev.newton_pairs_push(s_bad, np.ones(n))
        with pytest.raises(dto_amd.EngineError, match=r"y\[7\] is not finite"):
            ev.newton_pairs_push(np.ones(n), np.where(np.arange(n) == 7, np.nan, 1.0))
        assert ev.newton_pairs_info() == (0, M)
        for kw, word in ((dict(max_iter=0), "max_iter"), (dict(radius=-1.0), "radius"), (dict(rtol=np.nan), "rtol"), (dict(shift=np.inf), "shift")):
            with pytest.raises(dto_amd.EngineError, match=word):
                ev.preconditioned_newton_step(Z, SIGMA, lo=np.full(n, -1.0), **kw)
        pool = np.zeros(3 * n)
        dp = lambda a: a.ctypes.data_as(dto_amd.capi.c_double_p)
        info = np.full(16, np.nan)
        assert ev._lib.dto_preconditioned_newton_step(ev._h, dp(pool[:n]), SIGMA, None, None, None, dp(pool[n:2 * n]), None, 0.0, 0.0, 1e-6, 0.0, 5, 0,
                                                      dp(pool[2 * n:]), dp(info), None, None, dp(pool[2 * n - 1:3 * n - 1])) != 0
        assert "Zp overlaps lo" in ev._lib.dto_last_error(ev._h).decode()
        buf = np.zeros(2 * n)
        assert ev._lib.dto_newton_precondition(ev._h, None, 1, dp(buf[:n]), dp(buf[n - 1:2 * n - 1])) != 0
        assert "z overlaps r" in ev._lib.dto_last_error(ev._h).decode()
        with pytest.raises(dto_amd.EngineError, match="n_cols"):
            ev._check(ev._lib.dto_newton_precondition(ev._h, None, 0, dp(buf[:n]), dp(buf[n:])))
        assert ev.profile_get("precond")[1] == 0 and ev.profile_get("all")[1] == 0 and np.isnan(info).all() and not buf.any(), "nothing was enqueued"
        ev.profile_enable(False)
        s = steps("scaled_12x9", 0)
        same_bits(engine_step(ev, problem_of("scaled_12x9"), s["sc"]["half_box"]), s["empty", "half_box"][1], "after the refusals", upto=12)
    finally:
        ev.close()
