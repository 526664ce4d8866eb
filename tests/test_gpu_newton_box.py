"""GPU: the bound-constrained truncated-Newton step (dto_projected_newton_step_box and its _dev form, csrc/dto_newton_box.hip,
csrc/dto_newton_box_plan.h).

References.  BITS: the loop of include/dto_engine.h, "Bound-constrained truncated-Newton step", written in NumPy
(newton_box_cases.box_loop, which test_newton_box_plan_header.py holds the plain-C++ header to) around the same handle's
reduced_hessian_product and reduced_lagrangian_gradient -- p, info, trace, entry_state and Zp must be equal, not close.  EQUIVALENCE:
reduced_newton_step on the same handle.  VALUES: the oracle's dense reduced Hessian and gradient.  The scenarios come from the oracle
alone (newton_box_cases; test_newton_box_scenarios.py asserts what they are meant to be).  Outputs are pre-filled with NaN.

Shapes: 41 .. 250 entries (1 - 2 chunks) and 40 x 258 (11610 entries: 46 chunks, the last ragged); both "reduced_input_store" routes on
scaled_40x6 and on the long case."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import newton_box_cases as B
import reduced_cases as R
from test_gpu_newton_step import PRODUCT_NAMES, REBUILD_NAMES, dense_bar, device_arrays, evaluator, launches, problem_of, run_id
from test_newton_plan_header import CONVERGED, MAX_ITER

pytestmark = pytest.mark.gpu

SMALL = ["scaled_12x9", "scaled_12x9+con", "scaled_40x6", "tdb_order1", "structured_16x4"]
LONG = "scaled_40x258"
RUNS = [(n, 0) for n in SMALL] + [("scaled_40x6", 1), (LONG, 0), (LONG, 1)]
SIGMA = R.SIGMA
KINDS = B.SCENARIOS + ("max_iter_3",)


def scenarios_of(name):
    sc = dict(B.long_scenarios(name) if name == LONG else B.small_scenarios(name))
    sc["max_iter_3"] = dict(sc["half_box"], max_iter=3)
    return sc


def engine_step(ev, c, kw):
    x, info, tr, es, zp = ev.reduced_newton_step_box(c["Z"], SIGMA, c["mu"], trace=True, states=True, trajectory=True, **kw)
    return dict(p=x, info=info["raw"], trace=tr, states=es, Zp=zp, named=info)


def numpy_step(ev, c, kw):
    Z, mu = c["Z"], c["mu"]
    return B.box_loop(lambda d: ev.reduced_hessian_product(Z, d, SIGMA, mu), ev.reduced_lagrangian_gradient(Z, SIGMA, mu), B.nonfixed_of(c["p"]),
                      Z, **kw)


@functools.lru_cache(maxsize=None)
def steps(name, store):
    """every run of one (case, route) on ONE handle, each beside its restatement: computed once, shared, never written"""
    import torch
    c = problem_of(name)
    Z, mu = c["Z"], c["mu"]
    sc = scenarios_of(name)
    out = dict(c=c, sc=sc)
    ev = evaluator(c, store)
    try:
        for kind in KINDS:
            out[kind] = (engine_step(ev, c, sc[kind]), numpy_step(ev, c, sc[kind]))
        out["unbounded"] = ev.reduced_newton_step(Z, SIGMA, mu, trace=True, **sc["inf"])
        n = Z.size
        out["null_bounds"] = engine_step(ev, c, dict(sc["inf"], lo=None, hi=None))
        out["inf_vectors"] = engine_step(ev, c, dict(sc["inf"], lo=np.full(n, -np.inf), hi=np.full(n, np.inf)))
        if name != LONG:
            tight = {k: dict(sc[k], rtol=1e-10) for k in B.CONVEX}
            out["tight"] = {k: engine_step(ev, c, tight[k]) for k in B.CONVEX}
            out["tight_Ap"] = {k: ev.reduced_hessian_product(Z, out["tight"][k]["p"], SIGMA, mu) + sc["shift"] * out["tight"][k]["p"] for k in B.CONVEX}
            out["g"] = ev.reduced_lagrangian_gradient(Z, SIGMA, mu)
        # the other entry-point family, a repeated call, and a call after a merit value at another Z: the bits of the first run
        kw = sc["half_box"]
        (dZ, dlo, dhi), st = device_arrays(Z, kw["lo"], kw["hi"])
        dmu = 0 if mu is None else device_arrays(mu)[0][0]
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dZ.device)
        dp, dinfo, dtrace, des, dzp = nan(n), nan(12), nan(kw["max_iter"], 6), nan(n), nan(n)
        ev.reduced_newton_step_box_dev(dZ.data_ptr(), SIGMA, 0 if mu is None else dmu.data_ptr(), 0, dlo.data_ptr(), dhi.data_ptr(), 0.0, kw["shift"],
                                       kw["rtol"], 0.0, kw["max_iter"], dp.data_ptr(), dinfo.data_ptr(), dtrace.data_ptr(), des.data_ptr(),
                                       dzp.data_ptr(), stream=st)
        torch.cuda.synchronize()
        out["dev"] = dict(p=dp.cpu().numpy(), info=dinfo.cpu().numpy(), trace=dtrace.cpu().numpy(), states=des.cpu().numpy(), Zp=dzp.cpu().numpy())
        out["again"] = engine_step(ev, c, kw)
        Z2 = np.array(Z)
        Z2[c["p"].dt_idx] *= 1.25
        assert np.isfinite(ev.feasible_merit(Z2, SIGMA, mu))
        out["after_merit"] = engine_step(ev, c, kw)
        x_bare, info_bare = ev.reduced_newton_step_box(Z, SIGMA, mu, **kw)       # none of the optional outputs
        out["bare"] = (x_bare, info_bare["raw"])
    finally:
        ev.close()
    return out


def same_bits(got, want, what):
    assert not np.isnan(got["p"]).any() and not np.isnan(got["info"][:7]).any(), what
    for key in ("p", "info", "states", "Zp"):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert got["trace"].shape == want["trace"].shape and np.array_equal(got["trace"], want["trace"]), (what, "trace", got["trace"], want["trace"])


# ------------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_step_is_the_numpy_loop_bit_for_bit(run):
    s = steps(*run)
    for kind in KINDS:
        got, want = s[kind]
        i = got["named"]
        print(run_id(run), kind, "status", i["status"], "iterations", i["iterations"], "held", i["held"], "hit", i["hit"], "restarts", i["restarts"],
              "|F|", i["n_free"], "|r|/|g|", i["rnorm"] / i["gnorm"])
        same_bits(got, want, kind)
    assert s["max_iter_3"][0]["named"]["status"] == MAX_ITER and s["max_iter_3"][0]["named"]["iterations"] == 3
    assert s["half_box"][0]["named"]["hit"] >= 3 and s["half_box"][0]["named"]["restarts"] >= 2
    assert s["held"][0]["named"]["held"] == 4


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_both_families_a_repeated_call_and_a_call_after_a_merit_value_return_the_same_bits(run):
    s = steps(*run)
    first = s["half_box"][0]
    k = first["named"]["iterations"]
    dev = s["dev"]
    for key in ("p", "info", "states", "Zp"):
        assert np.array_equal(dev[key], first[key]), key
    assert np.array_equal(dev["trace"][:k], first["trace"]) and np.isnan(dev["trace"][k:]).all(), "rows past the last iteration stay NaN"
    for form in ("again", "after_merit"):
        same_bits(s[form], first, form)
    assert np.array_equal(s["bare"][0], first["p"]) and np.array_equal(s["bare"][1], first["info"]), "the optional outputs change nothing"


# ----------------------------------------------------------------------------------------------------------- equivalence
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_without_bounds_it_is_the_unbounded_step_bit_for_bit(run):
    s = steps(*run)
    x, info, tr = s["unbounded"]
    assert info["status"] == CONVERGED and info["iterations"] >= 2
    for form in (s["inf"][0], s["null_bounds"], s["inf_vectors"]):
        assert np.array_equal(form["p"], x) and np.array_equal(form["info"][:8], info["raw"])
        assert np.array_equal(form["trace"][:, :4], tr) and np.all(form["trace"][:, 4] == np.inf) and np.all(form["trace"][:, 5] == 0.0)
        assert np.array_equal(form["info"][8:11], [0.0, 0.0, 0.0]) and form["info"][11] == np.sum(form["states"] == B.FREE)
        assert np.array_equal(form["Zp"], s["c"]["Z"] + x)


# ----------------------------------------------------------------------------------------------------------- feasibility
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_step_stays_inside_the_box_exactly(run):
    s = steps(*run)
    p, Z = s["c"]["p"], s["c"]["Z"]
    S = R.index_sets(p)[0]
    n = Z.size
    for kind in KINDS:
        got, kw = s[kind][0], s["sc"][kind]
        lo, hi = kw.get("lo", np.full(n, -np.inf)), kw.get("hi", np.full(n, np.inf))
        es, zp, x, info = got["states"], got["Zp"], got["p"], got["info"]
        assert set(np.unique(es)) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0} and np.all(es[S] == B.FIXED)
        moving = es != B.FIXED
        assert np.all(zp[moving] >= lo[moving]) and np.all(zp[moving] <= hi[moving]), kind
        assert np.array_equal(zp[es == B.HIT_LO], lo[es == B.HIT_LO]) and np.array_equal(zp[es == B.HIT_HI], hi[es == B.HIT_HI]), kind
        still = (es == B.FIXED) | (es == B.HELD_LO) | (es == B.HELD_HI)
        assert np.all(x[still] == 0.0) and np.array_equal(zp[still], Z[still] + 0.0), kind
        assert info[8] == np.sum((es == B.HELD_LO) | (es == B.HELD_HI)) and info[9] == np.sum(es >= B.HIT_LO) and info[11] == np.sum(es == B.FREE), kind
        assert info[10] == np.sum(got["trace"][:, 5] > 0) - (1 if got["trace"][-1, 5] > 0 and info[0] not in (-1.0, float(MAX_ITER)) else 0), kind
        assert info[9] == np.sum(got["trace"][:, 5]), kind


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("kind", B.CONVEX)
def test_values_against_the_oracle(name, kind):
    """The active set: the engine's states are the states of the loop run with the oracle's matrix and gradient alone.  On the final face
    ||p_F - solve(A_FF, -(g_F + A_FB p_B))|| <= (2 rtol ||g|| + gradient_bar + product_bar(p)) / lambda_min(A_FF): test_gpu_newton_step.py's
    bar through ||A_FF^-1||.  The predicted decrease against -(g'p + p'Ap / 2) recomputed with one engine product: that test's 1e-10
    relative, plus n_hit eps ||A|| ||p|| for the clamps, whose rounding r is not corrected for."""
    s, c = steps(name, 0), R.case(name)
    ref, Cidx = c["ref"], c["ref"]["C"]
    kw = dict(s["sc"][kind], rtol=1e-10)
    got = s["tight"][kind]
    want = B.box_loop(B.oracle_product(name), np.array(ref["r_ref"]), B.nonfixed_of(c["p"]), c["Z"], **kw)
    assert got["named"]["status"] == CONVERGED and int(want["info"][0]) == CONVERGED
    assert np.array_equal(got["states"], want["states"]), "the engine ends on the oracle's face"
    es, x = got["states"][Cidx], got["p"][Cidx]
    F, Bd = es == B.FREE, es >= B.HIT_LO
    A = ref["Hr"] + s["sc"]["shift"] * np.eye(Cidx.size)
    g = ref["r_ref"][Cidx]
    pF = np.linalg.solve(A[np.ix_(F, F)], -(g[F] + A[np.ix_(F, Bd)] @ x[Bd]))
    err = float(np.linalg.norm(x[F] - pF))
    b = dense_bar(ref, c["levels"], 1e-10, A[np.ix_(F, F)], got["p"], got["named"]["gnorm"])
    print(name, kind, "face: free", int(F.sum()), "hit", int(Bd.sum()), "||p_F - p_F*||", err, "bar", b, "ratio", err / b)
    assert err <= b
    full = got["p"]
    recomputed = -(float(s["g"] @ full) + 0.5 * float(full @ s["tight_Ap"][kind]))
    slack = 1e-10 * abs(recomputed) + got["named"]["hit"] * np.finfo(float).eps * float(np.linalg.norm(A, 2)) * float(np.linalg.norm(full))
    print(name, kind, "predicted", got["named"]["predicted"], "recomputed", recomputed, "difference", got["named"]["predicted"] - recomputed, "bar", slack)
    assert abs(got["named"]["predicted"] - recomputed) <= slack


# --------------------------------------------------------------------------------------------------- kept points, launches
@pytest.mark.parametrize("run", [("scaled_40x6", 1), ("scaled_40x6", 0)], ids=run_id)
def test_a_step_is_k_kept_point_products_and_the_box_launches(run):
    name, store = run
    c = problem_of(name)
    p, Z, mu = c["p"], c["Z"], c["mu"]
    kw = scenarios_of(name)["half_box"]
    v = R.free_direction(p, np.random.default_rng(8))
    ev = evaluator(c, store)
    try:
        ev.reduced_lagrangian_gradient(Z, SIGMA, mu)
        first = ev.reduced_hessian_product(Z, v, SIGMA, mu)
        ev.profile_enable(True)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, v, SIGMA, mu), first)
        one, none = launches(ev, PRODUCT_NAMES), launches(ev, REBUILD_NAMES)
        assert none == (0,) * len(REBUILD_NAMES) and launches(ev, ("newton", "newton_box")) == (0, 0)
        ev.profile_reset()
        x, info = ev.reduced_newton_step_box(Z, SIGMA, mu, **kw)
        k = info["iterations"]
        ms, n_box, nbytes = ev.profile_get("newton_box")
        print(run_id(run), "iterations", k, "launches of one product", dict(zip(PRODUCT_NAMES, one)), "newton_box", n_box, "bytes", nbytes, "ms", ms)
        assert info["status"] == CONVERGED and k >= 2 and info["hit"] >= 3
        assert launches(ev, PRODUCT_NAMES) == tuple(k * n for n in one), "k kept-point single products"
        assert launches(ev, REBUILD_NAMES) == none, "no chain, tree-build, assembly or rollout launch"
        assert n_box == 2 + 3 * k and nbytes > 0, "start and its closing launch, then three per iteration; bytes as executed"
        assert launches(ev, ("newton",)) == (0,)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, v, SIGMA, mu), first)
        assert launches(ev, PRODUCT_NAMES) == one and launches(ev, REBUILD_NAMES) == none, "a following product is at its kept point"
        ev.profile_enable(False)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------------- use
@functools.lru_cache(maxsize=None)
def oracle_trust_region_run(name, width):
    """the README's loop run by the oracle alone: dense reduced Hessian and gradient per iterate, Newton on the dynamics rows for the
    feasible trajectory, the oracle's objective and constraint values for the merit"""
    c = R.case(name)
    p, mu, n_dyn = c["p"], c["mu"], c["n_dyn"]
    ev_o = O.OracleEvaluator(p)
    nonfixed = B.nonfixed_of(p)

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
        out = B.box_loop(lambda d: R.product_ref(ref, d), ref["r_ref"], nonfixed, Z, lo, hi, radius=delta, rtol=1e-6)
        return out["info"][6], int(out["info"][0]), out["Zp"]

    return B.trust_region_loop(step, merit, Z0, phi0), (lo, hi)


def test_a_trust_region_loop_with_a_box():
    """ten trials of the README's loop on scaled_12x9+con inside Z0 -+ 0.3: every accepted iterate is inside the box exactly, phi does
    not increase over the accepted trials, and the oracle's run of the same loop accepts the same trials.  (The width is chosen on the
    oracle's run alone: at 0.3 every trial's ratio rho is at least 0.05 away from the acceptance bar 0.1; at 0.2 the last two trials
    predict decreases of 2e-9 and 1e-19 and their ratios are rounding.)"""
    name, width = "scaled_12x9+con", 0.3
    c = R.case(name)
    mu, Cidx = c["mu"], c["ref"]["C"]
    ev = evaluator(c, 0)
    try:
        Z0 = ev.feasible_trajectory_engine(c["Z"])
        lo, hi = B.loop_box(Z0, Cidx, width)
        hits = []

        def step(Z, delta):
            x, info, Zp = ev.reduced_newton_step_box(Z, SIGMA, mu, lo, hi, radius=delta, rtol=1e-6, trajectory=True)
            hits.append((info["status"], info["iterations"], info["held"], info["hit"]))
            return info["predicted"], info["status"], Zp

        def merit(Zp):
            return ev.feasible_merit(Zp, SIGMA, mu, trajectory=True)

        iterates, values, accepted = B.trust_region_loop(step, merit, Z0, ev.feasible_merit(Z0, SIGMA, mu))
    finally:
        ev.close()
    (o_iterates, o_values, o_accepted), _ = oracle_trust_region_run(name, width)
    print("engine: accepted", accepted, "phi", values, "(status, iterations, held, hit) per trial", hits)
    print("oracle: accepted", o_accepted, "phi", o_values)
    for Zk in iterates:
        assert np.all(Zk[Cidx] >= lo[Cidx]) and np.all(Zk[Cidx] <= hi[Cidx]), "inside the box, exactly"
    assert np.all(np.diff(values) <= 0.0) and len(values) >= 2, "phi does not increase over the accepted trials"
    assert any(h[2] + h[3] > 0 for h in hits), "the box takes part"
    assert accepted == o_accepted


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_device_handle_leave_nothing_written_and_the_handle_usable():
    c = R.case("scaled_12x9")
    Z = c["Z"]
    n = Z.size
    ev = dto_amd.Evaluator(c["pe"], k_lo=1, k_hi=3)                # a sharded handle: what the single product refuses
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_projected_newton_step_box needs an unsharded handle"):
            ev.reduced_newton_step_box(Z)
    finally:
        ev.close()
    ev = evaluator(c, 0)
    try:
        ev.profile_enable(True)
        for kw, word in ((dict(max_iter=0), "max_iter"), (dict(radius=-1.0), "radius"), (dict(rtol=np.nan), "rtol"), (dict(shift=np.inf), "shift")):
            with pytest.raises(dto_amd.EngineError, match=word):
                ev.reduced_newton_step_box(Z, SIGMA, lo=np.full(n, -1.0), **kw)
        pool = np.zeros(3 * n)
        dp = lambda a: a.ctypes.data_as(dto_amd.capi.c_double_p)
        info = np.full(12, np.nan)
        assert ev._lib.dto_projected_newton_step_box(ev._h, dp(pool[:n]), SIGMA, None, None, dp(pool[n:2 * n]), None, 0.0, 0.0, 1e-6, 0.0, 5,
                                                     dp(pool[2 * n:]), dp(info), None, None, dp(pool[2 * n - 1:3 * n - 1])) != 0
        assert "Zp overlaps lo" in ev._lib.dto_last_error(ev._h).decode()
        assert ev.profile_get("newton_box")[1] == 0 and ev.profile_get("all")[1] == 0 and np.isnan(info).all(), "nothing was enqueued"
        ev.profile_enable(False)
        s = steps("scaled_12x9", 0)
        same_bits(engine_step(ev, problem_of("scaled_12x9"), s["sc"]["half_box"]), s["half_box"][0], "after the refusals")
    finally:
        ev.close()
