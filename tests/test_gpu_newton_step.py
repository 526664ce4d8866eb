"""GPU: the device truncated-Newton step (dto_projected_newton_step and its _dev form, csrc/dto_newton.hip, csrc/dto_newton_plan.h).

References.  BITS: the loop of include/dto_engine.h, "Truncated-Newton step", written in NumPy around the same handle's
reduced_hessian_product, with the stated dot order (the restatement test_newton_plan_header.py holds the header to) and np.sqrt -- p,
info and every trace row must be equal, not close.  VALUES: the oracle's dense reduced Hessian and gradient (reduced_cases.dense_reference),
p* = solve(Hr + shift I, -r) on C, held to the project's own bars pushed through ||A^-1||.  Outputs are pre-filled with NaN.

Shapes: the small cases of reduced_cases (41 .. 250 variables of the reduced problem: 1 .. 2 chunks of the dot) and two long ones,
40 x 258 (11610 entries: 46 chunks, the last ragged) and 64 x 320 (22080: 87 chunks, a lane of the final stage holds two partial sums)."""
import functools
import math

import numpy as np
import pytest

import dto_amd
import long_cases as LC
import reduced_cases as R
from helpers import to_engine
from test_newton_plan_header import BOUNDARY, CONTINUE, CONVERGED, MAX_ITER, NEG_CURVATURE, NOT_FINITE, decide_restated, dot_restated, lanes, tree64

pytestmark = pytest.mark.gpu

# the small path; the same with a constraint row (mu given); the one-launch chain; the general path; shared generators with a derivative
# between; a time-dependent integrator on the slab route of J w / J' w; the structured path
SMALL = ["scaled_12x9", "scaled_12x9+con", "scaled_40x6", "scaled_70x5", "multi_ket_between", "tdb_order1", "structured_16x4"]
LONG = ["scaled_40x258", "scaled_64x320"]
# (case, "reduced_input_store"): both routes on one small and one long case at least
RUNS = [(n, 0) for n in SMALL] + [("scaled_40x6", 1), ("scaled_12x9+con", 1)] + [(n, 1) for n in LONG] + [("scaled_64x320", 0)]
INDEFINITE = {"scaled_12x9": 1, "scaled_40x6": 2, "scaled_70x5": 3}    # the iteration in which the oracle's CG meets kappa <= 0 at shift = 0
SIGMA = R.SIGMA


def run_id(r):
    return f"{r[0]}-store{r[1]}"


def device_arrays(*arrays):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays], torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------------------------------------------------ the loop in NumPy
def dot(x, y):
    """the stated order, vectorised over the chunks: lane sums of four entries, the halving tree, one wavefront over the chunk sums"""
    prod = x * y
    nb = -(-prod.size // 256)
    a = np.zeros(nb * 256)
    a[:prod.size] = prod
    a = a.reshape(nb, 4, 64)
    lane = np.zeros((nb, 64))
    for t in range(4):
        lane = lane + a[:, t]
    return float(tree64(lanes(tree64(lane))))


def free_entries(p, free):
    M = np.ones(p.n_vars, dtype=bool)
    M[R.index_sets(p)[0]] = False
    if free is not None:
        M &= np.asarray(free) != 0.0     # (a NaN counts as free; the mask of a dependent entry decides nothing)
    return M


def cg_in_numpy(ev, p, Z, mu, free=None, radius=0.0, shift=0.0, rtol=1e-6, atol=0.0, max_iter=50):
    """(p, info [8], trace [iterations][4], the last direction d) by the header's loop, every y from ev.reduced_hessian_product"""
    M = free_entries(p, free)
    g = np.where(M, ev.reduced_lagrangian_gradient(Z, SIGMA, mu), 0.0)
    r, x, d = g.copy(), np.zeros(p.n_vars), -g
    rr0 = rr = dot(r, r)
    if rr == 0.0:
        return x, np.array([CONVERGED, 0.0, 0.0, 0.0, 0.0, 0.0, -0.5 * (0.0 + 0.0), 0.0]), np.zeros((0, 4)), d
    trace = []
    for j in range(1, max_iter + 1):
        y = ev.reduced_hessian_product(Z, d, SIGMA, mu)
        w = np.where(M, y + shift * d, 0.0)
        kappa, dd, pd, pp = dot(d, w), dot(d, d), dot(x, d), dot(x, x)
        status, s = decide_restated(kappa, dd, pd, pp, rr, radius, j)
        if status != NOT_FINITE:
            x = x + s * d
            r = r + s * w
        rr_new = dot(r, r)
        trace.append([kappa, dd, s, rr_new])
        if status == CONTINUE:
            if np.sqrt(rr_new) <= max(atol, rtol * np.sqrt(rr0)):
                status = CONVERGED
            else:
                d = (rr_new / rr) * d - r
                rr = rr_new
                if j == max_iter:
                    status = MAX_ITER
        if status != CONTINUE:
            break
    pg = dot(x, g)
    info = np.array([status, j, np.sqrt(rr0), np.sqrt(rr_new), np.sqrt(dot(x, x)), pg, -0.5 * (pg + dot(x, r)), kappa / dd])
    return x, info, np.array(trace), d


def same_bits(got, want, what):
    p, info, tr = got
    raw = info["raw"] if isinstance(info, dict) else info
    assert not np.isnan(p).any() and not np.isnan(raw[:7]).any(), what
    assert np.array_equal(p, want[0]), (what, "p", float(np.max(np.abs(p - want[0]))))
    assert np.array_equal(raw, want[1]), (what, "info", raw, want[1])
    assert tr.shape == want[2].shape and np.array_equal(tr, want[2]), (what, "trace", tr, want[2])


# ------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def problem_of(name):
    """what a run needs of a case without its dense reference: oracle problem, engine problem, keywords, the point, mu"""
    if name in LONG:
        p, kw = R.problem(name)
        Z = LC.long_point(p)
        Z.setflags(write=False)
        return dict(p=p, pe=to_engine(p), kw=kw, Z=Z, mu=None)
    c = R.case(name)
    return dict(p=c["p"], pe=c["pe"], kw=c["kw"], Z=c["Z"], mu=c["mu"])


def evaluator(c, store):
    ev = dto_amd.Evaluator(c["pe"], **c["kw"])
    if store:
        ev.set_option("reduced_input_store", 1)
    return ev


def power_shift(ev, c):
    """2 max |Rayleigh quotient| over 8 power iterations with the engine's product: A is then positive definite, condition <= 3"""
    p, Z, mu = c["p"], c["Z"], c["mu"]
    v = R.free_direction(p, np.random.default_rng(5))
    top = 0.0
    for _ in range(8):
        v = v / np.linalg.norm(v)
        y = ev.reduced_hessian_product(Z, v, SIGMA, mu)
        top = max(top, abs(float(v @ y)))
        v = y
    return 2.0 * top


@functools.lru_cache(maxsize=None)
def steps(name, store):
    """every run of one (case, route) on ONE handle, each beside its restatement: computed once, shared, never written"""
    import torch
    c = problem_of(name)
    p, Z, mu = c["p"], c["Z"], c["mu"]
    out = dict(c=c)
    ev = evaluator(c, store)
    try:
        def both(**kw):
            got = ev.reduced_newton_step(Z, SIGMA, mu, trace=True, **kw)
            return got, cg_in_numpy(ev, p, Z, mu, **kw)

        if name in LONG:
            out["shift"] = shift = power_shift(ev, c)
        else:
            Hr, C_ = ev.reduced_hessian_matrix(Z, SIGMA, mu)
            lam = np.linalg.eigvalsh(0.5 * (Hr + Hr.T))
            out["lam"] = lam
            out["shift"] = shift = 1.5 * abs(lam[0]) + 0.01 * lam[-1]
        out["converged"] = both(shift=shift, rtol=1e-8, max_iter=40)
        pstar = out["converged"][0][1]["pnorm"]
        out["boundary"] = both(shift=shift, rtol=1e-8, max_iter=40, radius=0.5 * pstar)
        out["max_iter"] = both(shift=shift, rtol=1e-8, max_iter=3)
        if name in INDEFINITE:
            out["negative"] = both(shift=0.0, rtol=1e-8, max_iter=40)
            out["negative_radius"] = both(shift=0.0, rtol=1e-8, max_iter=40, radius=1e3)
            d = out["negative"][1][3]      # the direction of the last iteration (the restatement's: the traces are equal bit for bit)
            out["negative_dAd"] = float(d @ ev.reduced_hessian_product(Z, d, SIGMA, mu))
        if name not in LONG:
            out["tight"] = ev.reduced_newton_step(Z, SIGMA, mu, shift=shift, rtol=1e-10, max_iter=60)
            x = out["tight"][0]
            out["tight_Ap"] = ev.reduced_hessian_product(Z, x, SIGMA, mu) + shift * x
            out["g"] = ev.reduced_lagrangian_gradient(Z, SIGMA, mu)
        # the other entry-point family, a repeated call, and a call after a merit value at another Z: the bits of the first run
        kw = dict(shift=shift, rtol=1e-8, max_iter=40)
        (dZ,), st = device_arrays(Z)
        dmu = 0 if mu is None else device_arrays(mu)[0][0]
        dp = torch.full_like(dZ, float("nan"))
        dinfo = torch.full((8,), float("nan"), dtype=torch.float64, device=dZ.device)
        dtrace = torch.full((40, 4), float("nan"), dtype=torch.float64, device=dZ.device)
        ev.reduced_newton_step_dev(dZ.data_ptr(), SIGMA, 0 if mu is None else dmu.data_ptr(), 0, 0.0, shift, 1e-8, 0.0, 40, dp.data_ptr(),
                                   dinfo.data_ptr(), dtrace.data_ptr(), stream=st)
        torch.cuda.synchronize()
        out["dev"] = (dp.cpu().numpy(), dinfo.cpu().numpy(), dtrace.cpu().numpy())
        out["again"] = ev.reduced_newton_step(Z, SIGMA, mu, trace=True, **kw)
        Z2 = np.array(Z)
        Z2[p.dt_idx] *= 1.25
        assert np.isfinite(ev.feasible_merit(Z2, SIGMA, mu))
        out["after_merit"] = ev.reduced_newton_step(Z, SIGMA, mu, trace=True, **kw)
    finally:
        ev.close()
    return out


# ------------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_the_step_is_the_numpy_loop_bit_for_bit(run):
    s = steps(*run)
    for kind in ("converged", "boundary", "max_iter", "negative", "negative_radius"):
        if kind in s:
            got, want = s[kind]
            print(run_id(run), kind, "status", got[1]["status"], "iterations", got[1]["iterations"], "|r|/|g|", got[1]["rnorm"] / got[1]["gnorm"])
            same_bits(got, want, kind)


def test_the_vectorised_dot_is_the_restated_one():
    rng = np.random.default_rng(2)
    for n in (41, 257, 11610, 22080):
        x, y = rng.standard_normal(n) * 10.0 ** rng.integers(-5, 6, n), rng.standard_normal(n)
        assert dot(x, y) == float(dot_restated(x, y))


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_both_families_a_repeated_call_and_a_call_after_a_merit_value_return_the_same_bits(run):
    s = steps(*run)
    first = s["converged"][0]
    k = first[1]["iterations"]
    dp, dinfo, dtrace = s["dev"]
    assert np.array_equal(dp, first[0]) and np.array_equal(dinfo, first[1]["raw"])
    assert np.array_equal(dtrace[:k], first[2]) and np.isnan(dtrace[k:]).all(), "rows past the last iteration are untouched"
    for form in ("again", "after_merit"):
        same_bits(s[form], (first[0], first[1]["raw"], first[2]), form)


# ------------------------------------------------------------------------------------------------------------ every exit
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_converged_boundary_and_max_iter(run):
    s = steps(*run)
    name = run[0]
    p = s["c"]["p"]
    S = R.index_sets(p)[0]
    x, info, tr = s["converged"][0]
    print(run_id(run), "shift", s["shift"], "converged in", info["iterations"], "|p|", info["pnorm"], "predicted", info["predicted"])
    assert info["status"] == CONVERGED and 1 <= info["iterations"] <= 40 and tr.shape == (info["iterations"], 4)
    assert info["rnorm"] <= 1e-8 * info["gnorm"] and info["gnorm"] > 0
    assert np.all(tr[:, 0] > 0) and np.all(x[S] == 0.0), "positive curvature all the way; p is exactly 0 on S"
    assert info["predicted"] > 0 and info["pg"] < 0
    xb, ib, tb = s["boundary"][0]
    assert ib["status"] == BOUNDARY and ib["iterations"] <= info["iterations"]
    radius = 0.5 * info["pnorm"]
    assert abs(ib["pnorm"] - radius) <= 1e-12 * radius and abs(np.linalg.norm(xb) - radius) <= 1e-12 * radius
    assert ib["predicted"] > 0 and np.all(xb[S] == 0.0)
    xm, im, tm = s["max_iter"][0]
    assert im["status"] == MAX_ITER and im["iterations"] == 3 and tm.shape == (3, 4)
    assert np.array_equal(tm, tr[:3]), "the first three iterations of the longer run"
    assert im["rnorm"] > 1e-8 * im["gnorm"]


@pytest.mark.parametrize("name", list(INDEFINITE))
def test_negative_curvature(name):
    s = steps(name, 0)
    lam = s["lam"]
    print(name, "engine's reduced Hessian: eigenvalues", lam[0], "..", lam[-1], "negative", int(np.sum(lam < 0)), "of", lam.size)
    assert lam[0] < 0 < lam[-1], "indefinite"
    x, info, tr = s["negative"][0]
    print(name, "shift 0: status", info["status"], "iteration", info["iterations"], "kappa", tr[-1, 0])
    assert info["status"] == NEG_CURVATURE and info["iterations"] == INDEFINITE[name]
    assert tr[-1, 0] <= 0 and np.all(tr[:-1, 0] > 0) and info["curvature"] == tr[-1, 0] / tr[-1, 1]
    assert tr[-1, 2] == (1.0 if info["iterations"] == 1 else 0.0), "without a radius: d in the first iteration, nothing later"
    assert s["negative_dAd"] <= 0, "d'Ad of the last direction, recomputed with an engine product"
    assert abs(s["negative_dAd"] - tr[-1, 0]) <= 1e-10 * abs(tr[-1, 0]), "NumPy's summation order against the stated one"
    if info["iterations"] == 1:
        assert np.array_equal(x, s["negative"][1][3]), "p = 0 + 1 * d"
    xr, ir, trr = s["negative_radius"][0]
    assert ir["status"] == NEG_CURVATURE and ir["iterations"] == INDEFINITE[name]
    assert abs(ir["pnorm"] - 1e3) <= 1e-12 * 1e3 and abs(np.linalg.norm(xr) - 1e3) <= 1e-12 * 1e3
    assert np.array_equal(trr[:-1], tr[:-1]) and trr[-1, 2] > 0, "the same iterations up to the exit, then to the boundary along d"


# ---------------------------------------------------------------------------------------------------------------- values
def dense_bar(ref, levels, rtol, A, pstar_full, gnorm):
    lam_min = float(np.linalg.eigvalsh(0.5 * (A + A.T))[0])
    assert lam_min > 0
    return (2.0 * rtol * gnorm + R.gradient_bar(ref, levels) + R.product_bar(ref, pstar_full)) / lam_min


@pytest.mark.parametrize("name", SMALL)
def test_values_against_the_dense_solve_of_the_oracle(name):
    """||p - p*|| <= (2 rtol ||g|| + gradient_bar + product_bar(p*)) / lambda_min(A_ref): the residual the iteration stops at (twice: the
    recurrence residual drifts from the true one), the error the gradient may have and the error a product with p* may have, each
    through ||A^-1||.  The test prints each ratio to the bar; DESIGN 4.32 records the largest."""
    s, c = steps(name, 0), R.case(name)
    ref, Cidx = c["ref"], c["ref"]["C"]
    x, info = s["tight"]
    assert info["status"] == CONVERGED
    A = ref["Hr"] + s["shift"] * np.eye(Cidx.size)
    pstar = np.zeros(x.size)
    pstar[Cidx] = np.linalg.solve(A, -ref["r_ref"][Cidx])
    err, b = float(np.linalg.norm(x - pstar)), dense_bar(ref, c["levels"], 1e-10, A, pstar, info["gnorm"])
    print(name, "||p - p*||", err, "bar", b, "ratio", err / b, "||p*||", np.linalg.norm(pstar), "iterations", info["iterations"])
    assert err <= b
    # the predicted decrease -(g'p + p'Ap / 2), recomputed with one engine product
    want = -(float(s["g"] @ x) + 0.5 * float(x @ s["tight_Ap"]))
    print(name, "predicted", info["predicted"], "recomputed", want)
    assert abs(info["predicted"] - want) <= 1e-10 * abs(want)


# ------------------------------------------------------------------------------------------------------------------ mask
def test_the_free_mask():
    name = "scaled_12x9+con"
    c = R.case(name)
    p, Z, mu, ref = c["p"], c["Z"], c["mu"], c["ref"]
    n, z = p.integrators[0].x_dim, p.z
    S, Cidx, _, _ = R.index_sets(p)
    free = np.ones(p.n_vars)
    fixed = [k * z + n + 2 + a for k in (2, 3, 4) for a in (0, 1)] + [6 * z + p.dt_idx]     # du of knots 3 - 5, one timestep
    free[fixed] = 0.0
    free[z + 3] = np.nan        # a dependent entry: its mask is not read
    free[S[-1]] = 0.0
    shift = steps(name, 0)["shift"]
    ev = evaluator(c, 0)
    try:
        got = ev.reduced_newton_step(Z, SIGMA, mu, free=free, shift=shift, rtol=1e-10, max_iter=60, trace=True)
        want = cg_in_numpy(ev, p, Z, mu, free=free, shift=shift, rtol=1e-10, max_iter=60)
    finally:
        ev.close()
    same_bits(got, want, "masked")
    x, info, _ = got
    assert info["status"] == CONVERGED
    assert np.all(x[fixed] == 0.0) and np.all(x[S] == 0.0) and not np.isnan(x).any()
    keep = np.flatnonzero(~np.isin(Cidx, fixed))
    A = (ref["Hr"] + shift * np.eye(Cidx.size))[np.ix_(keep, keep)]
    pstar = np.zeros(x.size)
    pstar[Cidx[keep]] = np.linalg.solve(A, -ref["r_ref"][Cidx[keep]])
    err, b = float(np.linalg.norm(x - pstar)), dense_bar(ref, c["levels"], 1e-10, A, pstar, info["gnorm"])
    print("masked", len(fixed), "of", Cidx.size, "free entries: ||p - p*||", err, "bar", b, "ratio", err / b)
    assert err <= b
    unmasked = steps(name, 0)["tight"][0]
    assert not np.array_equal(unmasked, x) and np.any(unmasked[fixed] != 0.0), "the mask takes part"


# --------------------------------------------------------------------------------------------------- kept points, launches
PRODUCT_NAMES = ("hess_product", "reduced_pack", "reduced_input", "dynsolve_scan", "dynsolve_couple", "dynsolve_deriv", "jac_product", "expmv",
                 "all")
REBUILD_NAMES = ("bgemm", "chain64", "dynsolve_tree", "assembly", "rollout_tree", "feasible")


def launches(ev, names):
    return tuple(ev.profile_get(n)[1] for n in names)


@pytest.mark.parametrize("run", [("scaled_40x6", 1), ("scaled_40x6", 0), ("scaled_70x5", 1)], ids=run_id)
def test_a_step_is_k_kept_point_products_and_the_newton_launches(run):
    name, store = run
    c = problem_of(name)
    p, Z, mu = c["p"], c["Z"], c["mu"]
    shift = steps(name, store)["shift"]
    v = R.free_direction(p, np.random.default_rng(8))
    ev = evaluator(c, store)
    try:
        ev.reduced_lagrangian_gradient(Z, SIGMA, mu)
        first = ev.reduced_hessian_product(Z, v, SIGMA, mu)      # the Hessian point at mu~ is built by the first product
        ev.profile_enable(True)
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, v, SIGMA, mu), first)
        one, none = launches(ev, PRODUCT_NAMES), launches(ev, REBUILD_NAMES)
        assert none == (0,) * len(REBUILD_NAMES) and launches(ev, ("newton",)) == (0,)
        ev.profile_reset()
        x, info = ev.reduced_newton_step(Z, SIGMA, mu, shift=shift, rtol=1e-8, max_iter=40)
        k = info["iterations"]
        ms, n_newton, nbytes = ev.profile_get("newton")
        print(run_id(run), "iterations", k, "launches of one product", dict(zip(PRODUCT_NAMES, one)), "newton", n_newton, "bytes", nbytes, "ms", ms)
        assert info["status"] == CONVERGED and k >= 2
        assert launches(ev, PRODUCT_NAMES) == tuple(k * n for n in one), "k kept-point single products"
        assert launches(ev, REBUILD_NAMES) == none, "no chain, tree-build or assembly launch"
        assert n_newton == 2 + 3 * k and nbytes > 0, "start and its closing launch, then three per iteration; bytes as executed"
        ev.profile_reset()
        assert np.array_equal(ev.reduced_hessian_product(Z, v, SIGMA, mu), first)
        assert launches(ev, PRODUCT_NAMES) == one and launches(ev, REBUILD_NAMES) == none, "a following product is at its kept point"
        ev.profile_enable(False)
    finally:
        ev.close()


# ------------------------------------------------------------------------------------------------------------------ loop
@pytest.mark.parametrize("name", ["scaled_12x9", "scaled_12x9+con"])
def test_a_trust_region_loop_descends(name):
    """ten trials of the textbook loop over feasible_merit and reduced_newton_step; the oracle's run of it went 28.96 -> 7.87 with 8
    accepted trials (scaled_12x9) and 27.54 -> -0.62 with 10 accepted (+con)"""
    c = R.case(name)
    mu = c["mu"]
    ev = evaluator(c, 0)
    try:
        Z = ev.feasible_trajectory_engine(c["Z"])
        phi0 = phi = ev.feasible_merit(Z, SIGMA, mu)
        delta, accepted = 1.0, 0
        for trial in range(10):
            x, info = ev.reduced_newton_step(Z, SIGMA, mu, radius=delta, rtol=1e-6)
            phi_t, Z_t = ev.feasible_merit(Z + x, SIGMA, mu, trajectory=True)
            rho = (phi - phi_t) / info["predicted"]
            print(name, "trial", trial, "delta", delta, "status", info["status"], "iterations", info["iterations"], "predicted", info["predicted"],
                  "phi", phi, "->", phi_t, "rho", rho)
            if rho > 0.1:
                assert info["predicted"] > 0
                Z, phi, accepted = Z_t, phi_t, accepted + 1
            if rho < 0.25:
                delta /= 4.0
            elif rho > 0.75 and info["status"] != CONVERGED:
                delta *= 2.0
    finally:
        ev.close()
    print(name, "phi", phi0, "->", phi, "accepted", accepted)
    assert accepted >= 5
    assert phi < (phi0 - 0.5 * abs(phi0) if name.endswith("+con") else 0.5 * phi0)


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_a_device_handle_leave_nothing_written_and_the_handle_usable():
    c = R.case("scaled_12x9")
    Z = c["Z"]
    ev = dto_amd.Evaluator(c["pe"], k_lo=1, k_hi=3)                # a sharded handle: what the single product refuses
    try:
        with pytest.raises(dto_amd.EngineError, match="dto_projected_newton_step needs an unsharded handle"):
            ev.reduced_newton_step(Z)
    finally:
        ev.close()
    ev = dto_amd.Evaluator(c["pe"], eval_hessian=False)
    try:
        with pytest.raises(dto_amd.EngineError, match="eval_hessian = 0"):
            ev.reduced_newton_step(Z)
        assert not np.isnan(ev.reduced_lagrangian_gradient(Z, SIGMA)).any()
    finally:
        ev.close()
    ev = evaluator(c, 0)
    try:
        ev.profile_enable(True)
        for kw, word in ((dict(max_iter=0), "max_iter"), (dict(radius=-1.0), "radius"), (dict(rtol=math.nan), "rtol"), (dict(shift=math.inf), "shift")):
            with pytest.raises(dto_amd.EngineError, match=word):
                ev.reduced_newton_step(Z, SIGMA, **kw)
        assert ev.profile_get("newton")[1] == 0 and ev.profile_get("all")[1] == 0, "nothing was enqueued"
        ev.profile_enable(False)
        s = steps("scaled_12x9", 0)
        same_bits(ev.reduced_newton_step(Z, SIGMA, None, shift=s["shift"], rtol=1e-8, max_iter=40, trace=True),
                  (s["converged"][0][0], s["converged"][0][1]["raw"], s["converged"][0][2]), "after the refusals")
    finally:
        ev.close()
