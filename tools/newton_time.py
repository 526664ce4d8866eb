#!/usr/bin/env python3
"""The truncated-Newton step as one engine call (Evaluator.reduced_newton_step_dev) beside the same CG written by hand around
reduced_hessian_product_dev with torch reductions, timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process, on ``synthetic.multi_ket_problem(n, 1, drives, N, scale)`` -- one ket with skew-symmetric generators, its
DerivativeIntegrator(u, du) and the knot constraint on u -- with option "reduced_input_store" = 1, at the kept point of
(Z, sigma = 0.7, a random mu), device-resident inputs and outputs.  shift = 2 max |Rayleigh quotient| over 8 power iterations with the
engine's product, so A = M T'HT M + shift M is positive definite with a condition number of at most 3; rtol = 0, so both loops run
exactly ``max_iter`` iterations (10 and 30) and end with MAX_ITER.

The YARDSTICK is what a user writes today: per iteration one reduced_hessian_product_dev (which checks its kept points: two 4-byte
readbacks on this route), w = mask * (y + shift d), torch.dot for kappa and rr', alpha and beta as Python floats (.item(): a host
synchronisation each) -- the existing code, not the code under test.  Its result agrees with the engine's to rounding, not to the bit:
torch's reduction order is its own.

After a warm-up of at least 30 ms of GPU work per member, single calls ALTERNATE (yardstick, engine step, yardstick, ...); medians of
``--reps`` each with the yardstick's min .. max.  Beside them: the median of a kept-point reduced_hessian_product_dev alone, the
"newton" profile name of one step (device milliseconds, launches and bytes, and both per iteration), and
    step_minus_products_ms = step - max_iter x product        (what the step costs beyond its products: the "newton" kernels, the
                                                               readbacks, and the point checks it does NOT repeat count negative)

A/B of how the step sums the chunk sums of its dots, one process per form on the TUNING library; the line says which
form ran ("combine_form"):

    DTO_ENGINE_LIB=libdto_engine_t.so DTO_NEWTON_COMBINE=0 python tools/newton_time.py   # every workgroup for itself (the engine's form)
    DTO_ENGINE_LIB=libdto_engine_t.so DTO_NEWTON_COMBINE=1 python tools/newton_time.py   # a one-workgroup launch of its own

``--box`` measures the bound-constrained step (Evaluator.reduced_newton_step_box_dev) instead, in the same way.  The YARDSTICK is then
the existing step (reduced_newton_step_dev) with its min .. max; beside it, calls alternating,
    box_inf:     the box step with lo = -inf and hi = +inf vectors (the same iterations, bit for bit, plus the box's own traffic)
    box_finite:  the box step inside Z -+ half the largest entry of the unbounded step's p on the independent entries
each with the "newton_box" profile name of one call (device milliseconds, launches, bytes, and both per iteration), the yardstick with
its "newton" profile, and
    excess_ms = (box step - yardstick) - (newton_box device ms - newton device ms) - (yardstick max - yardstick min)
-- what of the difference neither the kernels' own device time nor the yardstick's spread explains (negative: nothing).

``--auglag`` measures the augmented-Lagrangian step (Evaluator.auglag_newton_step_dev) with rho = 10 on the rows of the tool's knot
constraint and infinite bounds, in the same way.  The YARDSTICK is the box step (reduced_newton_step_box_dev) at the same (Z, sigma, mu):
another operator (the step adds the Gauss-Newton term and works at mu_eff), so the iterates differ; both run exactly ``max_iter``
iterations (rtol = 0, shift from the power iterations with the augmented operator).  Beside the two medians: the "auglag" profile name
of one call (device milliseconds, launches, bytes, and all three per iteration), the yardstick's "newton_box" profile, the active rows, and
    excess_ms = (auglag step - yardstick) - auglag device ms - (yardstick max - yardstick min)

``--minimize`` measures the reduced-space minimize call (Evaluator.reduced_minimize_dev, ten trials, no bounds, no penalties, the
tool's shift, rtol = 1e-6, max_iter = the largest of ``--iters``) beside the same loop written in Python over the existing _dev entry
points -- the step, the merit, torch ``.item()`` reads of the step's info and of phi, the decisions on the host: what a user wrote before
the call existed.  Calls alternate, medians of ``--reps`` with the yardstick's min .. max; ms per trial for both, the "minimize" profile
name's device time and bytes per trial, and whether the call's time is at most the yardstick's plus that device time plus the yardstick's
spread.  Then, with "newton_pairs" = 8, ``harvest=True`` against capacity 0 on the same run: total CG iterations and ms over the trials.

``--precond`` measures the L-BFGS-preconditioned step (Evaluator.preconditioned_newton_step_dev, option "newton_pairs" = 8) without
bounds.  The YARDSTICK is the box step (reduced_newton_step_box_dev); rtol = 0, so every call runs exactly ``max_iter`` iterations.
Beside it, calls alternating,
    empty:      the new step with an empty store (the box step's iterations bit for bit: what the new loop's own launches cost)
    pairs_8:    the new step with the 8 pairs a harvesting call left at the same point (the application's cost on top)
each with the "precond" profile name of one call and the yardstick's "newton_box" profile.  Then ``to_rtol``: at rtol = 1e-6, for the
tool's shift and for 0.55 of it, the iterations, the status and the median wall time of the box step, of the new step with an empty
store, and of the new step with the 8 pairs harvested by a previous call at the same point and shift.

One JSON line per shape.

    python tools/newton_time.py                       # 256 x 2000 and 64 x 1000
    python tools/newton_time.py --box                 # the bound-constrained step beside the existing one
    python tools/newton_time.py --auglag              # the augmented-Lagrangian step beside the bound-constrained one
    python tools/newton_time.py --precond             # the preconditioned step beside the bound-constrained one
    python tools/newton_time.py --minimize            # the one-call trust-region loop beside the loop over the _dev entry points
    python tools/newton_time.py --shapes 128x1000 --reps 9 --iters 10,30
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dto_amd  # noqa: E402

SIGMA = 0.7


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternating(yardstick, call, reps):
    """medians of `reps` single calls each, the two alternating; the yardstick's spread"""
    for fn in (yardstick, call):
        spent = 0.0
        while spent < 30.0:          # warm-up: at least 30 ms of work
            spent += event_ms(fn)
    ys, cs = [], []
    for _ in range(reps):
        ys.append(event_ms(yardstick))
        cs.append(event_ms(call))
    return {"yardstick_ms": round(statistics.median(ys), 4), "step_ms": round(statistics.median(cs), 4),
            "yardstick_min_ms": round(min(ys), 4), "yardstick_max_ms": round(max(ys), 4),
            "step_min_ms": round(min(cs), 4), "step_max_ms": round(max(cs), 4),
            "difference_ms": round(statistics.median(cs) - statistics.median(ys), 4)}


def measure_box(n, N, drives, scale, reps, iters):
    """the bound-constrained step beside the existing step (the yardstick): infinite bounds, then a finite box"""
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob)
    ev.set_option("reduced_input_store", 1)
    out = {"mode": "box", "n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps, "sigma": SIGMA, "route": "reduced_input_store"}
    try:
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Z = torch.from_numpy(Zh).to(dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        mu = torch.randn(ev.n_constraints, dtype=torch.float64, device=dev, generator=gen)
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        nv = ev.n_variables
        g, y, p, info, pb, info_b = f64(nv), f64(nv), f64(nv), f64(8), f64(nv), f64(12)
        free = torch.from_numpy(ev.independent_entries()).to(dev)
        mask = torch.zeros(nv, dtype=torch.float64, device=dev)
        mask[free] = 1.0
        out["n_variables"], out["chunks"] = nv, -(-nv // 256)
        ev.reduced_gradient_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), g.data_ptr(), 0, st)
        v = torch.randn(nv, dtype=torch.float64, device=dev, generator=gen) * mask
        top = 0.0
        for _ in range(8):
            v = v / torch.linalg.norm(v)
            ev.reduced_hessian_product_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), v.data_ptr(), y.data_ptr(), st)
            top = max(top, abs(float(torch.dot(v, y))))
            v = y.clone()
        shift = 2.0 * top
        out["shift"] = shift
        lo_inf, hi_inf = torch.full_like(Z, float("-inf")), torch.full_like(Z, float("inf"))

        def profile(name, fn, max_iter):
            ev.profile_enable(True); ev.profile_reset(); fn(); torch.cuda.synchronize()
            ms, launches, nbytes = ev.profile_get(name)
            ev.profile_enable(False)
            return {"ms": round(ms, 4), "launches": launches, "bytes": nbytes, "ms_per_iteration": round(ms / max_iter, 5),
                    "bytes_per_iteration": nbytes / max_iter}

        for max_iter in iters:
            step = lambda: ev.reduced_newton_step_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), 0, 0.0, shift, 0.0, 0.0, max_iter, p.data_ptr(),
                                                      info.data_ptr(), 0, st)
            box = lambda lo, hi: (lambda: ev.reduced_newton_step_box_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), 0, lo.data_ptr(), hi.data_ptr(), 0.0,
                                                                         shift, 0.0, 0.0, max_iter, pb.data_ptr(), info_b.data_ptr(), 0, 0, 0, st))
            step(); torch.cuda.synchronize()
            half = 0.5 * float(torch.max(torch.abs(p)))
            lo_f, hi_f = lo_inf.clone(), hi_inf.clone()
            lo_f[free], hi_f[free] = Z[free] - half, Z[free] + half
            res = {"half_width": half}
            for key, fn in (("box_inf", box(lo_inf, hi_inf)), ("box_finite", box(lo_f, hi_f))):
                pair = alternating(step, fn, reps)
                fn(); torch.cuda.synchronize()
                raw = info_b.cpu().numpy()
                pair.update(status=int(raw[0]), iterations=int(raw[1]), held=int(raw[8]), hit=int(raw[9]), restarts=int(raw[10]), n_free=int(raw[11]))
                if key == "box_inf":
                    pair["same_bits_as_yardstick"] = bool(torch.equal(pb, p))
                pair["newton_box_profile"] = profile("newton_box", fn, max_iter)
                pair["yardstick_newton_profile"] = profile("newton", step, max_iter)
                pair["excess_ms"] = round(pair["difference_ms"] - (pair["newton_box_profile"]["ms"] - pair["yardstick_newton_profile"]["ms"])
                                          - (pair["yardstick_max_ms"] - pair["yardstick_min_ms"]), 4)
                res[key] = pair
            out[f"max_iter_{max_iter}"] = res
        return out
    finally:
        ev.close()


def measure_auglag(n, N, drives, scale, reps, iters, rho_value=10.0):
    """the augmented-Lagrangian step beside the box step (the yardstick), infinite bounds, rho on the knot constraint's rows"""
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob)
    ev.set_option("reduced_input_store", 1)
    out = {"mode": "auglag", "n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps, "sigma": SIGMA, "rho": rho_value,
           "route": "reduced_input_store"}
    try:
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Z = torch.from_numpy(Zh).to(dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        mu = torch.randn(ev.n_constraints, dtype=torch.float64, device=dev, generator=gen)
        rho = torch.from_numpy(prob.penalty_vector(rho_value)).to(dev)
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        nv = ev.n_variables
        y, p, info, pa, info_a, rows_info = f64(1, nv), f64(nv), f64(12), f64(nv), f64(12), f64(8)
        mask = torch.zeros(nv, dtype=torch.float64, device=dev)
        mask[torch.from_numpy(ev.independent_entries()).to(dev)] = 1.0
        out["n_variables"], out["chunks"], out["rows"] = nv, -(-nv // 256), ev.n_constraints - ev.n_dynamics_constraints
        ev.auglag_rows_dev(Z.data_ptr(), mu.data_ptr(), rho.data_ptr(), 0, 0, rows_info.data_ptr(), st)
        torch.cuda.synchronize()
        out["active_rows"], out["max_viol"] = int(rows_info[1]), float(rows_info[2])
        v = (torch.randn(nv, dtype=torch.float64, device=dev, generator=gen) * mask).reshape(1, nv)
        top = 0.0
        for _ in range(8):
            v = v / torch.linalg.norm(v)
            ev.auglag_hessian_products_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), rho.data_ptr(), 1, v.data_ptr(), y.data_ptr(), st)
            top = max(top, abs(float(torch.sum(v * y))))
            v = y.clone()
        shift = 2.0 * top
        out["shift"] = shift

        def profile(name, fn, max_iter):
            ev.profile_enable(True); ev.profile_reset(); fn(); torch.cuda.synchronize()
            ms, launches, nbytes = ev.profile_get(name)
            ev.profile_enable(False)
            return {"ms": round(ms, 4), "launches": launches, "bytes": nbytes, "ms_per_iteration": round(ms / max_iter, 5),
                    "launches_per_iteration": launches / max_iter, "bytes_per_iteration": nbytes / max_iter}

        for max_iter in iters:
            box = lambda: ev.reduced_newton_step_box_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), 0, 0, 0, 0.0, shift, 0.0, 0.0, max_iter, p.data_ptr(),
                                                         info.data_ptr(), 0, 0, 0, st)
            al = lambda: ev.auglag_newton_step_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), rho.data_ptr(), 0, 0, 0, 0.0, shift, 0.0, 0.0, max_iter,
                                                   pa.data_ptr(), info_a.data_ptr(), 0, 0, 0, st)
            pair = alternating(box, al, reps)
            al(); torch.cuda.synchronize()
            raw = info_a.cpu().numpy()
            pair.update(status=int(raw[0]), iterations=int(raw[1]))
            pair["auglag_profile"] = profile("auglag", al, max_iter)
            pair["yardstick_newton_box_profile"] = profile("newton_box", box, max_iter)
            pair["excess_ms"] = round(pair["difference_ms"] - pair["auglag_profile"]["ms"] - (pair["yardstick_max_ms"] - pair["yardstick_min_ms"]), 4)
            out[f"max_iter_{max_iter}"] = pair
        return out
    finally:
        ev.close()


def measure_precond(n, N, drives, scale, reps, iters, m=8):
    """the preconditioned step beside the box step (the yardstick), no bounds: an empty store, then 8 harvested pairs"""
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob)
    ev.set_option("reduced_input_store", 1)
    ev.set_option("newton_pairs", m)
    out = {"mode": "precond", "n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps, "sigma": SIGMA, "newton_pairs": m,
           "route": "reduced_input_store"}
    try:
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Z = torch.from_numpy(Zh).to(dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        mu = torch.randn(ev.n_constraints, dtype=torch.float64, device=dev, generator=gen)
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        nv = ev.n_variables
        y, p, info, pp, info_p = f64(nv), f64(nv), f64(12), f64(nv), f64(16)
        mask = torch.zeros(nv, dtype=torch.float64, device=dev)
        mask[torch.from_numpy(ev.independent_entries()).to(dev)] = 1.0
        out["n_variables"], out["chunks"] = nv, -(-nv // 256)
        v = torch.randn(nv, dtype=torch.float64, device=dev, generator=gen) * mask
        top = 0.0
        for _ in range(8):
            v = v / torch.linalg.norm(v)
            ev.reduced_hessian_product_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), v.data_ptr(), y.data_ptr(), st)
            top = max(top, abs(float(torch.dot(v, y))))
            v = y.clone()
        shift = 2.0 * top
        out["shift"] = shift

        def profile(name, fn, max_iter):
            ev.profile_enable(True); ev.profile_reset(); fn(); torch.cuda.synchronize()
            ms, launches, nbytes = ev.profile_get(name)
            ev.profile_enable(False)
            return {"ms": round(ms, 4), "launches": launches, "bytes": nbytes, "ms_per_iteration": round(ms / max_iter, 5),
                    "launches_per_iteration": launches / max_iter, "bytes_per_iteration": nbytes / max_iter}

        def box(sh, rtol, max_iter):
            return lambda: ev.reduced_newton_step_box_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), 0, 0, 0, 0.0, sh, rtol, 0.0, max_iter, p.data_ptr(),
                                                          info.data_ptr(), 0, 0, 0, st)

        def pre(sh, rtol, max_iter, harvest=False):
            return lambda: ev.preconditioned_newton_step_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), 0, 0, 0, 0, 0.0, sh, rtol, 0.0, max_iter, harvest,
                                                             pp.data_ptr(), info_p.data_ptr(), 0, 0, 0, st)

        def harvest(sh):
            ev.newton_pairs_clear()
            pre(sh, 0.0, m, harvest=True)()
            torch.cuda.synchronize()
            return ev.newton_pairs_info()[0]

        for max_iter in iters:
            res = {}
            for key in ("empty", "pairs_8"):
                ev.newton_pairs_clear()
                if key == "pairs_8":
                    res["pairs_in_store"] = harvest(shift)
                fn = pre(shift, 0.0, max_iter)
                pair = alternating(box(shift, 0.0, max_iter), fn, reps)
                fn(); torch.cuda.synchronize()
                raw = info_p.cpu().numpy()
                pair.update(status=int(raw[0]), iterations=int(raw[1]), admitted=int(raw[12]), fallbacks=int(raw[14]),
                            rnorm_over_gnorm=float(raw[3] / raw[2]))
                pair["difference_ms_per_iteration"] = round(pair["difference_ms"] / max_iter, 5)
                if key == "empty":
                    box(shift, 0.0, max_iter)(); torch.cuda.synchronize()
                    pair["same_bits_as_yardstick"] = bool(torch.equal(pp, p))
                pair["precond_profile"] = profile("precond", fn, max_iter)
                pair["yardstick_newton_box_profile"] = profile("newton_box", box(shift, 0.0, max_iter), max_iter)
                res[key] = pair
            out[f"max_iter_{max_iter}"] = res
        to_rtol = {}
        for factor in (1.0, 0.55):
            sh, cap = factor * shift, 200

            def timed(fn, raw_of):
                for _ in range(2):
                    event_ms(fn)
                ms = statistics.median(event_ms(fn) for _ in range(reps))
                raw = raw_of.cpu().numpy()
                return {"ms": round(ms, 4), "status": int(raw[0]), "iterations": int(raw[1]), "rnorm_over_gnorm": float(raw[3] / raw[2])}

            row = {"shift": sh, "box": timed(box(sh, 1e-6, cap), info)}
            ev.newton_pairs_clear()
            row["empty"] = timed(pre(sh, 1e-6, cap), info_p)
            row["pairs_in_store"] = harvest(sh)
            row["pairs_8"] = timed(pre(sh, 1e-6, cap), info_p)
            row["pairs_8"]["admitted"] = int(info_p.cpu().numpy()[12])
            to_rtol[f"shift_x{factor}"] = row
        out["to_rtol_1e-6"] = to_rtol
        return out
    finally:
        ev.close()


def measure_minimize(n, N, drives, scale, reps, iters, m=8, trials=10):
    """the one-call trust-region loop (Evaluator.reduced_minimize_dev) beside the same loop written in Python over the _dev entry points
    with torch .item() reads (the yardstick), no bounds, no penalties; then harvested pairs against capacity 0 on the same run"""
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob)
    ev.set_option("reduced_input_store", 1)
    out = {"mode": "minimize", "n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps, "sigma": SIGMA, "trials": trials,
           "route": "reduced_input_store"}
    try:
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Z0 = torch.from_numpy(Zh).to(dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        mu = torch.randn(ev.n_constraints, dtype=torch.float64, device=dev, generator=gen)
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        nv = ev.n_variables
        y, p, Zc, Zp, Zt, info, minfo, dphi, dphit = f64(nv), f64(nv), f64(nv), f64(nv), f64(nv), f64(16), f64(16), f64(1), f64(1)
        mask = torch.zeros(nv, dtype=torch.float64, device=dev)
        mask[torch.from_numpy(ev.independent_entries()).to(dev)] = 1.0
        out["n_variables"], out["chunks"] = nv, -(-nv // 256)
        v = torch.randn(nv, dtype=torch.float64, device=dev, generator=gen) * mask
        top = 0.0
        for _ in range(8):
            v = v / torch.linalg.norm(v)
            ev.reduced_hessian_product_dev(Z0.data_ptr(), SIGMA, mu.data_ptr(), v.data_ptr(), y.data_ptr(), st)
            top = max(top, abs(float(torch.dot(v, y))))
            v = y.clone()
        shift = 2.0 * top
        out["shift"] = shift
        max_iter = max(iters)
        out["max_iter"] = max_iter
        log = {}

        def hand(harvest=False):
            """the loop a user writes today: the engine's step and merit on device pointers, the decisions on the host"""
            pairs = ev.newton_pairs_info()[1] > 0
            Zc.copy_(Z0)
            ev.feasible_merit_dev(Zc.data_ptr(), SIGMA, mu.data_ptr(), dphi.data_ptr(), Zc.data_ptr(), 0, st)
            phi, delta, cg, acc = dphi.item(), 1.0, 0, 0
            for _ in range(trials):
                if pairs:
                    ev.preconditioned_newton_step_dev(Zc.data_ptr(), SIGMA, mu.data_ptr(), 0, 0, 0, 0, delta, shift, 1e-6, 0.0, max_iter, harvest,
                                                      p.data_ptr(), info.data_ptr(), 0, 0, Zp.data_ptr(), st)
                else:
                    ev.reduced_newton_step_box_dev(Zc.data_ptr(), SIGMA, mu.data_ptr(), 0, 0, 0, delta, shift, 1e-6, 0.0, max_iter, p.data_ptr(),
                                                   info.data_ptr(), 0, 0, Zp.data_ptr(), st)
                status, its, predicted = info[0].item(), info[1].item(), info[6].item()
                ev.feasible_merit_dev(Zp.data_ptr(), SIGMA, mu.data_ptr(), dphit.data_ptr(), Zt.data_ptr(), 0, st)
                phi_t = dphit.item()
                ratio = (phi - phi_t) / predicted
                cg += int(its)
                if ratio > 0.1:
                    Zc.copy_(Zt)
                    phi, acc = phi_t, acc + 1
                if ratio < 0.25:
                    delta /= 4
                elif ratio > 0.75 and status != dto_amd.capi.NEWTON_CONVERGED:
                    delta *= 2
            log["hand"] = dict(phi=phi, iterations=cg, accepted=acc)

        def call(harvest=False):
            Zc.copy_(Z0)
            ev.reduced_minimize_dev(Zc.data_ptr(), SIGMA, mu.data_ptr(), 0, 0, 0, 0, 1, trials, harvest, minfo.data_ptr(), stream=st, shift=shift,
                                    max_iter=max_iter)

        pair = alternating(hand, call, reps)
        hand(); call(); torch.cuda.synchronize()
        raw = minfo.cpu().numpy()
        pair.update(status=int(raw[0]), trials_run=int(raw[2]), accepted=int(raw[3]), iterations=int(raw[11]), phi_first=float(raw[4]), phi=float(raw[5]),
                    yardstick=log["hand"], same_phi_as_yardstick=bool(raw[5] == log["hand"]["phi"]))
        k = max(int(raw[2]), 1)
        ev.profile_enable(True); ev.profile_reset(); call(); torch.cuda.synchronize()
        ms, launches, nbytes = ev.profile_get("minimize")
        ev.profile_enable(False)
        pair["minimize_profile"] = {"ms": round(ms, 4), "launches": launches, "bytes": nbytes, "ms_per_trial": round(ms / k, 5), "bytes_per_trial": nbytes / k}
        pair["yardstick_ms_per_trial"], pair["call_ms_per_trial"] = round(pair["yardstick_ms"] / trials, 4), round(pair["step_ms"] / k, 4)
        spread = pair["yardstick_max_ms"] - pair["yardstick_min_ms"]
        pair["claim_call_le_yardstick_plus_minimize_plus_spread"] = bool(pair["step_ms"] <= pair["yardstick_ms"] + ms + spread)
        out["loop"] = pair
        # harvested pairs against capacity 0 on the same run: total CG iterations and wall time of the one call
        res = {}
        for key, cap, harvest in (("capacity_0", 0, False), (f"pairs_{m}_harvest", m, True)):
            ev.set_option("newton_pairs", cap)
            fn = lambda: (ev.newton_pairs_clear(), call(harvest))
            for _ in range(2):
                event_ms(fn)
            t = [event_ms(fn) for _ in range(reps)]
            raw = minfo.cpu().numpy()
            res[key] = {"ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "iterations": int(raw[11]),
                        "accepted": int(raw[3]), "harvested": int(raw[12]), "fallbacks": int(raw[13]), "phi": float(raw[5]), "status": int(raw[0])}
        ev.set_option("newton_pairs", 0)
        out["harvest_over_trials"] = res
        return out
    finally:
        ev.close()


def measure(n, N, drives, scale, reps, iters):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob)
    ev.set_option("reduced_input_store", 1)
    tuning = "_t" in os.environ.get("DTO_ENGINE_LIB", "")   # the product library reads no environment variable
    form = "own_launch" if tuning and os.environ.get("DTO_NEWTON_COMBINE", "0") not in ("", "0") else "every_workgroup"
    out = {"n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps, "sigma": SIGMA, "route": "reduced_input_store",
           "combine_form": form}
    try:
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Z = torch.from_numpy(Zh).to(dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        mu = torch.randn(ev.n_constraints, dtype=torch.float64, device=dev, generator=gen)
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        nv = ev.n_variables
        g, y, p, info = f64(nv), f64(nv), f64(nv), f64(8)
        mask = torch.zeros(nv, dtype=torch.float64, device=dev)
        mask[torch.from_numpy(ev.independent_entries()).to(dev)] = 1.0
        out["n_variables"], out["chunks"] = nv, -(-nv // 256)
        prod = lambda v, o: ev.reduced_hessian_product_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), v.data_ptr(), o.data_ptr(), st)
        ev.reduced_gradient_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), g.data_ptr(), 0, st)
        v = torch.randn(nv, dtype=torch.float64, device=dev, generator=gen) * mask
        top = 0.0
        for _ in range(8):
            v = v / torch.linalg.norm(v)
            prod(v, y)
            top = max(top, abs(float(torch.dot(v, y))))
            v = y.clone()
        shift = 2.0 * top
        out["shift"] = shift

        def product_alone():
            prod(v, y)

        for _ in range(5):
            event_ms(product_alone)
        out["product_kept_ms"] = round(statistics.median(event_ms(product_alone) for _ in range(reps)), 4)

        def hand(max_iter):
            """the CG a user writes today: the engine's product, torch reductions, decisions on the host"""
            r = g * mask
            x = torch.zeros_like(r)
            d = -r
            rr = torch.dot(r, r).item()
            for _ in range(max_iter):
                prod(d, y)
                w = mask * (y + shift * d)
                kappa = torch.dot(d, w).item()
                if not kappa > 0.0:
                    break
                alpha = rr / kappa
                x += alpha * d
                r += alpha * w
                rr_new = torch.dot(r, r).item()
                d = (rr_new / rr) * d - r
                rr = rr_new
            return x

        for max_iter in iters:
            step = lambda: ev.reduced_newton_step_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), 0, 0.0, shift, 0.0, 0.0, max_iter, p.data_ptr(),
                                                      info.data_ptr(), 0, st)
            pair = alternating(lambda: hand(max_iter), step, reps)
            x = hand(max_iter)
            step(); torch.cuda.synchronize()
            raw = info.cpu().numpy()
            pair["status"], pair["iterations"] = int(raw[0]), int(raw[1])
            pair["step_against_yardstick_relative"] = float(torch.linalg.norm(p - x) / torch.linalg.norm(x))
            ev.profile_enable(True); ev.profile_reset(); step(); torch.cuda.synchronize()
            ms, launches, nbytes = ev.profile_get("newton")
            ev.profile_enable(False)
            pair["newton_profile"] = {"ms": round(ms, 4), "launches": launches, "bytes": nbytes, "ms_per_iteration": round(ms / max_iter, 5),
                                      "bytes_per_iteration": nbytes / max_iter}
            pair["step_minus_products_ms"] = round(pair["step_ms"] - max_iter * out["product_kept_ms"], 4)
            out[f"max_iter_{max_iter}"] = pair
        return out
    finally:
        ev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="256x2000,64x1000", help="comma-separated states x knots")
    ap.add_argument("--drives", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", default="10,30", help="comma-separated iteration counts")
    ap.add_argument("--scale", type=float, default=1.0, help="standard deviation of the generators' entries (1.0: the norms of the\n"
                    "headline benchmark; 0: 1 / sqrt(n), norms of order one)")
    ap.add_argument("--box", action="store_true", help="measure the bound-constrained step beside the existing step")
    ap.add_argument("--auglag", action="store_true", help="measure the augmented-Lagrangian step beside the bound-constrained step")
    ap.add_argument("--precond", action="store_true", help="measure the L-BFGS-preconditioned step beside the bound-constrained step")
    ap.add_argument("--minimize", action="store_true", help="measure the one-call trust-region loop beside the loop over the _dev entry points")
    a = ap.parse_args()
    run = measure_minimize if a.minimize else measure_precond if a.precond else measure_auglag if a.auglag else measure_box if a.box else measure
    for s in a.shapes.split(","):
        n, N = (int(x) for x in s.lower().split("x"))
        print(json.dumps(run(n, N, a.drives, a.scale, a.reps, [int(i) for i in a.iters.split(",")])), flush=True)


if __name__ == "__main__":
    main()
