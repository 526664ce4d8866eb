#!/usr/bin/env python3
"""Replicated-block generators (Evaluator(..., block_generators=True)) against the dense path on the same unitary problem,
timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process: a flagged and an unflagged handle on ``synthetic.unitary_problem(levels, drives=4, N)``; device-resident
inputs and outputs; eval_constraint, eval_constraint_jacobian and eval_hessian_lagrangian, each after a warm-up of at least 30 ms of
GPU work (the chip ramps for about that long); the median of ``--reps`` single-call timings.  The unflagged handle runs the dense
path untouched: it is the yardstick.  For the structured handle the line also gives the kernel time, the priced FP64 rate of the
sweep launches (dto_profile_get "expmv" / "expmv_adjoint") and the rate at which the value slab is produced (slab bytes / call time).
One JSON line per shape.

    python tools/kron_time.py                          # levels 8 x 1000 knots (n = 128), 16 x 500 (n = 512)
    python tools/kron_time.py --shapes 32x40 --dense 0 # n = 2048 (b = 64): the structured handle alone
    python tools/kron_time.py --objective-block 1      # also the Hessian at sigma = 0 and the difference: the objective's share
    python tools/kron_time.py --minimum-time 1         # synthetic.unitary_minimum_time_problem instead: the built-in quadratic-form
                                                       # fidelity bound (device-resident and through host pointers) against the same
                                                       # bound as a host-merged closure (host pointers: its blocks come from the host)
    python tools/kron_time.py --products 1             # also J w and J' w on both handles: through host pointers (wall clock, the
                                                       # copies included) and, where the library has them, the device-pointer
                                                       # entry points (HIP events), with the kernel time of "jac_product"
    python tools/kron_time.py --products 1 --small 4x1000   # the same two products on a small-path handle (states x knots)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dto_amd  # noqa: E402


def one_call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps):
    spent = 0.0
    while spent < 30.0:          # warm-up: at least 30 ms of GPU work
        spent += one_call_ms(fn)
    return statistics.median(one_call_ms(fn) for _ in range(reps))


def host_timed(fn, reps):
    """Median wall-clock milliseconds of a blocking host-pointer callback (host evaluation of closures and copies included)."""
    fn(); fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def measure_host(prob, flagged, reps, sigma=0.7):
    """eval_constraint, Jacobian and Hessian through host pointers (what a closure-based term forces)."""
    import numpy as np
    ev = dto_amd.Evaluator(prob, eval_hessian=True, block_generators=flagged)
    try:
        Z = prob.trajectory.vec()
        mu = np.random.default_rng(1).standard_normal(ev.n_constraints)
        g, J, H = np.empty(ev.n_constraints), np.empty(ev.n_jacobian_entries), np.empty(ev.n_hessian_entries)
        return {"constraint_ms": round(host_timed(lambda: ev.eval_constraint(g, Z), reps), 4),
                "jacobian_ms": round(host_timed(lambda: ev.eval_constraint_jacobian(J, Z), reps), 4),
                "hessian_ms": round(host_timed(lambda: ev.eval_hessian_lagrangian(H, Z, sigma, mu), reps), 4)}
    finally:
        ev.close()


def measure_products(prob, flagged, reps):
    """J w and J' w: host-pointer calls (wall clock) and the device-pointer entry points (HIP events) where the library exports them."""
    import numpy as np
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ev = dto_amd.Evaluator(prob, eval_hessian=True, block_generators=flagged)
    try:
        rng = np.random.default_rng(1)
        Z = prob.trajectory.vec()
        w, wt = rng.standard_normal(ev.n_variables), rng.standard_normal(ev.n_constraints)
        y, t = np.empty(ev.n_constraints), np.empty(ev.n_variables)
        out = {"Jw_host_ms": round(host_timed(lambda: ev.eval_constraint_jacobian_product(y, Z, w), reps), 4),
               "JTw_host_ms": round(host_timed(lambda: ev.eval_constraint_jacobian_transpose_product(t, Z, wt), reps), 4)}
        if not hasattr(ev._lib, "dto_eval_jacobian_product_dev"):
            return out
        dZ, dw, dwt = (torch.from_numpy(a).to(dev) for a in (Z, w, wt))
        dy = torch.empty(ev.n_constraints, dtype=torch.float64, device=dev)
        dt_ = torch.empty(ev.n_variables, dtype=torch.float64, device=dev)
        jw = lambda: ev.eval_jacobian_product_dev(dZ.data_ptr(), dw.data_ptr(), dy.data_ptr(), st)
        jtw = lambda: ev.eval_jacobian_transpose_product_dev(dZ.data_ptr(), dwt.data_ptr(), dt_.data_ptr(), st)
        out["Jw_dev_ms"] = round(timed(jw, reps), 4)
        out["JTw_dev_ms"] = round(timed(jtw, reps), 4)
        for name, fn in (("Jw", jw), ("JTw", jtw)):
            ev.profile_enable(True); ev.profile_reset(); fn(); torch.cuda.synchronize()
            ms, n, fl = ev.profile_get("jac_product")
            out[name + "_kernel_ms"] = round(ms, 4)
            out[name + "_kernel_launches"] = n
            out[name + "_kernel_TFLOPs"] = round(fl / ms * 1e-9, 3) if ms > 0 else None
            out[name + "_zero_fill_launches"] = ev.profile_get("zero_fill")[1]
            ev.profile_enable(False)
        return out
    finally:
        ev.close()


def measure_handle(prob, flagged, reps, sigma=0.7, objective_block=False):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ev = dto_amd.Evaluator(prob, eval_hessian=True, block_generators=flagged)
    try:
        g = torch.Generator(device="cpu").manual_seed(1)
        Z = torch.from_numpy(prob.trajectory.vec()).to(dev)
        mu = torch.randn(ev.n_constraints, generator=g, dtype=torch.float64).to(dev)
        out = {"blocks": ev.integrator_blocks(0)}
        con = torch.empty(ev.n_constraints, dtype=torch.float64, device=dev)
        out["constraint_ms"] = round(timed(lambda: ev.eval_constraint_dev(Z.data_ptr(), con.data_ptr(), st), reps), 4)
        J = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dev)
        jac = lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st)
        out["jacobian_ms"] = round(timed(jac, reps), 4)
        out["jacobian_slab_GB"] = round(8e-9 * ev.n_jacobian_entries, 3)
        out["jacobian_slab_TBps"] = round(8e-9 * ev.n_jacobian_entries / out["jacobian_ms"], 3)
        if flagged:
            ev.profile_enable(True); ev.profile_reset(); jac(); torch.cuda.synchronize()
            ms, _, fl = ev.profile_get("expmv")
            zms, _, zb = ev.profile_get("zero_fill")
            out.update({"jacobian_kernel_ms": round(ms, 4), "jacobian_kernel_TFLOPs": round(fl / ms * 1e-9, 3) if ms > 0 else None,
                        "jacobian_zero_fill_ms": round(zms, 4), "jacobian_zero_fill_TBps": round(zb / zms * 1e-9, 3) if zms > 0 else None})
            ev.profile_enable(False)
        del J
        H = torch.empty(ev.n_hessian_entries, dtype=torch.float64, device=dev)
        hes = lambda: ev.eval_hessian_dev(Z.data_ptr(), sigma, mu.data_ptr(), H.data_ptr(), st)
        out["hessian_ms"] = round(timed(hes, reps), 4)
        out["hessian_slab_GB"] = round(8e-9 * ev.n_hessian_entries, 3)
        if objective_block:  # the objective's share of the call: the same Hessian without it
            hes0 = lambda: ev.eval_hessian_dev(Z.data_ptr(), 0.0, mu.data_ptr(), H.data_ptr(), st)
            out["hessian_sigma0_ms"] = round(timed(hes0, reps), 4)
            out["objective_block_ms"] = round(out["hessian_ms"] - out["hessian_sigma0_ms"], 4)
        if flagged:
            ev.profile_enable(True); ev.profile_reset(); hes(); torch.cuda.synchronize()
            ms, _, fl = ev.profile_get("expmv_adjoint")
            zms, _, zb = ev.profile_get("zero_fill")
            out.update({"hessian_kernel_ms": round(ms, 4), "hessian_kernel_TFLOPs": round(fl / ms * 1e-9, 3) if ms > 0 else None,
                        "hessian_zero_fill_ms": round(zms, 4), "hessian_zero_fill_TBps": round(zb / zms * 1e-9, 3) if zms > 0 else None})
            ev.profile_enable(False)
        return out
    finally:
        ev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="8x1000,16x500", help="comma-separated levels x knots")
    ap.add_argument("--drives", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dense", type=int, default=1, help="0: time the structured handle alone")
    ap.add_argument("--sigma", type=float, default=0.7, help="objective weight of the Hessian (0: the constraint side alone -- the\n"
                    "terminal infidelity's n x n block is assembled by one launch of its own, the same on both handles)")
    ap.add_argument("--objective-block", type=int, default=0, help="1: also time the Hessian at sigma = 0 and report the difference")
    ap.add_argument("--minimum-time", type=int, default=0, help="1: time synthetic.unitary_minimum_time_problem, built-in bound against\n"
                    "host-merged closure")
    ap.add_argument("--products", type=int, default=0, help="1: also time J w and J' w (host pointers and device pointers)")
    ap.add_argument("--small", default="", help="with --products 1: states x knots of one small-path problem timed first")
    a = ap.parse_args()
    if a.products and a.small:
        n, N = (int(x) for x in a.small.lower().split("x"))
        prob = dto_amd.host.synthetic.make_scaled_problem(N, n, 4, seed=42)
        print(json.dumps({"small_states": n, "knots": N, "products": measure_products(prob, False, a.reps)}), flush=True)
    for s in a.shapes.split(","):
        levels, N = (int(x) for x in s.lower().split("x"))
        out = {"levels": levels, "n": 2 * levels * levels, "knots": N, "drives": a.drives, "sigma": a.sigma}
        if a.minimum_time:
            built_in = dto_amd.host.synthetic.unitary_minimum_time_problem(levels, a.drives, N, seed=42)
            closure = dto_amd.host.synthetic.unitary_minimum_time_problem(levels, a.drives, N, seed=42, closure=True)
            out["problem"] = "unitary_minimum_time_problem"
            for name, flagged in (("structured", True), ("dense", False)) if a.dense else (("structured", True),):
                out[name] = {"built_in_dev": measure_handle(built_in, flagged, a.reps, a.sigma),
                             "built_in_host": measure_host(built_in, flagged, a.reps, a.sigma),
                             "closure_host": measure_host(closure, flagged, a.reps, a.sigma)}
            print(json.dumps(out), flush=True)
            continue
        prob = dto_amd.host.synthetic.unitary_problem(levels, a.drives, N, seed=42)
        out["structured"] = measure_handle(prob, True, a.reps, a.sigma, a.objective_block)
        if a.products:
            out["structured"]["products"] = measure_products(prob, True, a.reps)
            if a.dense:
                out["dense_products"] = measure_products(prob, False, a.reps)
        if a.dense:
            out["dense"] = measure_handle(prob, False, a.reps, a.sigma, a.objective_block)
            out["speedup"] = {k: round(out["dense"][k + "_ms"] / out["structured"][k + "_ms"], 2) for k in ("constraint", "jacobian", "hessian")}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
