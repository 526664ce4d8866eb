#!/usr/bin/env python3
"""The device TimeDependentBilinearIntegrator at 65..256 states (csrc/dto_tdb_mfma.hip), timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process: a problem with random generators of unit-order norm (`drives` drives, two carrier terms, 16 sub-steps),
both spline orders; device-resident inputs and outputs; eval_constraint, eval_constraint_jacobian and eval_hessian_lagrangian, each
after a warm-up of at least 30 ms of GPU work; the median of ``--reps`` single-call timings.  Beside the call time the line gives
the new kernel's time alone and its FP64 rate from the flop count as executed (dto_profile_get "tdb_mfma").  ``--host 72x20``
adds the host-evaluated path (on_device=False: Python RK4, numeric derivatives, merged by the engine) against the device path on
the same problem, through host pointers, one call each.  One JSON line per shape and order.

    python tools/tdb_time.py                                  # 72 x 500, 128 x 500, 256 x 250 and the host path at 72 x 20
    python tools/tdb_time.py --shapes 128x500 --orders 1 --host ""
    python tools/tdb_time.py --small 1                        # the scalar kernel's sizes (4 .. 64 states, csrc/dto_tdb.hip) through
                                                              # host pointers, as this probe reported them before
    python tools/tdb_time.py --block 1                        # replicated-block generators (csrc/dto_tdb_kron.hip): a unitary's
                                                              # I_r (x) B family, flagged (block_generators=True) against unflagged
                                                              # handles alternated in one process; order 1; 72 x 500, 128 x 500,
                                                              # 162 x 250 both ways, 512 x 100 flagged only (the dense kernels stop
                                                              # at 256 states)
    python tools/tdb_time.py --block 1 --products 1           # the structured path's device-pointer J w / J' w (k_tdb_kron_product):
                                                              # two flagged handles of one problem, option "tdb_matrix_free_products"
                                                              # 1 and 0 (the slab route), their calls alternated in one process,
                                                              # beside each handle's eval_constraint and Jacobian; --products-route
                                                              # slab times the slab handle alone
    python tools/tdb_time.py --products 1 --shapes 4x1000,64x1000,128x500,256x250 --orders 1 --host ""
                                                              # adds the device-pointer J w / J' w with the handle option
                                                              # "tdb_matrix_free_products" on (csrc/dto_tdb.hip and dto_tdb_mfma.hip,
                                                              # product modes) next to eval_constraint and the Jacobian;
                                                              # --products-route slab leaves the option alone (the slab route: what
                                                              # a build without the option does, e.g. one named by DTO_ENGINE_LIB)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dto_amd  # noqa: E402


def problem(n, N, drives, order, substeps, on_device=True, seed=42):
    rng = np.random.default_rng(seed)
    traj = dto_amd.NamedTrajectory({"x": rng.standard_normal((n, N)), "u": 0.4 * rng.standard_normal((drives, N)),
                                    "t": np.cumsum(np.full(N, 0.3))[None, :], "dt": 0.25 + 0.1 * rng.random((1, N))}, timestep="dt")
    s = 1.0 / np.sqrt(n / 4.0)
    G = s * rng.standard_normal((drives + 1, n, n))
    mods = [("cos", 1.7, 0.5 * s * rng.standard_normal((drives + 1, n, n))), ("sin", 0.6, 0.5 * s * rng.standard_normal((drives + 1, n, n)))]
    tdb = dto_amd.TimeDependentBilinearIntegrator(dto_amd.ModulatedGenerators(G, mods), "x", "u", "t", traj, spline_order=order,
                                                  substeps=substeps, on_device=on_device)
    return dto_amd.DirectTrajOptProblem(traj, dto_amd.QuadraticRegularizer("u", traj, 1.0), [tdb])


def block_problem(levels, N, drives, order, substeps, seed=42):
    """States 2 levels^2: generators kron(I_levels, B) with random 2 levels x 2 levels blocks of `problem`'s scale, two carriers."""
    rng = np.random.default_rng(seed)
    b, n = 2 * levels, 2 * levels * levels
    traj = dto_amd.NamedTrajectory({"x": rng.standard_normal((n, N)), "u": 0.4 * rng.standard_normal((drives, N)),
                                    "t": np.cumsum(np.full(N, 0.3))[None, :], "dt": 0.25 + 0.1 * rng.random((1, N))}, timestep="dt")
    s = 1.0 / np.sqrt(b / 4.0)
    rep = lambda B: np.stack([np.kron(np.eye(levels), Bj) for Bj in B])
    G = rep(s * rng.standard_normal((drives + 1, b, b)))
    mods = [("cos", 1.7, rep(0.5 * s * rng.standard_normal((drives + 1, b, b)))), ("sin", 0.6, rep(0.5 * s * rng.standard_normal((drives + 1, b, b))))]
    tdb = dto_amd.TimeDependentBilinearIntegrator(dto_amd.ModulatedGenerators(G, mods), "x", "u", "t", traj, spline_order=order, substeps=substeps)
    return dto_amd.DirectTrajOptProblem(traj, dto_amd.QuadraticRegularizer("u", traj, 1.0), [tdb])


def measure_block(prob, reps, with_dense, sigma=0.7):
    """Flagged and unflagged handles of one problem in one process, their timed calls alternated: per call a warm-up of at least
    30 ms on each handle, then `reps` rounds of one call on each; medians.  Kernel time and rate from the profile names."""
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    evs = {"flagged": dto_amd.Evaluator(prob, eval_hessian=True, block_generators=True)}
    if with_dense:
        evs["unflagged"] = dto_amd.Evaluator(prob, eval_hessian=True)
    try:
        e0 = evs["flagged"]
        Z = torch.from_numpy(prob.trajectory.vec()).to(dev)
        mu = torch.randn(e0.n_constraints, generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float64).to(dev)
        con = torch.empty(e0.n_constraints, dtype=torch.float64, device=dev)
        J = torch.empty(e0.n_jacobian_entries, dtype=torch.float64, device=dev)
        H = torch.empty(e0.n_hessian_entries, dtype=torch.float64, device=dev)
        out = {"blocks": e0.integrator_blocks(0)}

        def calls(ev):
            return {"constraint": lambda: ev.eval_constraint_dev(Z.data_ptr(), con.data_ptr(), st),
                    "jacobian": lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st),
                    "hessian": lambda: ev.eval_hessian_dev(Z.data_ptr(), sigma, mu.data_ptr(), H.data_ptr(), st)}

        fns = {k: calls(ev) for k, ev in evs.items()}
        for name in ("constraint", "jacobian", "hessian"):
            for k in evs:
                spent = 0.0
                while spent < 30.0:
                    spent += one_call_ms(fns[k][name])
            ts = {k: [] for k in evs}
            for _ in range(reps):
                for k in evs:
                    ts[k].append(one_call_ms(fns[k][name]))
            for k, ev in evs.items():
                out[f"{k}_{name}_ms"] = round(statistics.median(ts[k]), 4)
                prof = "tdb_kron" if k == "flagged" else "tdb_mfma"
                ev.profile_enable(True); ev.profile_reset(); fns[k][name](); torch.cuda.synchronize()
                ms, launches, fl = ev.profile_get(prof)
                ev.profile_enable(False)
                out[f"{k}_{name}_{prof}_ms"] = round(ms, 4)
                out[f"{k}_{name}_{prof}_TFLOPs"] = round(fl / ms * 1e-9, 3) if ms > 0 else None
        return out
    finally:
        for ev in evs.values():
            ev.close()


def measure_block_products(prob, reps, route):
    """Flagged handles of one problem with option "tdb_matrix_free_products" at 1 and at 0 (route "slab": the latter alone), their
    timed calls alternated as in measure_block; eval_constraint, the Jacobian, J w and J' w through device pointers.  Kernel time
    and rate of the products from "tdb_product" (matrix-free) or "tdb_kron" (slab: the Jacobian call inside the product)."""
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    evs = {}
    if route == "matrix_free":
        evs["matrix_free"] = dto_amd.Evaluator(prob, eval_hessian=True, block_generators=True)
        evs["matrix_free"].set_option("tdb_matrix_free_products", 1)
    evs["slab"] = dto_amd.Evaluator(prob, eval_hessian=True, block_generators=True)
    try:
        e0 = evs["slab"]
        Z = torch.from_numpy(prob.trajectory.vec()).to(dev)
        gen = torch.Generator(device="cpu").manual_seed(2)
        w = torch.randn(e0.n_variables, generator=gen, dtype=torch.float64).to(dev)
        wt = torch.randn(e0.n_constraints, generator=gen, dtype=torch.float64).to(dev)
        con = torch.empty(e0.n_constraints, dtype=torch.float64, device=dev)
        J = torch.empty(e0.n_jacobian_entries, dtype=torch.float64, device=dev)
        y = torch.empty(e0.n_constraints, dtype=torch.float64, device=dev)
        yt = torch.empty(e0.n_variables, dtype=torch.float64, device=dev)
        out = {"blocks": e0.integrator_blocks(0), "jac_slab_MiB": round(8.0 * e0.n_jacobian_entries / 2**20, 1)}

        def calls(ev):
            return {"constraint": lambda: ev.eval_constraint_dev(Z.data_ptr(), con.data_ptr(), st),
                    "jacobian": lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st),
                    "jw": lambda: ev.eval_jacobian_product_dev(Z.data_ptr(), w.data_ptr(), y.data_ptr(), st),
                    "jtw": lambda: ev.eval_jacobian_transpose_product_dev(Z.data_ptr(), wt.data_ptr(), yt.data_ptr(), st)}

        fns = {k: calls(ev) for k, ev in evs.items()}
        for name in ("constraint", "jacobian", "jw", "jtw"):
            for k in evs:
                spent = 0.0
                while spent < 30.0:
                    spent += one_call_ms(fns[k][name])
            ts = {k: [] for k in evs}
            for _ in range(reps):
                for k in evs:
                    ts[k].append(one_call_ms(fns[k][name]))
            for k, ev in evs.items():
                out[f"{k}_{name}_ms"] = round(statistics.median(ts[k]), 4)
                prof = "tdb_product" if k == "matrix_free" and name in ("jw", "jtw") else "tdb_kron"
                ev.profile_enable(True); ev.profile_reset(); fns[k][name](); torch.cuda.synchronize()
                ms, launches, fl = ev.profile_get(prof)
                ev.profile_enable(False)
                out[f"{k}_{name}_{prof}_ms"] = round(ms, 4)
                out[f"{k}_{name}_{prof}_TFLOPs"] = round(fl / ms * 1e-9, 3) if ms > 0 else None
        return out
    finally:
        for ev in evs.values():
            ev.close()


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


def measure_device(prob, reps, sigma=0.7, products=False, route="matrix_free"):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ev = dto_amd.Evaluator(prob, eval_hessian=True)
    try:
        if products and route == "matrix_free":
            ev.set_option("tdb_matrix_free_products", 1)
        Z = torch.from_numpy(prob.trajectory.vec()).to(dev)
        mu = torch.randn(ev.n_constraints, generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float64).to(dev)
        con = torch.empty(ev.n_constraints, dtype=torch.float64, device=dev)
        J = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dev)
        H = torch.empty(ev.n_hessian_entries, dtype=torch.float64, device=dev)
        calls = {"constraint": lambda: ev.eval_constraint_dev(Z.data_ptr(), con.data_ptr(), st),
                 "jacobian": lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st),
                 "hessian": lambda: ev.eval_hessian_dev(Z.data_ptr(), sigma, mu.data_ptr(), H.data_ptr(), st)}
        out = {}
        if products:
            gen = torch.Generator(device="cpu").manual_seed(2)
            w = torch.randn(ev.n_variables, generator=gen, dtype=torch.float64).to(dev)
            y = torch.empty(ev.n_constraints, dtype=torch.float64, device=dev)
            yt = torch.empty(ev.n_variables, dtype=torch.float64, device=dev)
            del calls["hessian"]
            calls["jw"] = lambda: ev.eval_jacobian_product_dev(Z.data_ptr(), w.data_ptr(), y.data_ptr(), st)
            calls["jtw"] = lambda: ev.eval_jacobian_transpose_product_dev(Z.data_ptr(), mu.data_ptr(), yt.data_ptr(), st)
            out["products_route"] = route
        for name, fn in calls.items():
            out[name + "_ms"] = round(timed(fn, reps), 4)
            ev.profile_enable(True); ev.profile_reset(); fn(); torch.cuda.synchronize()
            ms, launches, fl = ev.profile_get("tdb_product" if products and route == "matrix_free" and name in ("jw", "jtw") else "tdb_mfma")
            ev.profile_enable(False)
            out[name + "_kernel_ms"] = round(ms, 4)
            out[name + "_kernel_launches"] = launches
            out[name + "_kernel_TFLOPs"] = round(fl / ms * 1e-9, 3) if ms > 0 else None
        return out
    finally:
        ev.close()


def measure_host_pointers(prob, reps):
    """One blocking call each through host pointers (wall clock): what the host-evaluated path can be compared on."""
    ev = dto_amd.Evaluator(prob, eval_hessian=True)
    try:
        Z = prob.trajectory.vec()
        mu = np.random.default_rng(1).standard_normal(ev.n_constraints)
        g, J, H = np.empty(ev.n_constraints), np.empty(ev.n_jacobian_entries), np.empty(ev.n_hessian_entries)
        out = {}
        for name, fn in (("constraint", lambda: ev.eval_constraint(g, Z)), ("jacobian", lambda: ev.eval_constraint_jacobian(J, Z)),
                         ("hessian", lambda: ev.eval_hessian_lagrangian(H, Z, 0.7, mu))):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append(1e3 * (time.perf_counter() - t0))
            out[name + "_ms"] = round(statistics.median(ts), 3)
        return out
    finally:
        ev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="72x500,128x500,256x250", help="comma-separated states x knots")
    ap.add_argument("--orders", default="0,1")
    ap.add_argument("--drives", type=int, default=4)
    ap.add_argument("--substeps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", default="72x20", help="states x knots of the host-evaluated comparison (empty: none)")
    ap.add_argument("--small", type=int, default=0, help="1: 4 .. 64 states (k_tdb), 2 drives, order 1, host pointers; nothing else")
    ap.add_argument("--block", type=int, default=0, help="1: replicated-block generators, flagged against unflagged handles; nothing else")
    ap.add_argument("--block-shapes", default="6x500,8x500,9x250,16x100", help="with --block: comma-separated levels x knots (states = 2 levels^2)")
    ap.add_argument("--products", type=int, default=0, help="1: time the device-pointer J w / J' w (option tdb_matrix_free_products on) instead of the Hessian; with --block 1 on flagged handles")
    ap.add_argument("--products-route", default="matrix_free", choices=["matrix_free", "slab"], help="with --products: slab leaves the option alone")
    a = ap.parse_args()
    if a.block:
        for s in [x for x in a.block_shapes.split(",") if x]:
            levels, N = (int(x) for x in s.lower().split("x"))
            n = 2 * levels * levels
            out = {"n": n, "levels": levels, "knots": N, "drives": a.drives, "substeps": a.substeps, "order": 1}
            prob = block_problem(levels, N, a.drives, 1, a.substeps)
            if a.products:
                out.update(measure_block_products(prob, a.reps, a.products_route))
            else:
                out.update(measure_block(prob, a.reps, with_dense=n <= 256))
            print(json.dumps(out), flush=True)
        return
    if a.small:
        for n, N in ((4, 1000), (16, 500), (32, 500), (64, 200)):
            out = {"n": n, "knots": N, "drives": 2, "substeps": a.substeps, "order": 1, "through": "host pointers, wall clock"}
            out.update(measure_host_pointers(problem(n, N, 2, 1, a.substeps), 5))
            print(json.dumps(out), flush=True)
        return
    for s in [x for x in a.shapes.split(",") if x]:
        n, N = (int(x) for x in s.lower().split("x"))
        for order in (int(x) for x in a.orders.split(",")):
            out = {"n": n, "knots": N, "drives": a.drives, "substeps": a.substeps, "order": order}
            out.update(measure_device(problem(n, N, a.drives, order, a.substeps), a.reps, products=bool(a.products), route=a.products_route))
            print(json.dumps(out), flush=True)
    if a.host:
        n, N = (int(x) for x in a.host.lower().split("x"))
        out = {"n": n, "knots": N, "drives": a.drives, "substeps": a.substeps, "order": 1, "through": "host pointers, wall clock"}
        out["device"] = measure_host_pointers(problem(n, N, a.drives, 1, a.substeps), 3)
        out["host_evaluated"] = measure_host_pointers(problem(n, N, a.drives, 1, a.substeps, on_device=False), 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
