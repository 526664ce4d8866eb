#!/usr/bin/env python3
"""Whole-dynamics solves on the device (Evaluator.dynamics_solve_all_dev) beside the same process's single-integrator solve and
Jacobian, timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process, on ``synthetic.multi_ket_problem(n, 1, drives, N, scale)`` -- one ket with skew-symmetric generators and
DerivativeIntegrator(u, du): two integrators, two levels -- with device-resident inputs and outputs; every figure after a warm-up of
at least 30 ms of GPU work, the median of ``--reps`` single-call timings:

    dynamics_solve_all_dev, forward and adjoint, for n_cols = 1 and 16, at a NEW point (two points that differ in one bit of a
        control alternate, so every call evaluates the Jacobian, rebuilds the tree and gathers the couplings) and at the CACHED point,
    dynamics_solve_dev of the ket's own block for the same column counts, new and cached, and eval_jacobian_dev  -- the yardsticks:
        a new-point whole-dynamics solve runs the same Jacobian and tree plus the couplings and the derivative scan,
    the profile split ("dynsolve_tree", "dynsolve_scan", "dynsolve_couple", "dynsolve_deriv"; device ms, launches, and flops or bytes
        as executed) of one new-point and one cached solve per direction with overlap_sweep = 0,

and, once, k_deriv_scan alone: a handle with one DerivativeIntegrator of ``drives`` components at N = 2000 and 16000, cached-point
solves of 1, 16 and 64 columns and their "dynsolve_deriv" device time.  One JSON line per shape, one for the scans.

    python tools/elim_time.py                       # 256 x 2000 and 64 x 1000
    python tools/elim_time.py --shapes 128x1000 --reps 9
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

PARTS = ("dynsolve_tree", "dynsolve_scan", "dynsolve_couple", "dynsolve_deriv")


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


def profile_split(ev, call):
    ev.profile_enable(True); ev.profile_reset(); call(); torch.cuda.synchronize()
    out = {}
    for part in PARTS:
        ms, launches, work = ev.profile_get(part)
        out[part] = {"ms": round(ms, 4), "launches": launches, "gflop_or_GB": round(work * 1e-9, 4)}
    ev.profile_enable(False)
    return out


def measure(n, N, drives, scale, reps):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob, eval_hessian=False)
    out = {"n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps}
    try:
        it = prob.integrators[0]
        D, levels, offset, level = ev.dynamics_layout()
        out["n_states"], out["levels"] = D, levels
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Zh2 = Zh.copy()
        Zh2[it.u_off] = np.nextafter(Zh2[it.u_off], np.inf)           # the other point: one bit of one control
        Z, Z2 = torch.from_numpy(Zh).to(dev), torch.from_numpy(Zh2).to(dev)
        J = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dev)
        out["jacobian_ms"] = round(timed(lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st), reps), 4)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        # the coupling store: the ket's rows in the u columns of both knots (dto_elim_plan.h)
        out["coupling_store_MB"] = round(8e-6 * (N - 1) * 2 * drives * n, 3)
        for n_cols in (1, min(16, n)):
            B = torch.randn((N, n_cols, D), dtype=torch.float64, device=dev, generator=gen)
            Y = torch.full((N, n_cols, D), float("nan"), dtype=torch.float64, device=dev)
            Bk = torch.randn((N, n_cols, n), dtype=torch.float64, device=dev, generator=gen)
            Yk = torch.full((N, n_cols, n), float("nan"), dtype=torch.float64, device=dev)
            for adjoint in (False, True):
                tag = "%s_cols%d" % ("adjoint" if adjoint else "forward", n_cols)
                flip = [0]

                def point():
                    flip[0] ^= 1
                    return (Z2 if flip[0] else Z).data_ptr()

                new_all = lambda: ev.dynamics_solve_all_dev(point(), B.data_ptr(), n_cols, Y.data_ptr(), adjoint=adjoint, stream=st)
                cached_all = lambda: ev.dynamics_solve_all_dev(Z.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(), adjoint=adjoint, stream=st)
                new_one = lambda: ev.dynamics_solve_dev(point(), Bk.data_ptr(), n_cols, Yk.data_ptr(), adjoint=adjoint, stream=st)
                cached_one = lambda: ev.dynamics_solve_dev(Z.data_ptr(), Bk.data_ptr(), n_cols, Yk.data_ptr(), adjoint=adjoint, stream=st)
                out["all_new_%s_ms" % tag] = round(timed(new_all, reps), 4)
                cached_all(); torch.cuda.synchronize()
                out["all_cached_%s_ms" % tag] = round(timed(cached_all, reps), 4)
                out["one_new_%s_ms" % tag] = round(timed(new_one, reps), 4)
                cached_one(); torch.cuda.synchronize()
                out["one_cached_%s_ms" % tag] = round(timed(cached_one, reps), 4)
                out["all_minus_one_new_%s_ms" % tag] = round(out["all_new_%s_ms" % tag] - out["one_new_%s_ms" % tag], 4)
                assert bool(torch.isfinite(Y).all())
        # the split: one kernel at a time
        ev.set_option("overlap_sweep", 0)
        for adjoint in (False, True):
            tag = "%s_cols%d" % ("adjoint" if adjoint else "forward", n_cols)
            out["split_new_" + tag] = profile_split(ev, lambda: ev.dynamics_solve_all_dev(Z2.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(),
                                                                                          adjoint=adjoint, stream=st))
            out["split_cached_" + tag] = profile_split(ev, lambda: ev.dynamics_solve_all_dev(Z2.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(),
                                                                                             adjoint=adjoint, stream=st))
            ev.dynamics_solve_all_dev(Z.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(), adjoint=adjoint, stream=st)   # (the next new point)
        return out
    finally:
        ev.close()


def derivative_scan(d, reps):
    """k_deriv_scan alone: one DerivativeIntegrator(u, du) of d components"""
    DerivativeIntegrator, DirectTrajOptProblem = dto_amd.DerivativeIntegrator, dto_amd.DirectTrajOptProblem
    QuadraticRegularizer, NamedTrajectory = dto_amd.QuadraticRegularizer, dto_amd.NamedTrajectory
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {"derivative_scan_components": d, "reps": reps}
    rng = np.random.default_rng(1)
    for N in (2000, 16000):
        traj = NamedTrajectory({"u": rng.standard_normal((d, N)), "du": rng.standard_normal((d, N)), "dt": np.full((1, N), 0.1)}, timestep="dt")
        ev = dto_amd.Evaluator(DirectTrajOptProblem(traj, QuadraticRegularizer("u", traj, 1.0), [DerivativeIntegrator("u", "du", traj)]),
                               eval_hessian=False)
        try:
            Z = torch.from_numpy(np.ascontiguousarray(traj.vec(), dtype=np.float64)).to(dev)
            for n_cols in (1, 16, 64):
                B = torch.randn((N, n_cols, d), dtype=torch.float64, device=dev)
                Y = torch.full((N, n_cols, d), float("nan"), dtype=torch.float64, device=dev)
                for adjoint in (False, True):
                    call = lambda: ev.dynamics_solve_all_dev(Z.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(), adjoint=adjoint, stream=st)
                    tag = "N%d_%s_cols%d" % (N, "adjoint" if adjoint else "forward", n_cols)
                    out["call_" + tag + "_ms"] = round(timed(call, reps), 4)
                    out["kernel_" + tag + "_ms"] = profile_split(ev, call)["dynsolve_deriv"]["ms"]
                    assert bool(torch.isfinite(Y).all())
        finally:
            ev.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="256x2000,64x1000", help="comma-separated states x knots")
    ap.add_argument("--drives", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="standard deviation of the generators' entries (1.0: the norms of the\n"
                    "headline benchmark, several squarings per propagator; 0: 1 / sqrt(n), norms of order one)")
    a = ap.parse_args()
    for s in a.shapes.split(","):
        n, N = (int(x) for x in s.lower().split("x"))
        print(json.dumps(measure(n, N, a.drives, a.scale, a.reps)), flush=True)
    print(json.dumps(derivative_scan(a.drives, a.reps)), flush=True)


if __name__ == "__main__":
    main()
