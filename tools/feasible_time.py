#!/usr/bin/env python3
"""Feasible-trajectory rollout and reduced merit value on the device (Evaluator.feasible_trajectory_dev, feasible_merit_dev) beside the
same process's yardsticks, timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process, on ``synthetic.multi_ket_problem(n, 1, drives, N, scale)`` -- one ket with skew-symmetric generators, its
DerivativeIntegrator(u, du) and the knot constraint on u -- at a dynamically feasible point (du set to the differences of u, then one
feasible_trajectory_engine call: the Jacobian inside every call below is then evaluated at the same bits), device-resident inputs and
outputs, sigma = 0.7 and a random mu on the constraint rows.  Every pair after a warm-up of at least 30 ms of GPU work per member,
single calls ALTERNATING (yardstick, engine call, yardstick, ...), the median of ``--reps`` each, with the yardstick's spread (min and
max of its samples):

    feasible_trajectory_dev IN PLACE beside rollout_dev of the ket (X0 = the state of knot 1, all knots): the same Jacobian, tree and
        descent, so the difference should be what the "feasible" profile name reports (the derivative recurrence and the scatter) --
        reported with that name's device time, launches and bytes from one profiled call, and the verdict "explained" when the
        difference does not exceed that time plus the yardstick's spread; and the same OUT OF PLACE (one device copy of Z more);
        for what the difference exceeds that time by, the device time of EVERY kernel of one call each with "overlap_sweep" = 0
        (names "all", "rollout_gather", "rollout_tree", "rollout_descent", "feasible"): the sums' difference is time in kernels, the
        rest of the calls' difference is time between them (one launch more on a stream that small shapes keep waiting for the host);
    feasible_trajectory_dev (with its upload and download: feasible_trajectory_engine on host vectors) beside the host composition
        Evaluator.feasible_trajectory, what a user had before -- wall-clock milliseconds, both block;
    feasible_merit_dev beside the hand composition feasible_trajectory_dev + eval_objective_dev + eval_constraint_dev + a torch dot on
        the constraint rows.

One JSON line per shape.

    python tools/feasible_time.py                       # 256 x 2000 and 64 x 1000
    python tools/feasible_time.py --shapes 128x1000 --reps 9
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dto_amd  # noqa: E402

SIGMA = 0.7
SPLIT = ("all", "rollout_gather", "rollout_tree", "rollout_descent", "feasible")   # every kernel of the two calls, each under one name


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternating(yardstick, call, reps, one=event_ms):
    """medians of `reps` single calls each, the two alternating; the yardstick's spread"""
    for fn in (yardstick, call):
        spent = 0.0
        while spent < 30.0:          # warm-up: at least 30 ms of work
            spent += one(fn)
    ys, cs = [], []
    for _ in range(reps):
        ys.append(one(yardstick))
        cs.append(one(call))
    return {"yardstick_ms": round(statistics.median(ys), 4), "call_ms": round(statistics.median(cs), 4),
            "yardstick_min_ms": round(min(ys), 4), "yardstick_max_ms": round(max(ys), 4),
            "call_min_ms": round(min(cs), 4), "call_max_ms": round(max(cs), 4),
            "difference_ms": round(statistics.median(cs) - statistics.median(ys), 4)}


def feasible_point(prob, ev):
    """the problem's point with du = the differences of u, rolled out once"""
    tr = prob.trajectory
    N, z = tr.N, tr.dim
    dt = tr.components[tr.timestep][0]
    Z = np.ascontiguousarray(tr.vec(), dtype=np.float64).copy()
    Zk = Z[:N * z].reshape(N, z)
    for it in prob.integrators:
        if isinstance(it, dto_amd.DerivativeIntegrator):
            x, xd = slice(it.x_off, it.x_off + it.x_dim), slice(it.xdot_off, it.xdot_off + it.x_dim)
            Zk[:-1, xd] = (Zk[1:, x] - Zk[:-1, x]) / Zk[:-1, dt:dt + 1]
    return ev.feasible_trajectory_engine(Z)


def measure(n, N, drives, scale, reps):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob, eval_hessian=False)
    out = {"n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps}
    try:
        Zh = feasible_point(prob, ev)
        n_dyn, n_cons = ev.n_dynamics_constraints, ev.n_constraints
        muh = np.zeros(n_cons)
        muh[n_dyn:] = np.random.default_rng(11).standard_normal(n_cons - n_dyn)
        Z, mu = torch.from_numpy(Zh).to(dev), torch.from_numpy(muh).to(dev)
        f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
        Zf, X, g, f, phi = f64(ev.n_variables), f64(N, 1, n), f64(n_cons), f64(1), f64(1)
        ket = next(i for i, it in enumerate(prob.integrators) if not isinstance(it, dto_amd.DerivativeIntegrator))

        roll = lambda: ev.rollout_dev(Z.data_ptr(), 0, 1, X.data_ptr(), integrator=ket, stream=st)
        Zw = Z.clone()   # in place: at a feasible point every call writes the bits it read
        feas = lambda: ev.feasible_trajectory_dev(Zw.data_ptr(), Zw.data_ptr(), stream=st)
        pair = alternating(roll, feas, reps)
        assert bool(torch.equal(Zw, Z))
        ev.profile_enable(True); ev.profile_reset(); feas(); torch.cuda.synchronize()
        ms, launches, nbytes = ev.profile_get("feasible")
        ev.profile_enable(False)
        pair["feasible_profile"] = {"ms": round(ms, 4), "launches": launches, "bytes": nbytes}
        slack = ms + (pair["yardstick_max_ms"] - pair["yardstick_min_ms"])
        pair["explained"] = bool(pair["difference_ms"] <= slack)
        out["trajectory_in_place_beside_rollout_dev"] = pair
        # where a difference beyond the "feasible" kernels comes from: the device time of every kernel of one call each, one kernel
        # at a time (overlap_sweep = 0) -- what the calls' difference exceeds this by is time between kernels, not in them
        ev.set_option("overlap_sweep", 0)
        split = {}
        for tag, fn in (("rollout_dev", roll), ("feasible_trajectory_dev", feas)):
            fn(); torch.cuda.synchronize()
            ev.profile_enable(True); ev.profile_reset(); fn(); torch.cuda.synchronize()
            split[tag] = {name: {"ms": round(ev.profile_get(name)[0], 4), "launches": ev.profile_get(name)[1]} for name in SPLIT}
            split[tag]["sum_ms"] = round(sum(v["ms"] for v in split[tag].values()), 4)
            ev.profile_enable(False)
        split["kernel_time_difference_ms"] = round(split["feasible_trajectory_dev"]["sum_ms"] - split["rollout_dev"]["sum_ms"], 4)
        ev.set_option("overlap_sweep", 1)
        out["kernel_time_split_serial"] = split
        copy = lambda: ev.feasible_trajectory_dev(Z.data_ptr(), Zf.data_ptr(), stream=st)   # out of place: one device copy of Z more
        out["trajectory_out_of_place_beside_rollout_dev"] = alternating(roll, copy, reps)
        assert bool(torch.equal(Zf, Z))

        host = lambda: ev.feasible_trajectory(Zh)
        engine = lambda: ev.feasible_trajectory_engine(Zh)
        out["host_vectors_beside_host_composition_wall"] = alternating(host, engine, reps, one=wall_ms)
        assert np.array_equal(ev.feasible_trajectory(Zh), ev.feasible_trajectory_engine(Zh))

        def hand():
            ev.feasible_trajectory_dev(Z.data_ptr(), Zf.data_ptr(), stream=st)
            ev.eval_objective_dev(Zf.data_ptr(), f.data_ptr(), st)
            ev.eval_constraint_dev(Zf.data_ptr(), g.data_ptr(), st)
            return SIGMA * f + torch.dot(mu[n_dyn:], g[n_dyn:])

        merit = lambda: ev.feasible_merit_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), phi.data_ptr(), Zf.data_ptr(), g.data_ptr(), stream=st)
        out["merit_beside_hand_composition"] = alternating(hand, merit, reps)
        want = float(hand().cpu()[0]); merit(); torch.cuda.synchronize()
        out["merit_minus_hand"] = float(phi.cpu()[0]) - want
        return out
    finally:
        ev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="256x2000,64x1000", help="comma-separated states x knots")
    ap.add_argument("--drives", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="standard deviation of the generators' entries (1.0: the norms of the\n"
                    "headline benchmark; 0: 1 / sqrt(n), norms of order one)")
    a = ap.parse_args()
    for s in a.shapes.split(","):
        n, N = (int(x) for x in s.lower().split("x"))
        print(json.dumps(measure(n, N, a.drives, a.scale, a.reps)), flush=True)


if __name__ == "__main__":
    main()
