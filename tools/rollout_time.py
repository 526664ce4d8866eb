#!/usr/bin/env python3
"""Open-loop rollout on the device (Evaluator.rollout_dev) beside the same process's Jacobian and a SciPy host rollout, timed with HIP
events (a tools/ probe; GPU).

Per shape, in ONE process, on ``synthetic.multi_ket_problem(n, 1, drives, N, scale)`` (one ket, skew-symmetric generators: the
propagators are orthogonal, so the rolled states stay of order one over any horizon): device-resident inputs and outputs; every figure
after a warm-up of at least 30 ms of GPU work, the median of ``--reps`` single-call timings:

    rollout_dev, all knots and final knot alone, for n_cols = 1, 16 and x_dim (a full basis: the cumulative propagators),
    eval_jacobian_dev at the same point  -- the yardstick: a rollout evaluates one Jacobian and adds the gather, tree and descent,
    the "rollout" profile split (gather, tree, descent; device ms, launches, flops as executed) with overlap_sweep = 0,

and, once, the rollout a user has without the engine: scipy.sparse.linalg.expm_multiply step by step on the host, one column, with the
largest difference between its states and the device's.  The workspace the rollout adds is reported in GB.  One JSON line per shape.

    python tools/rollout_time.py                       # 256 x 2000 and 64 x 1000
    python tools/rollout_time.py --shapes 128x1000 --reps 9
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


def host_rollout(prob, Z, x0):
    """The rollout without the engine: expm_multiply through every interval, one column."""
    from scipy.sparse.linalg import expm_multiply
    traj, it = prob.trajectory, prob.integrators[0]
    N, z = traj.N, traj.dim
    Zk = Z[:N * z].reshape(N, z)
    G = np.asarray(it.G)
    dt_idx = traj.components[traj.timestep][0]
    X = np.empty((N, it.x_dim))
    X[0] = x0
    t0 = time.perf_counter()
    for k in range(N - 1):
        A = G[0] + np.einsum("j,jrc->rc", Zk[k, it.u_off:it.u_off + it.u_dim], G[1:])
        X[k + 1] = expm_multiply(Zk[k, dt_idx] * A, X[k])
    return X, time.perf_counter() - t0


def workspace_gb(n, N, n_cols, jac_entries):
    """The device memory a rollout adds to the handle, by csrc/dto_rollout_plan.h's formulas: the product tree, the padded trajectory
    and the private Jacobian slab (shared with the slab route of the Jacobian-vector products)."""
    npad, K = -(-n // 64) * 64, N - 1
    L = max(K - 1, 0).bit_length()                       # smallest L with 2^L >= K
    col_pad = -(-n_cols // 16) * 16 if n_cols <= 48 else -(-n_cols // 64) * 64
    return {"tree": round(8e-9 * ((2 << L) - 1) * npad * npad, 3), "trajectory": round(8e-9 * N * col_pad * npad, 3),
            "jacobian_slab": round(8e-9 * jac_entries, 3)}


def measure(n, N, drives, scale, reps):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob, eval_hessian=False)
    out = {"n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps}
    try:
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Z = torch.from_numpy(Zh).to(dev)
        J = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dev)
        jac = lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st)
        out["jacobian_ms"] = round(timed(jac, reps), 4)
        X0 = torch.eye(n, dtype=torch.float64, device=dev)
        for n_cols in sorted({1, min(16, n), n}):
            for all_knots in (True, False):
                X = torch.full((N if all_knots else 1, n_cols, n), float("nan"), dtype=torch.float64, device=dev)
                roll = lambda: ev.rollout_dev(Z.data_ptr(), X0.data_ptr(), n_cols, X.data_ptr(), all_knots=all_knots, stream=st)
                out["rollout_%s_cols%d_ms" % ("all" if all_knots else "final", n_cols)] = round(timed(roll, reps), 4)
                assert bool(torch.isfinite(X).all())
                del X
        out["workspace_GB"] = workspace_gb(n, N, n, ev.n_jacobian_entries)   # what the full-basis rollout above left allocated
        # the split: one kernel at a time
        ev.set_option("overlap_sweep", 0)
        out["jacobian_serial_ms"] = round(timed(jac, reps), 4)
        for n_cols in sorted({1, n}):
            X = torch.full((N, n_cols, n), float("nan"), dtype=torch.float64, device=dev)
            roll = lambda: ev.rollout_dev(Z.data_ptr(), X0.data_ptr(), n_cols, X.data_ptr(), stream=st)
            out["rollout_all_cols%d_serial_ms" % n_cols] = round(timed(roll, reps), 4)
            ev.profile_enable(True); ev.profile_reset(); roll(); torch.cuda.synchronize()
            for part in ("rollout", "rollout_gather", "rollout_tree", "rollout_descent"):
                ms, launches, flops = ev.profile_get(part)
                out["%s_cols%d" % (part, n_cols)] = {"ms": round(ms, 4), "launches": launches, "gflop": round(flops * 1e-9, 3),
                                                     "tflops": round(flops / ms * 1e-9, 2) if ms > 0 and flops > 0 else None}
            ev.profile_enable(False)
            if n_cols == 1:
                first = X[:, 0].cpu().numpy()
            del X
        # what a user has today: the host rollout, once
        Xh, seconds = host_rollout(prob, Zh, np.eye(n)[0])
        out["scipy_host_rollout_s"] = round(seconds, 3)
        out["device_minus_scipy_max"] = float(np.max(np.abs(first - Xh)))
        return out
    finally:
        ev.close()


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


if __name__ == "__main__":
    main()
