#!/usr/bin/env python3
"""Solves with the dynamics block on the device (Evaluator.dynamics_solve_dev) beside the same process's rollout and Jacobian and the
SciPy host recurrences, timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process, on ``synthetic.multi_ket_problem(n, 1, drives, N, scale)`` (one ket, skew-symmetric generators: the
propagators are orthogonal): device-resident inputs and outputs; every figure after a warm-up of at least 30 ms of GPU work, the
median of ``--reps`` single-call timings:

    dynamics_solve_dev, forward and adjoint, all knots, for n_cols = 1, 16 and x_dim, at a NEW point (two points that differ in one
        bit of a control alternate, so every call rebuilds the tree) and at the CACHED point (the scan alone),
    rollout_dev for the same column counts and eval_jacobian_dev at the same point  -- the yardsticks,
    the "dynsolve" profile split ("dynsolve_tree", "dynsolve_scan"; device ms, launches, flops as executed) of one new-point and one
        cached solve per direction with overlap_sweep = 0,

and, once, the solves a user has without the engine: the two recurrences with scipy.sparse.linalg.expm_multiply step by step on the
host, one column, with the largest difference between their result and the device's.  The workspace the solves add is reported in GB.
One JSON line per shape.

    python tools/dynsolve_time.py                       # 256 x 2000 and 64 x 1000
    python tools/dynsolve_time.py --shapes 128x1000 --reps 9
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


def host_solves(prob, Z, b):
    """The two recurrences without the engine: expm_multiply through every interval, one column.  b: (N, x_dim)."""
    from scipy.sparse.linalg import expm_multiply
    traj, it = prob.trajectory, prob.integrators[0]
    N, z = traj.N, traj.dim
    Zk = Z[:N * z].reshape(N, z)
    G = np.asarray(it.G)
    dt_idx = traj.components[traj.timestep][0]
    A = [Zk[k, dt_idx] * (G[0] + np.einsum("j,jrc->rc", Zk[k, it.u_off:it.u_off + it.u_dim], G[1:])) for k in range(N - 1)]
    Y, Lam = np.empty_like(b), np.empty_like(b)
    t0 = time.perf_counter()
    Y[0] = b[0]
    for k in range(N - 1):
        Y[k + 1] = expm_multiply(A[k], Y[k]) + b[k + 1]
    t1 = time.perf_counter()
    Lam[N - 1] = b[N - 1]
    for k in range(N - 2, -1, -1):
        Lam[k] = expm_multiply(A[k].T, Lam[k + 1]) + b[k]
    return Y, Lam, t1 - t0, time.perf_counter() - t1


def workspace_gb(n, N, n_cols):
    """What the solves add to a handle that has rolled out (csrc/dto_rollout_plan.h): the offset tree and the copy of Z are theirs; the
    product tree and the padded trajectory are the rollout's."""
    npad, K = -(-n // 64) * 64, N - 1
    L = max(K - 1, 0).bit_length()                       # smallest L with 2^L >= K
    col_pad = -(-n_cols // 16) * 16 if n_cols <= 48 else -(-n_cols // 64) * 64
    return {"offset_tree": round(8e-9 * ((2 << L) - 1) * col_pad * npad, 3), "tree": round(8e-9 * ((2 << L) - 1) * npad * npad, 3),
            "trajectory": round(8e-9 * N * col_pad * npad, 3)}


def profile_split(ev, call):
    ev.profile_enable(True); ev.profile_reset(); call(); torch.cuda.synchronize()
    out = {}
    for part in ("dynsolve", "dynsolve_tree", "dynsolve_scan"):
        ms, launches, flops = ev.profile_get(part)
        out[part] = {"ms": round(ms, 4), "launches": launches, "gflop": round(flops * 1e-9, 3),
                     "tflops": round(flops / ms * 1e-9, 2) if ms > 0 and flops > 0 else None}
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
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Zh2 = Zh.copy()
        Zh2[it.u_off] = np.nextafter(Zh2[it.u_off], np.inf)           # the other point: one bit of one control
        Z, Z2 = torch.from_numpy(Zh).to(dev), torch.from_numpy(Zh2).to(dev)
        J = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dev)
        jac = lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st)
        out["jacobian_ms"] = round(timed(jac, reps), 4)
        X0 = torch.eye(n, dtype=torch.float64, device=dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        first = {}
        for n_cols in sorted({1, min(16, n), n}):
            B = torch.randn((N, n_cols, n), dtype=torch.float64, device=dev, generator=gen)
            Y = torch.full((N, n_cols, n), float("nan"), dtype=torch.float64, device=dev)
            roll = lambda: ev.rollout_dev(Z.data_ptr(), X0.data_ptr(), n_cols, Y.data_ptr(), stream=st)
            out["rollout_all_cols%d_ms" % n_cols] = round(timed(roll, reps), 4)
            for adjoint in (False, True):
                tag = "%s_cols%d" % ("adjoint" if adjoint else "forward", n_cols)
                flip = [0]

                def new_point():
                    flip[0] ^= 1
                    ev.dynamics_solve_dev((Z2 if flip[0] else Z).data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(), adjoint=adjoint, stream=st)

                cached = lambda: ev.dynamics_solve_dev(Z.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(), adjoint=adjoint, stream=st)
                out["solve_new_%s_ms" % tag] = round(timed(new_point, reps), 4)
                cached(); torch.cuda.synchronize()
                out["solve_cached_%s_ms" % tag] = round(timed(cached, reps), 4)
                assert bool(torch.isfinite(Y).all())
                if n_cols == 1:
                    first[adjoint] = (B[:, 0].cpu().numpy(), Y[:, 0].cpu().numpy())
            del B, Y
        out["workspace_GB"] = workspace_gb(n, N, n)   # what the full-basis solves above left allocated
        # the split: one kernel at a time
        ev.set_option("overlap_sweep", 0)
        for n_cols in sorted({1, n}):
            B = torch.randn((N, n_cols, n), dtype=torch.float64, device=dev, generator=gen)
            Y = torch.full((N, n_cols, n), float("nan"), dtype=torch.float64, device=dev)
            for adjoint in (False, True):
                tag = "%s_cols%d" % ("adjoint" if adjoint else "forward", n_cols)
                out["split_new_" + tag] = profile_split(ev, lambda: ev.dynamics_solve_dev(Z2.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(),
                                                                                          adjoint=adjoint, stream=st))
                out["split_cached_" + tag] = profile_split(ev, lambda: ev.dynamics_solve_dev(Z2.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(),
                                                                                             adjoint=adjoint, stream=st))
                ev.dynamics_solve_dev(Z.data_ptr(), B.data_ptr(), n_cols, Y.data_ptr(), adjoint=adjoint, stream=st)   # (the next new point)
            del B, Y
        # what a user has today: the host recurrences, once (both directions were given the same right-hand side)
        Yh, Lh, s_fw, s_ad = host_solves(prob, Zh, first[False][0])
        out["scipy_host_forward_s"], out["scipy_host_adjoint_s"] = round(s_fw, 3), round(s_ad, 3)
        out["device_minus_scipy_forward_max"] = float(np.max(np.abs(first[False][1] - Yh)))
        out["device_minus_scipy_adjoint_max"] = float(np.max(np.abs(first[True][1] - Lh)))
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
