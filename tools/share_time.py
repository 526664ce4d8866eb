#!/usr/bin/env python3
"""Shared propagator chain (Evaluator(..., shared_generators=True)) against one chain per integrator on the same multi-ket problem,
timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process: a flagged and an unflagged handle on ``synthetic.multi_ket_problem(n, kets, drives, N, scale)``;
device-resident inputs and outputs; eval_constraint, eval_constraint_jacobian, eval_hessian_lagrangian and one solver iteration
(objective, gradient, constraint, Jacobian, Hessian at one point), each after a warm-up of at least 30 ms of GPU work (the chip
ramps for about that long); the median of ``--reps`` single-call timings.  The unflagged handle runs every integrator's chain: it
is the yardstick.  Its chain time per member comes from its own profile with overlap_sweep = 0 (dto_profile_get "bgemm" + "basis";
"bgemm" counts the one-launch chain of 33..64 states too); the line reports the time saved per Jacobian against
(kets - 1) x that, and the rate of the copy kernel (dto_profile_get "share": bytes written, plus one block read per interval).
One JSON line per shape.  ``saved_over_followers_chains`` of such a line compares the two handles of ONE build in one process; the
yardstick for a change of the engine is the PARENT commit in alternated processes: run the parent's build with ``--flagged 0``
(or its library under this tool), this build as it is, several times each, every process appending its lines to a file, and
``--combine parent.jsonl new.jsonl`` prints per shape the min - max of every callback over the runs and the condition
(parent's median Jacobian - this build's flagged median) / ((kets - 1) x the parent's own chain time per member) >= 0.7.

    python tools/share_time.py                               # 256 x 2000 x 4, 128 x 1000 x 4, 64 x 1000 x 4
    python tools/share_time.py --shapes 512x500x2
    python tools/share_time.py --flagged 0                   # the unflagged handle alone (a build without the flag's code paths)
    python tools/share_time.py --combine parent.jsonl new.jsonl
"""
import argparse
import json
import os
import statistics
import sys

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


def measure_handle(prob, flagged, reps, sigma=0.7):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    kw = {"shared_generators": True} if flagged else {}
    ev = dto_amd.Evaluator(prob, eval_hessian=True, **kw)
    try:
        g = torch.Generator(device="cpu").manual_seed(1)
        Z = torch.from_numpy(prob.trajectory.vec()).to(dev)
        mu = torch.randn(ev.n_constraints, generator=g, dtype=torch.float64).to(dev)
        out = {"share": ev.integrator_share(1)} if flagged else {}
        f = torch.empty(1, dtype=torch.float64, device=dev)
        grad = torch.empty(ev.n_variables, dtype=torch.float64, device=dev)
        con = torch.empty(ev.n_constraints, dtype=torch.float64, device=dev)
        J = torch.empty(ev.n_jacobian_entries, dtype=torch.float64, device=dev)
        H = torch.empty(ev.n_hessian_entries, dtype=torch.float64, device=dev)
        cons = lambda: ev.eval_constraint_dev(Z.data_ptr(), con.data_ptr(), st)
        jac = lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st)
        hes = lambda: ev.eval_hessian_dev(Z.data_ptr(), sigma, mu.data_ptr(), H.data_ptr(), st)

        def iteration():
            ev.eval_objective_dev(Z.data_ptr(), f.data_ptr(), st)
            ev.eval_gradient_dev(Z.data_ptr(), grad.data_ptr(), st)
            cons(); jac(); hes()

        out["constraint_ms"] = round(timed(cons, reps), 4)
        out["jacobian_ms"] = round(timed(jac, reps), 4)
        out["hessian_ms"] = round(timed(hes, reps), 4)
        out["iteration_ms"] = round(timed(iteration, reps), 4)
        out["jacobian_slab_GB"] = round(8e-9 * ev.n_jacobian_entries, 3)
        # per-kernel times: one kernel at a time
        ev.set_option("overlap_sweep", 0)
        out["jacobian_serial_ms"] = round(timed(jac, reps), 4)
        ev.profile_enable(True); ev.profile_reset(); jac(); torch.cuda.synchronize()
        chain = ev.profile_get("bgemm")[0] + ev.profile_get("basis")[0]
        out["chain_ms"] = round(chain, 4)
        out["sweep_ms"] = round(ev.profile_get("expmv")[0], 4)
        out["zero_fill_ms"] = round(ev.profile_get("zero_fill")[0], 4)
        if flagged:
            ms, launches, written = ev.profile_get("share")
            n = prob.integrators[0].x_dim
            read = 8.0 * n * n * (prob.trajectory.N - 1)
            out.update({"share_ms": round(ms, 4), "share_launches": launches, "share_GB_written": round(written * 1e-9, 3),
                        "share_TBps": round((written + read) / ms * 1e-9, 3) if ms > 0 else None})
        ev.profile_enable(False)
        return out
    finally:
        ev.close()


def combine(parent_file, new_file):
    """Alternated runs: per shape the spread of every figure and the issue's condition on the Jacobian."""
    def lines(path):
        by = {}
        for l in open(path):
            if l.startswith("{"):
                d = json.loads(l)
                by.setdefault((d["n"], d["knots"], d["kets"]), []).append(d)
        return by
    par, new = lines(parent_file), lines(new_file)
    keys = ("constraint_ms", "jacobian_ms", "hessian_ms", "iteration_ms")
    for shape in sorted(new):
        P = shape[2]
        out = {"n": shape[0], "knots": shape[1], "kets": P, "runs": [len(par.get(shape, [])), len(new[shape])]}
        rng = lambda rows, side, k: [round(f(r[side][k] for r in rows), 4) for f in (min, max)]
        for k in keys:
            out[k] = {"parent": rng(par[shape], "plain", k), "unflagged": rng(new[shape], "plain", k), "shared": rng(new[shape], "shared", k)}
        chain = statistics.median(r["plain"]["chain_ms"] for r in par[shape]) / P
        saved = statistics.median(r["plain"]["jacobian_ms"] for r in par[shape]) - statistics.median(r["shared"]["jacobian_ms"] for r in new[shape])
        out.update({"parent_chain_ms_per_member": round(chain, 4), "jacobian_saved_ms": round(saved, 4),
                    "saved_over_followers_chains": round(saved / ((P - 1) * chain), 3),
                    "share_ms": rng(new[shape], "shared", "share_ms"), "share_TBps": rng(new[shape], "shared", "share_TBps"),
                    "shared_chain_ms": rng(new[shape], "shared", "chain_ms"), "shared_sweep_ms": rng(new[shape], "shared", "sweep_ms"),
                    "parent_sweep_ms": rng(par[shape], "plain", "sweep_ms"), "shared_zero_fill_ms": rng(new[shape], "shared", "zero_fill_ms")})
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="256x2000x4,128x1000x4,64x1000x4", help="comma-separated states x knots x kets")
    ap.add_argument("--drives", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--scale", type=float, default=1.0, help="standard deviation of the generators' entries (1.0: the norms of the\n"
                    "headline benchmark, several squarings per propagator; 0: 1 / sqrt(n), norms of order one)")
    ap.add_argument("--flagged", type=int, default=1, help="0: the unflagged handle alone")
    ap.add_argument("--plain", type=int, default=1, help="0: the flagged handle alone")
    ap.add_argument("--combine", nargs=2, metavar=("PARENT", "NEW"), help="files of this tool's lines from alternated runs of the parent\n"
                    "commit's build (--flagged 0) and of this build: spreads and the condition on the Jacobian")
    a = ap.parse_args()
    if a.combine:
        return combine(*a.combine)
    for s in a.shapes.split(","):
        n, N, P = (int(x) for x in s.lower().split("x"))
        prob = dto_amd.host.synthetic.multi_ket_problem(n, P, a.drives, N, seed=42, u_bound=4.0, scale=a.scale or None)
        out = {"n": n, "knots": N, "kets": P, "drives": a.drives, "scale": a.scale}
        if a.plain:
            out["plain"] = measure_handle(prob, False, a.reps)
        if a.flagged:
            out["shared"] = measure_handle(prob, True, a.reps)
        if a.plain and a.flagged:
            per_member = out["plain"]["chain_ms"] / P
            saved = out["plain"]["jacobian_ms"] - out["shared"]["jacobian_ms"]
            out["chain_ms_per_member"] = round(per_member, 4)
            out["jacobian_saved_ms"] = round(saved, 4)
            out["saved_over_followers_chains"] = round(saved / ((P - 1) * per_member), 3)   # the condition: >= 0.7
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
