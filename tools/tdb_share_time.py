#!/usr/bin/env python3
"""One propagation per group of TimeDependentBilinearIntegrators (Evaluator(..., shared_generators=True), the group launches of
k_tdb_mfma in csrc/dto_tdb_mfma.hip) against one launch per integrator, timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process: a flagged and an unflagged handle on ``synthetic.multi_ket_modulated_problem(n, kets, drives, N, order,
substeps, n_mods)``; device-resident inputs and outputs; eval_constraint, eval_constraint_jacobian and eval_hessian_lagrangian.  Per
callback a warm-up of at least 30 ms of GPU work on every leg, then ``--reps`` rounds of one call on each leg, alternated: the
unflagged handle (the yardstick), the flagged handle, and the flagged handle with ``tdb_share_members`` = 1 (one launch per member
through the same handle: the A/B switch).  Medians, the ratios flagged / unflagged, the kernel's own time, launches and FP64 rate as
executed (dto_profile_get "tdb_mfma"), and the scratch of one resident workgroup at the group's launch size.  ``kets`` = 1 times a
lone integrator (the unflagged handle alone).  One JSON line per shape.

    python tools/tdb_share_time.py                           # 128 x 500 x 2 and 128 x 500 x 4: 4 drives, two carriers, 16 sub-steps, order 1
    python tools/tdb_share_time.py --shapes 128x500x1        # the lone integrator
    python tools/tdb_share_time.py --shapes 72x200x3 --hessian 0
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


def group_scratch_MB(n, drives, order, n_mods, members, need):
    """Doubles of one resident workgroup's slot in a group launch (tdbm_layout of csrc/dto_tdb_mfma_layout.h), in MB."""
    pad32 = lambda v: (v + 31) // 32 * 32
    np_, p = pad32(n), drives + 2 + (drives if order else 0)
    P2, Q = p * (p + 1) // 2, (drives + 1) * (1 + n_mods)
    c1 = (1, 1 + p, 1 + p + P2)[need]
    stride = pad32(c1) if need == 2 else c1
    ctot = pad32(members * stride) + (np_ if need == 1 else 0)
    ucols = members * (32 if need == 2 else 1)
    total = 4 * np_ * ctot + np_ * np_ + Q * ucols * np_ + (np_ * 32 * members if need == 2 else 0) + (1 + p + P2) * Q
    return round(8e-6 * total, 3)


def measure(prob, kets, reps, hessian, sigma=0.7):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    evs = {"unflagged": dto_amd.Evaluator(prob, eval_hessian=hessian)}
    if kets >= 2:
        evs["flagged"] = dto_amd.Evaluator(prob, eval_hessian=hessian, shared_generators=True)
    try:
        e0 = evs["unflagged"]
        Z = torch.from_numpy(prob.trajectory.vec()).to(dev)
        mu = torch.randn(e0.n_constraints, generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float64).to(dev)
        con = torch.empty(e0.n_constraints, dtype=torch.float64, device=dev)
        J = torch.empty(e0.n_jacobian_entries, dtype=torch.float64, device=dev)
        H = torch.empty(e0.n_hessian_entries if hessian else 1, dtype=torch.float64, device=dev)
        out = {"share": evs["flagged"].integrator_share(0)} if kets >= 2 else {}

        def calls(ev):
            c = {"constraint": lambda: ev.eval_constraint_dev(Z.data_ptr(), con.data_ptr(), st),
                 "jacobian": lambda: ev.eval_jacobian_dev(Z.data_ptr(), J.data_ptr(), st)}
            if hessian:
                c["hessian"] = lambda: ev.eval_hessian_dev(Z.data_ptr(), sigma, mu.data_ptr(), H.data_ptr(), st)
            return c

        # legs: (name, handle, tdb_share_members or None)
        legs = [("unflagged", evs["unflagged"], None)]
        if kets >= 2:
            legs += [("flagged", evs["flagged"], kets), ("flagged_members_1", evs["flagged"], 1)]
        fns = {k: calls(ev) for k, ev in evs.items()}

        def run(leg, name):
            lname, ev, members = leg
            if members is not None:
                ev.set_option("tdb_share_members", min(members, out["share"][1]))
            return fns["unflagged" if lname == "unflagged" else "flagged"][name]

        for name in fns["unflagged"]:
            for leg in legs:
                fn, spent = run(leg, name), 0.0
                while spent < 30.0:
                    spent += one_call_ms(fn)
            ts = {leg[0]: [] for leg in legs}
            for _ in range(reps):
                for leg in legs:
                    ts[leg[0]].append(one_call_ms(run(leg, name)))
            for leg in legs:
                lname, ev, _ = leg
                out[f"{lname}_{name}_ms"] = round(statistics.median(ts[lname]), 4)
                fn = run(leg, name)
                ev.profile_enable(True); ev.profile_reset(); fn(); torch.cuda.synchronize()
                ms, launches, fl = ev.profile_get("tdb_mfma")
                ev.profile_enable(False)
                out[f"{lname}_{name}_tdb_mfma"] = {"ms": round(ms, 4), "launches": launches, "TFLOPs": round(fl / ms * 1e-9, 3) if ms > 0 else None}
            if kets >= 2:
                out[f"{name}_flagged_over_unflagged"] = round(out[f"flagged_{name}_ms"] / out[f"unflagged_{name}_ms"], 4)
                out[f"{name}_members_1_over_unflagged"] = round(out[f"flagged_members_1_{name}_ms"] / out[f"unflagged_{name}_ms"], 4)
        return out
    finally:
        for ev in evs.values():
            ev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="128x500x2,128x500x4", help="comma-separated states x knots x kets")
    ap.add_argument("--drives", type=int, default=4)
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--substeps", type=int, default=16)
    ap.add_argument("--mods", type=int, default=2, help="carrier terms (0 .. 2)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hessian", type=int, default=1)
    a = ap.parse_args()
    for s in [x for x in a.shapes.split(",") if x]:
        n, N, P = (int(x) for x in s.lower().split("x"))
        prob = dto_amd.synthetic.multi_ket_modulated_problem(n, P, a.drives, N, order=a.order, substeps=a.substeps, n_mods=a.mods)
        out = {"n": n, "knots": N, "kets": P, "drives": a.drives, "order": a.order, "substeps": a.substeps, "mods": a.mods}
        out.update(measure(prob, P, a.reps, bool(a.hessian)))
        if P >= 2:
            g = out["share"][1]
            out["scratch_MB_per_workgroup"] = {k: group_scratch_MB(n, a.drives, a.order, a.mods, g, need)
                                               for need, k in enumerate(("constraint", "jacobian", "hessian"))}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
