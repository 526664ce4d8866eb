#!/usr/bin/env python3
"""Hessian-vector products (dto_eval_hessian_product_dev) on the device, timed with HIP events (a tools/ probe; GPU).

Per shape: eval_hessian_lagrangian alone (device-resident, for comparison); the first product of a handle, split into the
host-side index build (setup), the Hessian and the gather into the compact copy; the first product at a NEW point of a handle
that has its index (re-assembly: the private slab clears only its variable runs); the steady-state product at the cached point
(with its 4-byte compare readback) and the product launch alone with the bytes per second it reaches; the private slab's and
the index's device memory.  One JSON line per shape.

    python tools/hv_time.py                      # 256 x 2000 (BASELINE configs[2]), 64 x 1000, the 1024 x 500 share
    python tools/hv_time.py --shapes 256x16000   # any n x N (m = 4)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import dto_amd  # noqa: E402


def make(n, N):
    if n == 1024:  # the configs[4] workload (bilinear + derivative integrators, L1 slack) on one GPU's share of knots
        return dto_amd.host.synthetic.make_l1_slack_problem(N, n, 4)
    return dto_amd.host.synthetic.make_scaled_problem(N, n, 4, seed=42)


def timed(fn, reps, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(n, N, reps):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = make(n, N)
    ev = dto_amd.Evaluator(prob, eval_hessian=True)
    try:
        g = torch.Generator(device="cpu").manual_seed(1)
        Z = torch.from_numpy(prob.trajectory.vec()).to(dev)
        Z2 = Z + 1e-3 * torch.randn(Z.shape, generator=g, dtype=torch.float64).to(dev)
        mu = torch.randn(ev.n_constraints, generator=g, dtype=torch.float64).to(dev)
        v = [torch.randn(ev.n_variables, generator=g, dtype=torch.float64).to(dev) for _ in range(2)]
        y = torch.empty(ev.n_variables, dtype=torch.float64, device=dev)
        prod = lambda z, vv: ev.eval_hessian_product_dev(z.data_ptr(), 0.7, mu.data_ptr(), vv.data_ptr(), y.data_ptr(), st)
        out = {"shape": f"{n}x{N}", "n_vars": ev.n_variables, "hess_len": ev.n_hessian_entries}
        # the first product of the handle: index build + private slab (allocated and zero-filled in full) + Hessian + gather
        ev.profile_enable(True)
        ev.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prod(Z, v[0])
        torch.cuda.synchronize()
        first = (time.perf_counter() - t0) * 1e3
        setup_ms, _, mem = ev.profile_get("hess_product_setup")
        hp_ms, hp_n, _ = ev.profile_get("hess_product")
        ev.profile_reset()
        prod(Z, v[1])  # cached point: the product launch alone under "hess_product"
        torch.cuda.synchronize()
        k_ms, k_n, k_bytes = ev.profile_get("hess_product")
        ev.profile_enable(False)
        out.update({"first_product_ms": round(first, 3), "setup_ms": round(setup_ms, 3),
                    "gather_ms": round(hp_ms - k_ms, 4), "hessian_in_first_ms": round(first - setup_ms - hp_ms, 3),
                    "memory_GB": round(mem / 1e9, 3)})
        # eval_hessian_lagrangian on its own, device-resident (a buffer of its own)
        H = torch.empty(ev.n_hessian_entries, dtype=torch.float64, device=dev)
        hess = lambda z: ev.eval_hessian_dev(z.data_ptr(), 0.7, mu.data_ptr(), H.data_ptr(), st)
        hess(Z)
        out["eval_hessian_ms"] = round(timed(lambda: hess(Z), reps, st), 3)
        del H
        # a new point on a handle with its index: Hessian (variable runs cleared) + gather + product
        pts = [Z, Z2]
        state = {"i": 0}

        def new_point():
            state["i"] ^= 1
            prod(pts[state["i"]], v[0])
        new_point()
        out["product_new_point_ms"] = round(timed(new_point, reps, st), 3)
        out["ratio_new_point_to_eval_hessian"] = round(out["product_new_point_ms"] / out["eval_hessian_ms"], 3)
        # steady state at the cached point: the compare (one 4-byte readback) + the product
        prod(Z, v[0])
        torch.cuda.synchronize()
        alt = {"i": 0}

        def same_point():
            alt["i"] ^= 1
            prod(Z, v[alt["i"]])
        out["product_cached_us"] = round(timed(same_point, max(50, reps * 10), st) * 1e3, 2)
        out["product_kernel_us"] = round(k_ms / max(k_n, 1) * 1e3, 2)
        out["product_kernel_GBps"] = round(k_bytes / max(k_n, 1) / (k_ms / max(k_n, 1) * 1e-3) / 1e9, 1) if k_ms > 0 else None
        return out
    finally:
        ev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="256x2000,64x1000,1024x500", help="comma-separated n x N")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for s in a.shapes.split(","):
        n, N = (int(x) for x in s.lower().split("x"))
        print(json.dumps(measure(n, N, a.reps)), flush=True)


if __name__ == "__main__":
    main()
