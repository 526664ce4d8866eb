#!/usr/bin/env python3
"""Reduced-space gradient and Hessian-vector product on the device (Evaluator.reduced_gradient_dev, reduced_hessian_product_dev)
beside the same process's hand composition through the existing `_dev` entry points, timed with HIP events (a tools/ probe; GPU).

Per shape, in ONE process, on ``synthetic.multi_ket_problem(n, 1, drives, N, scale)`` -- one ket with skew-symmetric generators, its
DerivativeIntegrator(u, du) and the knot constraint on u -- with device-resident inputs and outputs, sigma = 0.7 and a random mu on
the constraint rows; every figure after a warm-up of at least 30 ms of GPU work, the median of ``--reps`` single-call timings:

    reduced_gradient_dev and reduced_hessian_product_dev at a NEW point (two points that differ in one bit of a control alternate, so
        every call computes the reduced point: gradient, Jacobian with trees, costates, and for the product the Hessian assembly) and
        at the CACHED point (the gradient copies its result; the product runs steps 1 .. 8 of the header alone);
    the HAND COMPOSITION of the same steps -- the yardstick: the same kernels through eval_gradient_dev,
        eval_jacobian_product_dev, eval_jacobian_transpose_product_dev, dynamics_solve_all_dev and eval_hessian_product_dev, with the
        caller's own repacking in torch indexing on the device -- new and cached (cached: mu~ kept by the caller, steps 1 .. 8);
    the profile split of one cached product: "reduced_pack", "hess_product", "dynsolve_scan", "dynsolve_couple", "dynsolve_deriv";
    with ``--host-shape`` the host-vector Python Evaluator.reduced_gradient(Z) at that shape: what a user had before;
    the two ROUTES of the operators -- the default one and option "reduced_input_store" = 1 (J v^ and J' w from the kept input
        blocks) -- on two handles of the same problem in the same process, their single calls ALTERNATING (default, store, default,
        ...), the median of ``--reps`` each: gradient and product at a new point, product at the kept point; per route the profile
        split of one kept product with its device total, "reduced_input" with its bytes as executed, the store's size, and the
        largest difference between the routes' results.

One JSON line per shape, and a second one ({"routes": ...}) for the routes; ``--routes only`` prints the second alone.
``--block`` instead times the BLOCK products at the kept point, both routes in one process: for n_cols in 1, 4, 16, 64 and chunk widths
(option "reduced_block_width") 16, 32, 64 one reduced_hessian_products_dev call against a loop of n_cols reduced_hessian_product_dev
calls -- the single path is the yardstick -- the two ALTERNATING, medians of ``--reps``; the same for eval_hessian_products_dev against
eval_hessian_product_dev; and on the store route the per-name profile of one block of 16 and of one single product with
"overlap_sweep" = 0.  One JSON line ({"block": ...}) per shape.

    python tools/reduced_time.py                       # 256 x 2000 and 64 x 1000, host-vector gradient at 64 x 1000
    python tools/reduced_time.py --shapes 128x1000 --reps 9
    python tools/reduced_time.py --block
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

PARTS = ("reduced_pack", "hess_product", "dynsolve_scan", "dynsolve_couple", "dynsolve_deriv", "dynsolve_tree")
OWN = ("reduced_input", "reduced_pack", "dynsolve_scan", "dynsolve_couple", "dynsolve_deriv", "dynsolve_tree")   # names "all" leaves out
SIGMA = 0.7


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


class Hand:
    """the operators out of today's `_dev` entry points, repacked with torch indexing on the device"""

    def __init__(self, ev, prob, dev, st):
        self.ev, self.st, self.dev = ev, st, dev
        tr = prob.trajectory
        self.N, self.z = tr.N, tr.dim
        self.D, _, offset, _ = ev.dynamics_layout()
        self.its = [(it.x_off, it.x_dim, int(offset[i]), ev._integrator_row0[i]) for i, it in enumerate(prob.integrators)]
        self.n_dyn = ev.n_dynamics_constraints
        f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        self.G, self.t, self.q, self.zh = f(ev.n_variables), f(ev.n_variables), f(ev.n_variables), f(ev.n_variables)
        self.w, self.rho, self.mut = f(ev.n_constraints), f(ev.n_constraints), f(ev.n_constraints)
        self.B, self.L, self.Y = f(self.N, 1, self.D), f(self.N, 1, self.D), f(self.N, 1, self.D)

    def knots(self, x):
        return x[:self.N * self.z].view(self.N, self.z)

    def pack(self, x, B):
        xk = self.knots(x)
        for x_off, d, off, _ in self.its:
            B[:, 0, off:off + d] = xk[:, x_off:x_off + d]

    def rows(self, L, w):
        w.zero_()
        for _, d, off, row0 in self.its:
            w[row0:row0 + (self.N - 1) * d] = L[1:, 0, off:off + d].reshape(-1)

    def finish(self, q, t, L):
        y = q - t
        yk = self.knots(y)
        for x_off, d, off, _ in self.its:
            yk[:, x_off:x_off + d] = 0.0
            yk[0, x_off:x_off + d] = L[0, 0, off:off + d]
        return y

    def gradient(self, Z, mu):
        ev, st, p = self.ev, self.st, Z.data_ptr()
        ev.eval_gradient_dev(p, self.G.data_ptr(), st)
        g = SIGMA * self.G
        if mu is not None:
            self.w.copy_(mu)
            self.w[:self.n_dyn] = 0.0
            ev.eval_jacobian_transpose_product_dev(p, self.w.data_ptr(), self.t.data_ptr(), st)
            g = g + self.t
        self.pack(g, self.B)
        ev.dynamics_solve_all_dev(p, self.B.data_ptr(), 1, self.L.data_ptr(), adjoint=True, stream=st)
        self.rows(self.L, self.w)
        ev.eval_jacobian_transpose_product_dev(p, self.w.data_ptr(), self.t.data_ptr(), st)
        torch.neg(self.w, out=self.mut)
        self.mut[self.n_dyn:] = mu[self.n_dyn:] if mu is not None else 0.0
        return self.finish(g, self.t, self.L)

    def product(self, Z, v):
        """steps 1 .. 8 with the mu~ of the last gradient"""
        ev, st, p = self.ev, self.st, Z.data_ptr()
        self.zh.copy_(v)
        zk = self.knots(self.zh)
        for x_off, d, _, _ in self.its:
            zk[:, x_off:x_off + d] = 0.0
        ev.eval_jacobian_product_dev(p, self.zh.data_ptr(), self.rho.data_ptr(), st)
        vk = self.knots(v)
        for x_off, d, off, row0 in self.its:
            self.B[0, 0, off:off + d] = vk[0, x_off:x_off + d]
            self.B[1:, 0, off:off + d] = -self.rho[row0:row0 + (self.N - 1) * d].view(self.N - 1, d)
        ev.dynamics_solve_all_dev(p, self.B.data_ptr(), 1, self.Y.data_ptr(), stream=st)
        for x_off, d, off, _ in self.its:
            zk[:, x_off:x_off + d] = self.Y[:, 0, off:off + d]
        ev.eval_hessian_product_dev(p, SIGMA, self.mut.data_ptr(), self.zh.data_ptr(), self.q.data_ptr(), st)
        self.pack(self.q, self.B)
        ev.dynamics_solve_all_dev(p, self.B.data_ptr(), 1, self.L.data_ptr(), adjoint=True, stream=st)
        self.rows(self.L, self.w)
        ev.eval_jacobian_transpose_product_dev(p, self.w.data_ptr(), self.t.data_ptr(), st)
        return self.finish(self.q, self.t, self.L)


def measure(n, N, drives, scale, reps, host_gradient):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    ev = dto_amd.Evaluator(prob)
    out = {"n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps, "sigma": SIGMA}
    try:
        it = prob.integrators[0]
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Zh2 = Zh.copy()
        Zh2[it.u_off] = np.nextafter(Zh2[it.u_off], np.inf)           # the other point: one bit of one control
        Z, Z2 = torch.from_numpy(Zh).to(dev), torch.from_numpy(Zh2).to(dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        mu = torch.randn(ev.n_constraints, dtype=torch.float64, device=dev, generator=gen)
        v = torch.randn(ev.n_variables, dtype=torch.float64, device=dev, generator=gen)
        r = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dev)
        y = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dev)
        hand = Hand(ev, prob, dev, st)
        out["n_variables"], out["n_constraints"], out["n_states"] = ev.n_variables, ev.n_constraints, hand.D
        flip = [0]

        def point():
            flip[0] ^= 1
            return Z2 if flip[0] else Z

        grad = lambda Zp: ev.reduced_gradient_dev(Zp.data_ptr(), SIGMA, mu.data_ptr(), r.data_ptr(), 0, st)
        prod = lambda Zp: ev.reduced_hessian_product_dev(Zp.data_ptr(), SIGMA, mu.data_ptr(), v.data_ptr(), y.data_ptr(), st)

        def hand_new_product():
            Zp = point()
            hand.gradient(Zp, mu)
            return hand.product(Zp, v)

        out["gradient_new_ms"] = round(timed(lambda: grad(point()), reps), 4)
        grad(Z); torch.cuda.synchronize()
        out["gradient_cached_ms"] = round(timed(lambda: grad(Z), reps), 4)
        out["product_new_ms"] = round(timed(lambda: prod(point()), reps), 4)
        prod(Z); torch.cuda.synchronize()
        out["product_cached_ms"] = round(timed(lambda: prod(Z), reps), 4)
        y_engine, r_engine = y.clone(), None
        grad(Z); torch.cuda.synchronize()
        r_engine = r.clone()
        out["hand_gradient_new_ms"] = round(timed(lambda: hand.gradient(point(), mu), reps), 4)
        out["hand_product_new_ms"] = round(timed(hand_new_product, reps), 4)
        r_hand = hand.gradient(Z, mu); torch.cuda.synchronize()
        out["hand_product_cached_ms"] = round(timed(lambda: hand.product(Z, v), reps), 4)
        y_hand = hand.product(Z, v); torch.cuda.synchronize()
        out["same_bits_as_hand"] = bool(torch.equal(r_hand, r_engine) and torch.equal(y_hand, y_engine))
        prod(Z); torch.cuda.synchronize()
        ev.profile_enable(True); ev.profile_reset(); prod(Z); torch.cuda.synchronize()
        split = {}
        for part in PARTS:
            ms, launches, work = ev.profile_get(part)
            split[part] = {"ms": round(ms, 4), "launches": launches, "gflop_or_GB": round(work * 1e-9, 5)}
        ev.profile_enable(False)
        out["split_cached_product"] = split
        if host_gradient:
            ev.reduced_gradient(Zh)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter(); ev.reduced_gradient(Zh); ts.append(1e3 * (time.perf_counter() - t0))
            out["host_vector_python_reduced_gradient_cached_ms"] = round(statistics.median(ts), 4)
            ts = []
            for i in range(reps):
                t0 = time.perf_counter(); ev.reduced_gradient(Zh2 if i % 2 == 0 else Zh); ts.append(1e3 * (time.perf_counter() - t0))
            out["host_vector_python_reduced_gradient_new_ms"] = round(statistics.median(ts), 4)
        return out
    finally:
        ev.close()


def alternating(fns, reps):
    """medians of `reps` single calls of each function, the functions taking turns; after at least 30 ms of GPU work each"""
    for fn in fns:
        spent = 0.0
        while spent < 30.0:
            spent += one_call_ms(fn)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(one_call_ms(fn))
    return [round(statistics.median(t), 4) for t in ts]


def measure_routes(n, N, drives, scale, reps):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    evs = [dto_amd.Evaluator(prob), dto_amd.Evaluator(prob)]
    out = {"n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps, "sigma": SIGMA, "routes": ["default", "reduced_input_store"]}
    try:
        evs[1].set_option("reduced_input_store", 1)
        it = prob.integrators[0]
        Zh = np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)
        Zh2 = Zh.copy()
        Zh2[it.u_off] = np.nextafter(Zh2[it.u_off], np.inf)
        Z, Z2 = torch.from_numpy(Zh).to(dev), torch.from_numpy(Zh2).to(dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        mu = torch.randn(evs[0].n_constraints, dtype=torch.float64, device=dev, generator=gen)
        v = torch.randn(evs[0].n_variables, dtype=torch.float64, device=dev, generator=gen)
        rs = [torch.full((evs[0].n_variables,), float("nan"), dtype=torch.float64, device=dev) for _ in evs]
        ys = [torch.full((evs[0].n_variables,), float("nan"), dtype=torch.float64, device=dev) for _ in evs]
        flips = [[0], [0]]

        def point(i):
            flips[i][0] ^= 1
            return Z2 if flips[i][0] else Z

        grad = lambda i, Zp: evs[i].reduced_gradient_dev(Zp.data_ptr(), SIGMA, mu.data_ptr(), rs[i].data_ptr(), 0, st)
        prod = lambda i, Zp: evs[i].reduced_hessian_product_dev(Zp.data_ptr(), SIGMA, mu.data_ptr(), v.data_ptr(), ys[i].data_ptr(), st)
        out["gradient_new_ms"] = alternating([lambda i=i: grad(i, point(i)) for i in (0, 1)], reps)
        out["product_new_ms"] = alternating([lambda i=i: prod(i, point(i)) for i in (0, 1)], reps)
        for i in (0, 1):
            grad(i, Z); prod(i, Z)
        torch.cuda.synchronize()
        out["product_kept_ms"] = alternating([lambda i=i: prod(i, Z) for i in (0, 1)], reps)
        scale_y, scale_r = float(ys[0].abs().max()), float(rs[0].abs().max())
        out["largest_difference_between_routes"] = {"product": float((ys[0] - ys[1]).abs().max()), "product_scale": scale_y,
                                                    "gradient": float((rs[0] - rs[1]).abs().max()), "gradient_scale": scale_r}
        splits = []
        for i, ev in enumerate(evs):
            ev.profile_enable(True); ev.profile_reset(); prod(i, Z); torch.cuda.synchronize()
            split, total = {}, ev.profile_get("all")[0]
            for part in OWN + ("hess_product", "jac_product", "expmv", "all"):
                ms, launches, work = ev.profile_get(part)
                split[part] = {"ms": round(ms, 4), "launches": launches, "gflop_or_GB": round(work * 1e-9, 5)}
                total += ms if part in OWN else 0.0
            split["device_total_ms"] = round(total, 4)
            ev.profile_enable(False)
            splits.append(split)
        out["split_kept_product"] = splits
        out["reduced_input_bytes_as_executed"] = evs[1].profile_get("reduced_input")[2]
        return out
    finally:
        for ev in evs:
            ev.close()


BLOCK_COLS = (1, 4, 16, 64)
BLOCK_WIDTHS = (16, 32, 64)
BLOCK_PARTS = ("reduced_input", "reduced_pack", "hess_product", "dynsolve_scan", "dynsolve_couple", "dynsolve_deriv", "jac_product", "expmv")


def measure_block(n, N, drives, scale, reps):
    """--block: the block products against loops of single products at the kept point, both routes in one process"""
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    prob = dto_amd.host.synthetic.multi_ket_problem(n, 1, drives, N, seed=42, u_bound=4.0, scale=scale or None)
    routes = ("default", "reduced_input_store")
    evs = [dto_amd.Evaluator(prob), dto_amd.Evaluator(prob)]
    out = {"n": n, "knots": N, "drives": drives, "scale": scale, "reps": reps, "sigma": SIGMA, "n_cols": list(BLOCK_COLS), "widths": list(BLOCK_WIDTHS)}
    try:
        evs[1].set_option("reduced_input_store", 1)
        nv = evs[0].n_variables
        Z = torch.from_numpy(np.ascontiguousarray(prob.trajectory.vec(), dtype=np.float64)).to(dev)
        gen = torch.Generator(device=dev); gen.manual_seed(7)
        mu = torch.randn(evs[0].n_constraints, dtype=torch.float64, device=dev, generator=gen)
        V = torch.randn(max(BLOCK_COLS), nv, dtype=torch.float64, device=dev, generator=gen)
        Y = torch.full((max(BLOCK_COLS), nv), float("nan"), dtype=torch.float64, device=dev)
        Y1 = torch.full((max(BLOCK_COLS), nv), float("nan"), dtype=torch.float64, device=dev)
        out["n_variables"] = nv
        for ev, route in zip(evs, routes):
            def block(k, ev=ev):
                ev.reduced_hessian_products_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), k, V.data_ptr(), Y.data_ptr(), st)

            def loop(k, ev=ev):
                for c in range(k):
                    ev.reduced_hessian_product_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), V[c].data_ptr(), Y1[c].data_ptr(), st)

            table, same = {}, True
            for width in BLOCK_WIDTHS:
                ev.set_option("reduced_block_width", width)       # (drops the kept points: the next calls build them again)
                block(1); loop(1); torch.cuda.synchronize()
                row = {}
                for k in BLOCK_COLS:
                    b, l = alternating([lambda: block(k), lambda: loop(k)], reps)
                    same = same and bool(torch.equal(Y[:k], Y1[:k]))
                    row[str(k)] = {"block_ms": b, "singles_ms": l, "ratio": round(b / l, 4), "block_ms_per_column": round(b / k, 4)}
                table[str(width)] = row
            out[route] = {"projected": table, "same_bits_as_singles": same}
            if route == "reduced_input_store":                    # which part scales: the per-name profile of one block of 16 and of one single
                ev.set_option("overlap_sweep", 0)
                ev.set_option("reduced_block_width", 16)
                split = {}
                for what, fn in (("block_16", lambda: block(16)), ("single", lambda: loop(1))):
                    fn(); torch.cuda.synchronize()
                    ev.profile_enable(True); ev.profile_reset(); fn(); torch.cuda.synchronize()
                    split[what] = {part: {"ms": round(ev.profile_get(part)[0], 4), "launches": ev.profile_get(part)[1],
                                          "GB": round(ev.profile_get(part)[2] * 1e-9, 5)} for part in BLOCK_PARTS}
                    ev.profile_enable(False)
                ev.set_option("overlap_sweep", 1)
                out["split_store_route"] = split
        # H V alone (the caller's [n_cols][n_vars] planes), on the default-route handle: the option does not reach it
        ev = evs[0]
        htable = {}
        for width in BLOCK_WIDTHS:
            ev.set_option("reduced_block_width", width)
            ev.eval_hessian_product_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), V[0].data_ptr(), Y1[0].data_ptr(), st); torch.cuda.synchronize()
            row = {}
            for k in BLOCK_COLS:
                def hb(k=k):
                    ev.eval_hessian_products_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), k, V.data_ptr(), Y.data_ptr(), st)

                def hl(k=k):
                    for c in range(k):
                        ev.eval_hessian_product_dev(Z.data_ptr(), SIGMA, mu.data_ptr(), V[c].data_ptr(), Y1[c].data_ptr(), st)
                b, l = alternating([hb, hl], reps)
                row[str(k)] = {"block_ms": b, "singles_ms": l, "ratio": round(b / l, 4), "same_bits": bool(torch.equal(Y[:k], Y1[:k]))}
            htable[str(width)] = row
        out["hessian_products"] = htable
        return out
    finally:
        for ev in evs:
            ev.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", default="256x2000,64x1000", help="comma-separated states x knots")
    ap.add_argument("--host-shape", default="64x1000", help="the shape at which the host-vector Python reduced_gradient is timed too")
    ap.add_argument("--drives", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="standard deviation of the generators' entries (1.0: the norms of the\n"
                    "headline benchmark, several squarings per propagator; 0: 1 / sqrt(n), norms of order one)")
    ap.add_argument("--routes", default="yes", choices=("yes", "no", "only"), help="the default route beside option reduced_input_store = 1")
    ap.add_argument("--block", action="store_true", help="the block products (reduced_hessian_products_dev, eval_hessian_products_dev)\n"
                    "against loops of single products at the kept point, per route, chunk width and column count; nothing else")
    a = ap.parse_args()
    for s in a.shapes.split(","):
        n, N = (int(x) for x in s.lower().split("x"))
        if a.block:
            print(json.dumps({"block": measure_block(n, N, a.drives, a.scale, a.reps)}), flush=True)
            continue
        if a.routes != "only":
            print(json.dumps(measure(n, N, a.drives, a.scale, a.reps, s.lower() == a.host_shape.lower())), flush=True)
        if a.routes != "no":
            print(json.dumps({"routes": measure_routes(n, N, a.drives, a.scale, a.reps)}), flush=True)


if __name__ == "__main__":
    main()
