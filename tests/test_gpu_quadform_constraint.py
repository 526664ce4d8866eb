"""GPU: the quadratic-form knot constraint g(v) = [v' M v - c] (DTO_CONSTRAINT_QUADFORM_MINUS_C, csrc/dto_quadform.hip) and the
cooperative kernels of the low-rank infidelity objective.  Expected values are the oracle's closure form of the same term
(analytic g, 2 (M v)', 2 mu M): 1e-10 max(1, |ref|) for values, Jacobian and products, 1e-8 max(1, |ref|) for the Hessian and
H v, indices bit-exact.  Handles run with host_xfer_check on (tests/conftest.py)."""
import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import TOL, TOL_H, rel_err, run_all
from quadform_cases import check_against_oracle, check_structure, sym, to_oracle, with_quadforms

pytestmark = pytest.mark.gpu


def run_case(base, specs, Z=None, tag="", seed=0):
    prob_o, prob_e, _ = with_quadforms(base, specs)
    ev_o = O.OracleEvaluator(prob_o)
    ev = dto_amd.Evaluator(prob_e)
    try:
        return check_against_oracle(ev, ev_o, prob_o, Z=Z, seed=seed, tag=tag)
    finally:
        ev.close()


@pytest.mark.parametrize("n,equality", [(6, False), (8, True), (7, False)])
def test_small_dense_form_at_all_knots(n, equality):
    N, m = 6, 2
    base = O.make_scaled_problem(N, n, m, seed=20 + n, with_constraint=True)
    M = sym(np.random.default_rng(n), n)
    run_case(base, [dict(comps=list(range(n)), times1=list(range(1, N + 1)), M=M, c=0.4, equality=equality)], tag=f"dense n={n}")


def test_a_knot_listed_twice_keeps_the_later_hessian_block():
    N, n, m = 7, 6, 2
    base = O.make_scaled_problem(N, n, m, seed=31)
    M = sym(np.random.default_rng(31), n)
    run_case(base, [dict(comps=list(range(n)), times1=[2, 5, 2, 7, 5, 5], M=M, c=-0.2, equality=False)], tag="repeated knot")


def test_components_of_two_trajectory_components_in_descending_order():
    N, n, m = 6, 5, 3
    base = O.make_scaled_problem(N, n, m, seed=32, with_constraint=True)
    comps = [n + 1, 3, n + m + 2, 0, n]  # u_1, x_3, du_2, x_0, u_0
    M = sym(np.random.default_rng(32), len(comps))
    run_case(base, [dict(comps=comps, times1=[1, 3, 4, 6], M=M, c=1.5, equality=True)], tag="mixed comps")


def test_zero_rows_of_the_matrix():
    N, n, m = 6, 8, 2
    base = O.make_scaled_problem(N, n, m, seed=33)
    M = sym(np.random.default_rng(33), n)
    M[[2, 5], :] = 0.0
    M[:, [2, 5]] = 0.0
    out, _ = run_case(base, [dict(comps=list(range(n)), times1=[2, 3, 6], M=M, c=0.0, equality=False)], tag="zero rows")


def test_entries_outside_the_pattern_of_the_initial_point_are_dropped():
    """v0 = 0 at knot 3: the row has no entries, and stays without at a point where 2 (M v) is non-zero."""
    N, n, m = 6, 6, 2
    base = O.make_scaled_problem(N, n, m, seed=34)
    base.Z0.reshape(N, base.z)[2, :n] = 0.0
    M = sym(np.random.default_rng(34), n)
    Z = base.Z0 + 0.1 * np.random.default_rng(35).standard_normal(base.Z0.size)
    prob_o, prob_e, _ = with_quadforms(base, [dict(comps=list(range(n)), times1=[2, 3, 5], M=M, c=0.3, equality=False)])
    ev_o = O.OracleEvaluator(prob_o)
    ev = dto_amd.Evaluator(prob_e)
    try:
        rows, _ = ev.jacobian_structure()
        assert np.count_nonzero(rows == ev_o.n_dynamics_constraints + 2) == 0  # the listing of knot 3
        assert np.all(2.0 * (M @ Z.reshape(N, base.z)[2, :n]) != 0.0)
        check_against_oracle(ev, ev_o, prob_o, Z=Z, tag="dropped entries")
    finally:
        ev.close()


def test_ket_fidelity_bound():
    """make_ket_problem's shape: the bound F(psi_t) >= F_min as M = -A'A, c = -F_min, at the last knot and at interior knots (one
    twice), next to the low-rank infidelity objective on the same components."""
    base = O.make_ket_problem()
    A = O.ket_fidelity_factor(np.array([0.6, 0.0, 0.0, 0.8]))
    M = -(A.T @ A)
    M = 0.5 * (M + M.T)
    run_case(base, [dict(comps=[0, 1, 2, 3], times1=[base.N], M=M, c=-0.99, equality=False),
                    dict(comps=[0, 1, 2, 3], times1=[2, 3, 3, 5], M=M, c=-0.5, equality=False)], tag="ket bound")


@pytest.mark.parametrize("levels,N,blocks", [(4, 6, (8, 4, 0)), (8, 5, (16, 8, 1)), (16, 3, (32, 16, 1))])
def test_unitary_minimum_time_problem(levels, N, blocks):
    pe = dto_amd.synthetic.unitary_minimum_time_problem(levels, 2, N, fidelity=0.9, seed=7)
    prob_o = to_oracle(pe)
    ev_o = O.OracleEvaluator(prob_o)
    for flagged in (True, False):
        ev = dto_amd.Evaluator(pe, block_generators=flagged)
        try:
            assert ev.integrator_blocks(0) == (blocks if flagged else (2 * levels * levels, 1, 0)), ev.integrator_blocks(0)
            check_against_oracle(ev, ev_o, prob_o, tag=f"minimum time, {levels} levels, flagged={flagged}")
        finally:
            ev.close()


def test_built_in_kind_and_host_closure_agree():
    N, n, m = 6, 7, 2
    base = O.make_scaled_problem(N, n, m, seed=36, with_constraint=True)
    rng = np.random.default_rng(36)
    specs = [dict(comps=list(range(n)), times1=[1, 4, 4, 6], M=sym(rng, n), c=0.7, equality=False),
             dict(comps=[n + 1, 2, n], times1=[2, 3], M=sym(rng, 3), c=0.0, equality=True)]
    prob_o, prob_e, prob_c = with_quadforms(base, specs)
    a, b = dto_amd.Evaluator(prob_e), dto_amd.Evaluator(prob_c)
    try:
        for sa, sb in ((a.jacobian_structure(), b.jacobian_structure()), (a.hessian_lagrangian_structure(), b.hessian_lagrangian_structure()),
                       (a.constraint_bounds(), b.constraint_bounds())):
            assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
        Z = base.Z0 + 0.05 * rng.standard_normal(base.Z0.size)
        mu = rng.standard_normal(a.n_constraints)
        oa, ob = run_all(a, None, Z, mu, 0.7), run_all(b, None, Z, mu, 0.7)
        figures = {k: rel_err(oa[k], ob[k]) for k in ("cons", "jac", "hess")}
        print(figures)
        assert figures["cons"] <= TOL and figures["jac"] <= TOL and figures["hess"] <= TOL_H, figures
    finally:
        a.close(); b.close()


def minimum_time(N=12):
    return dto_amd.synthetic.unitary_minimum_time_problem(8, 2, N, fidelity=0.9, seed=5)


@pytest.mark.parametrize("ranges", [((1, 5), (6, 12)), ((1, 4), (5, 8), (9, 12))])
def test_shards_are_slices_of_the_whole(ranges):
    pe = minimum_time()
    Z = pe.trajectory.vec()
    whole = dto_amd.Evaluator(pe, block_generators=True)
    try:
        mu = np.random.default_rng(6).standard_normal(whole.n_constraints)
        ow = run_all(whole, None, Z, mu, 0.7)
        parts = {k: [] for k in ("jac", "hess", "grad")}
        for lo, hi in ranges:
            ev = dto_amd.Evaluator(pe, block_generators=True, k_lo=lo, k_hi=hi)
            try:
                o = run_all(ev, None, Z, mu, 0.7)
                for k in parts:
                    parts[k].append(o[k])
                starts, lens = ev.shard_rows()
                ref = np.concatenate([ow["cons"][a - 1:a - 1 + n] for a, n in zip(starts, lens)])
                assert np.array_equal(o["cons"], ref)
                # the terminal listing (the last NLP row) lands in the last shard only
                has_last = any(a - 1 + n == whole.n_constraints for a, n in zip(starts, lens))
                assert has_last == (hi == pe.trajectory.N)
            finally:
                ev.close()
        for k in parts:
            assert np.array_equal(np.concatenate(parts[k]), ow[k]), k
    finally:
        whole.close()


def _device_setup(pe, flagged=True, seed=4):
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    ev = dto_amd.Evaluator(pe, block_generators=flagged)
    dZ = torch.from_numpy(pe.trajectory.vec()).to(dev)
    dmu = torch.from_numpy(np.random.default_rng(seed).standard_normal(ev.n_constraints)).to(dev)
    return torch, dev, st, ev, dZ, dmu


def _device_calls(torch, dev, st, ev, dZ, dmu):
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    f, gr, g, J, H = nan(1), nan(ev.shard.grad_len), nan(ev.shard.cons_len), nan(ev.shard.jac_len), nan(ev.shard.hess_len)
    ev.eval_objective_dev(dZ.data_ptr(), f.data_ptr(), st)
    ev.eval_gradient_dev(dZ.data_ptr(), gr.data_ptr(), st)
    ev.eval_constraint_dev(dZ.data_ptr(), g.data_ptr(), st)
    ev.eval_jacobian_dev(dZ.data_ptr(), J.data_ptr(), st)
    ev.eval_hessian_dev(dZ.data_ptr(), 0.7, dmu.data_ptr(), H.data_ptr(), st)
    torch.cuda.synchronize()
    return {"f": f, "grad": gr, "cons": g, "jac": J, "hess": H}


def test_repeated_calls_and_device_pointers_give_the_same_bits():
    pe = minimum_time()
    torch, dev, st, ev, dZ, dmu = _device_setup(pe)
    try:
        runs = [_device_calls(torch, dev, st, ev, dZ, dmu) for _ in range(3)]
        for other in runs[1:]:
            for k in runs[0]:
                assert torch.equal(runs[0][k], other[k]), k
        Z, mu = dZ.cpu().numpy(), dmu.cpu().numpy()
        hosts = [run_all(ev, None, Z, mu, 0.7) for _ in range(3)]
        for k in ("grad", "cons", "jac", "hess"):
            for o in hosts:
                assert np.array_equal(o[k], runs[0][k].cpu().numpy()), k
        assert all(o["f"] == float(runs[0]["f"][0]) for o in hosts)
        w = np.random.default_rng(8).standard_normal(ev.n_variables)
        wt = np.random.default_rng(9).standard_normal(ev.n_constraints)
        prods = []
        for _ in range(3):
            y1 = np.full(ev.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y1, Z, w)
            y2 = np.full(ev.n_variables, np.nan); ev.eval_constraint_jacobian_transpose_product(y2, Z, wt)
            y3 = np.full(ev.n_variables, np.nan); ev.eval_hessian_lagrangian_product(y3, Z, w, 0.7, mu)
            prods.append((y1, y2, y3))
        for other in prods[1:]:
            for x, y in zip(prods[0], other):
                assert np.array_equal(x, y)
    finally:
        ev.close()


def test_bound_output_leaves_constant_entries_alone():
    """Bound Jacobian and Hessian vectors on the minimum-time problem: right after every call at three points, and an entry the
    hand-off plan calls constant, marked after priming, is still marked after the next call."""
    from dto_amd import capi
    pe = minimum_time()
    torch, dev, st, ev, dZ0, dmu0 = _device_setup(pe)
    ref = dto_amd.Evaluator(pe, block_generators=True)
    try:
        rng = np.random.default_rng(0)
        Z0 = pe.trajectory.vec()
        dZ = [torch.from_numpy(Z0 + 0.05 * k * rng.standard_normal(Z0.size)).to(dev) for k in range(3)]
        dmu = [torch.from_numpy(rng.standard_normal(ev.n_constraints)).to(dev) for _ in range(3)]

        def call(e, k, which, o):
            if which == "jac":
                e.eval_jacobian_dev(dZ[k].data_ptr(), o.data_ptr(), st)
            else:
                e.eval_hessian_dev(dZ[k].data_ptr(), 0.7, dmu[k].data_ptr(), o.data_ptr(), st)
            torch.cuda.synchronize()

        # constants of the plan: row 16 of column 0 of knot 1 (outside that column's own 16 x 16 block of the structured
        # integrator); Hessian entry (U_0, U_0) of knot 1 (no term has a second derivative there: the form is listed at knot N)
        for which, vec, pos in (("jac", capi.VECTOR_JACOBIAN, 16), ("hess", capi.VECTOR_HESSIAN, 0)):
            n = ref.shard.jac_len if which == "jac" else ref.shard.hess_len
            want = []
            for k in range(3):
                o = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
                call(ref, k, which, o)
                want.append(o)
            buf = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
            ev.bind_output_dev(vec, buf.data_ptr())
            for k in (0, 1, 2, 0):
                call(ev, k, which, buf)
                assert torch.equal(buf, want[k]), (which, k, int((buf != want[k]).sum()))
            assert all(w[pos] == 0.0 for w in want)
            buf[pos] = 7.0
            call(ev, 1, which, buf)
            assert buf[pos] == 7.0
            buf[pos] = 0.0
            assert torch.equal(buf, want[1])
            ev.bind_output_dev(vec, 0)
    finally:
        ev.close(); ref.close()


@pytest.mark.parametrize("levels,N", [(4, 6), (8, 5)])
def test_unitary_problem_objective_still_matches_the_oracle(levels, N):
    """The low-rank infidelity's gradient and Hessian now come from one thread per entry: f, grad f and H of unitary_problem
    against the oracle on a flagged and an unflagged handle."""
    pe = dto_amd.synthetic.unitary_problem(levels, 2, N, seed=5)
    prob_o = to_oracle(pe)
    ev_o = O.OracleEvaluator(prob_o)
    for flagged in (True, False):
        ev = dto_amd.Evaluator(pe, block_generators=flagged)
        try:
            check_against_oracle(ev, ev_o, prob_o, tag=f"unitary, {levels} levels, flagged={flagged}")
        finally:
            ev.close()
