"""GPU: J w and J' w on the structured (csrc/dto_kron.hip) and small (csrc/dto_small.hip) paths without a value slab, and the
device-pointer entry points dto_eval_jacobian_product_dev / dto_eval_jacobian_transpose_product_dev.  Expected values are the
oracle's eval_constraint_jacobian_product / eval_constraint_jacobian_transpose_product at helpers.TOL (1e-10 max(1, |ref|), the bar
for first-order quantities); outputs are filled with NaN beforehand so that a missing writer shows."""
import functools

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import TOL, rel_err, to_engine
from test_gpu_block_generators import kron_problem, to_oracle

pytestmark = pytest.mark.gpu

SLAB_ROUTE_ONLY = ("zero_fill", "bgemm", "chain64", "assembly", "share")


def _with_constraint(p, comps):
    p.constraints = [O.KnotConstraint("sqnorm", list(comps), 1.0, list(range(2, p.N + 1)), equality=False)]
    return p


def _small(n, big_step=False):
    m, N = (1, 2) if n == 2 else (3, 4)
    p = O.make_scaled_problem(N, n, m, seed=100 + n, skew=big_step)
    if big_step:  # ||A||_1 ~ 13 at the second knot: the sweeps sub-step (q = 2), k_small's exponential squares; 1e-4: a few terms
        Zk = p.Z0.reshape(N, p.z)
        Zk[1, p.dt_idx] = 6.0
        Zk[2, p.dt_idx] = 1e-4
        p.Z0 = Zk.reshape(-1).copy()
    return p


# name -> (oracle problem, engine problem, Evaluator keywords)
def _build(name):
    kind, _, arg = name.partition(":")
    if kind == "kron":
        b, r, m, N = (int(v) for v in arg.split("x"))
        p = kron_problem(b, r, m, N, seed=b + r)
        return p, to_engine(p), dict(block_generators=True)
    if kind == "unitary":
        pe = dto_amd.synthetic.unitary_problem(levels=8, drives=2, N=6, dt_large=3.0, dt_small=1e-4)
        return to_oracle(pe), pe, dict(block_generators=True)
    if kind == "small":
        p = _small(int(arg))
        return p, to_engine(p), {}
    if kind == "small_big_step":
        p = _small(9, big_step=True)
        return p, to_engine(p), {}
    if kind == "mixed":  # structured + dense (40: general path, 8: small path) + DerivativeIntegrator + ||u||^2 - 1 <= 0
        p = _with_constraint(kron_problem(16, 4, 2, 4, seed=9, extra_dense=int(arg)), range(64, 66))
        return p, to_engine(p), dict(block_generators=True)
    if kind == "flag_clear":
        p = kron_problem(16, 4, 2, 3, seed=20)
        return p, to_engine(p), {}
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """The problem, a point, the two vectors and the oracle's products: computed once, shared by every test, never written."""
    p, pe, kw = _build(name)
    ev_o = O.OracleEvaluator(p)
    rng = np.random.default_rng(31)
    Z = p.Z0.copy()
    w, wt = rng.standard_normal(p.n_vars), rng.standard_normal(ev_o.n_constraints)
    ref = (ev_o.eval_constraint_jacobian_product(Z, w), ev_o.eval_constraint_jacobian_transpose_product(Z, wt))
    for a in (Z, w, wt) + ref:
        a.setflags(write=False)
    return dict(p=p, pe=pe, kw=kw, Z=Z, w=w, wt=wt, Jw=ref[0], JTw=ref[1])


def host_products(ev, Z, w, wt):
    y = np.full(ev.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, Z, w)
    t = np.full(ev.n_variables, np.nan); ev.eval_constraint_jacobian_transpose_product(t, Z, wt)
    return y, t


def dev_products(ev, Z, w, wt):
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    dZ, dw, dwt = (torch.from_numpy(np.array(a)).to(dev) for a in (Z, w, wt))
    y = torch.full((ev.n_constraints,), float("nan"), dtype=torch.float64, device=dev)
    t = torch.full((ev.n_variables,), float("nan"), dtype=torch.float64, device=dev)
    ev.eval_jacobian_product_dev(dZ.data_ptr(), dw.data_ptr(), y.data_ptr(), st)
    ev.eval_jacobian_transpose_product_dev(dZ.data_ptr(), dwt.data_ptr(), t.data_ptr(), st)
    torch.cuda.synchronize()
    return y.cpu().numpy(), t.cpu().numpy()


def check_case(name, **extra):
    c = case(name)
    ev = dto_amd.Evaluator(c["pe"], **dict(c["kw"], **extra))
    try:
        yh, th = host_products(ev, c["Z"], c["w"], c["wt"])
        yd, td = dev_products(ev, c["Z"], c["w"], c["wt"])
        errs = {"Jw": rel_err(yh, c["Jw"]), "JTw": rel_err(th, c["JTw"]), "Jw_dev": rel_err(yd, c["Jw"]), "JTw_dev": rel_err(td, c["JTw"])}
        print(name, extra, errs, ev.last_stats())
        for k, v in errs.items():
            assert v <= TOL, (name, k, v)   # (NaN, a missing writer, fails the comparison)
        assert np.array_equal(yh, yd) and np.array_equal(th, td), name
    finally:
        ev.close()


# b x r x m x N: baseline; b no multiple of 16; MT = 2, one drive, first and last knot neighbours; MT = 4, LDS at its largest;
# blocks grouped below 16 rows; two column tiles per group with a ragged second tile
STRUCTURED = ["kron:16x4x2x3", "kron:12x6x3x3", "kron:20x5x1x2", "kron:64x3x4x3", "kron:4x16x2x3", "kron:16x18x2x3", "unitary"]
SMALL = ["small:2", "small:4", "small:9", "small:32", "small_big_step"]


@pytest.mark.parametrize("name", STRUCTURED)
def test_structured_products_match_the_oracle(name):
    check_case(name)


@pytest.mark.parametrize("name", SMALL)
def test_small_products_match_the_oracle(name):
    check_case(name)


@pytest.mark.parametrize("name", ["mixed:40", "mixed:8"])
def test_mixed_handle_lands_every_kind_in_one_vector(name):
    c = case(name)
    assert len(c["p"].integrators) == 3 and len(c["p"].constraints) == 1
    check_case(name)


def _launches(ev, name):
    return ev.profile_get(name)[1]


@pytest.mark.parametrize("name", ["kron:16x4x2x3", "small:4"])
def test_structured_and_small_handles_form_no_slab(name):
    c = case(name)
    ev = dto_amd.Evaluator(c["pe"], **c["kw"])
    try:
        ev.profile_enable()
        ev.profile_reset()
        y, t = host_products(ev, c["Z"], c["w"], c["wt"])
        assert _launches(ev, "jac_product") >= 2   # one or more per product
        for other in SLAB_ROUTE_ONLY:
            assert _launches(ev, other) == 0, other
        assert rel_err(y, c["Jw"]) <= TOL and rel_err(t, c["JTw"]) <= TOL
    finally:
        ev.close()


def test_time_dependent_and_external_handles_keep_the_slab_route():
    for p in (O.make_tdb_problem(), O.make_closure_problem()):
        ev_o = O.OracleEvaluator(p)
        ev = dto_amd.Evaluator(to_engine(p))
        try:
            rng = np.random.default_rng(8)
            w, wt = rng.standard_normal(p.n_vars), rng.standard_normal(ev_o.n_constraints)
            ev.profile_enable()
            ev.profile_reset()
            y, t = host_products(ev, p.Z0, w, wt)
            assert _launches(ev, "zero_fill") >= 1
            assert _launches(ev, "jac_product") == 0
            assert rel_err(y, ev_o.eval_constraint_jacobian_product(p.Z0, w)) <= TOL
            assert rel_err(t, ev_o.eval_constraint_jacobian_transpose_product(p.Z0, wt)) <= TOL
        finally:
            ev.close()


@pytest.mark.parametrize("name", ["unitary", "small:9", "mixed:8"])
def test_products_repeat_bit_for_bit_and_leave_nothing_behind(name):
    c = case(name)
    ev = dto_amd.Evaluator(c["pe"], **c["kw"])
    try:
        Z, mu = c["Z"], c["wt"]
        Z2 = Z + 0.01 * np.random.default_rng(5).standard_normal(Z.size)

        def others(at):
            g = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(g, at)
            J = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(J, at)
            H = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(H, at, 0.7, mu)
            return g, J, H

        before = others(Z)
        runs = []
        for i in range(3):
            runs.append(host_products(ev, Z, c["w"], c["wt"]) + dev_products(ev, Z, c["w"], c["wt"]))
            others(Z if i == 0 else Z2)
        for r in runs[1:]:
            for a, b in zip(runs[0], r):
                assert np.array_equal(a, b)
        host_products(ev, Z, c["w"], c["wt"])
        for a, b in zip(before, others(Z)):
            assert np.array_equal(a, b)
    finally:
        ev.close()


@pytest.mark.parametrize("name", ["kron:16x4x2x3", "small:4"])
def test_jacobian_only_handle(name):
    check_case(name, eval_hessian=False)


def test_flag_clear_keeps_the_general_route():
    check_case("flag_clear")
