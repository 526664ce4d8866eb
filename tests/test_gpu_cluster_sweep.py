"""GPU: the generator sweeps of 128- and 256-state integrators on short horizons, where the single-workgroup (fused) form cannot
fill the chip.  Two forms serve them, and every case asserts through the profile counters (dto_profile_get "sweep_gs" ..
"sweep_step") which one ran:

- one round of the Taylor series (q == 1): the generator-stationary form (csrc/dto_sweep_gs.hip, k_sweep_gs) for every sweep --
  eval_constraint, the Jacobian's tangent columns, the Hessian's forward column and adjoint sweep -- whole and sharded;
- sub-stepped sweeps (q > 1, larger time steps): the row-split cluster form (csrc/dto_sweep_fused.hip, k_sweep_cluster) for the
  multi-column sweeps.  R workgroups share an interval group, each computes npad / R rows of every Taylor term and the slices are
  exchanged through global memory with agent-scope 8-byte atomics.  eval_constraint's single column takes the step form there.

Checked against the oracle at the usual bars AND against the step-per-launch form of the same engine (option sweep_form = 1),
for 128- and 256-state integrators; repeated calls are bit-identical (the exchange protocol must not let a stale slice through:
every word of every callback is compared).  Every instance of both kernels, pinned one by one: tests/test_gpu_sweep_forms.py."""
import numpy as np
import pytest

import dto_oracle as O
from helpers import assert_sweep_form, rel_err, sweep_forms, to_engine

pytestmark = pytest.mark.gpu


def _callbacks(ev, Z, mu):
    """The three callbacks, and the forms their sweeps took."""
    forms = []
    ev.profile_reset()
    c = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(c, Z)
    forms.append(sweep_forms(ev)); ev.profile_reset()
    j = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(j, Z)
    forms.append(sweep_forms(ev)); ev.profile_reset()
    h = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(h, Z, 0.9, mu)
    forms.append(sweep_forms(ev))
    return (c, j, h), forms


def _compare(n, m, N, scale, substepped):
    import dto_amd
    p = O.make_scaled_problem(N, n, m, seed=100 + n, with_constraint=True)
    if scale != 1.0:   # larger steps: ||A|| grows, the sweep runs q > 1 rounds (the sums go through the exchange as well)
        Zk = p.Z0[:p.z * N].reshape(N, p.z)
        Zk[:, p.dt_idx] *= scale
    ev_o = O.OracleEvaluator(p)
    Z = p.Z0
    mu = np.random.default_rng(5).standard_normal(ev_o.n_constraints)
    want = (ev_o.eval_constraint(Z), ev_o.eval_constraint_jacobian(Z), ev_o.eval_hessian_lagrangian(Z, 0.9, mu))
    ev = dto_amd.Evaluator(to_engine(p))
    ev_step = dto_amd.Evaluator(to_engine(p))
    ev_step.set_option("sweep_form", 1)
    ev.profile_enable(True)
    ev_step.profile_enable(True)
    try:
        got, forms = _callbacks(ev, Z, mu)
        ref, ref_forms = _callbacks(ev_step, Z, mu)
        print(forms)
        for f in ref_forms:
            assert_sweep_form(f, "step", what="sweep_form = 1")
        if substepped:
            assert_sweep_form(forms[0], "step", what="eval_constraint")   # a single column: the cluster form refuses it
            assert_sweep_form(forms[1], "cluster", what="Jacobian")
            assert forms[2]["cluster"] >= 1 and forms[2]["gs"] == forms[2]["fused"] == forms[2]["s64"] == 0, forms[2]
        else:
            for f, what in zip(forms, ("eval_constraint", "Jacobian", "Hessian")):
                assert_sweep_form(f, "gs", what=what)
        for g, w, r, tol in zip(got, want, ref, (1e-10, 1e-10, 1e-8)):
            assert rel_err(g, w) <= tol and rel_err(g, r) <= tol
        for _ in range(3):   # no stale slice: every repetition reproduces every word
            again, _f = _callbacks(ev, Z, mu)
            for a, g in zip(again, got):
                assert np.array_equal(a, g)
    finally:
        ev.close(); ev_step.close()


@pytest.mark.parametrize("n,m,N", [(100, 3, 14), (200, 4, 12), (256, 2, 9)], ids=["128-states", "256-states", "256-exact"])
def test_short_horizons_take_the_gs_form(n, m, N):
    """q == 1: the fused planner refuses 13 or fewer intervals, every sweep runs generator-stationary (the Jacobian's with
    source terms)."""
    _compare(n, m, N, 1.0, substepped=False)


@pytest.mark.parametrize("n,m,N,scale", [(120, 2, 10, 6.0), (200, 3, 10, 6.0), (256, 2, 8, 6.0)],
                         ids=["sub-stepped", "256-sub-stepped", "256-exact-sub-stepped"])
def test_cluster_sweep_matches_the_oracle_and_the_step_form(n, m, N, scale):
    """q > 1 on a short horizon: the planner's own cluster shape (128 states: R = 2; 256 states: R = 2 or 4)."""
    _compare(n, m, N, scale, substepped=True)


def test_gs_sweep_on_shards():
    """Three shards of a 128-state problem (first intervals 1, 7, 14): each shard's Jacobian sweep is generator-stationary with
    source terms; the slabs side by side are the whole Jacobian."""
    import dto_amd
    p = O.make_scaled_problem(20, 128, 2, seed=77)
    ev_o = O.OracleEvaluator(p)
    Z = p.Z0
    want = ev_o.eval_constraint_jacobian(Z)
    got = np.full_like(want, np.nan)
    for lo, hi in dto_amd.distributed.shard_ranges(p.N, 3):
        e = dto_amd.Evaluator(to_engine(p), k_lo=lo, k_hi=hi)
        e.profile_enable(True)
        e.profile_reset()
        o = np.empty(e.shard.jac_len); e.eval_constraint_jacobian(o, Z)
        assert_sweep_form(sweep_forms(e), "gs", what=(lo, hi))
        got[e.shard.jac_lo:e.shard.jac_lo + e.shard.jac_len] = o
        e.close()
    assert rel_err(got, want) <= 1e-10
