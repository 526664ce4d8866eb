"""GPU: the form every generator sweep takes, and every instance of the two forms that hand data between workgroups.

`run_sweep` (csrc/dto_engine.cpp) runs a sweep in the form `choose_sweep` (csrc/dto_sweep_plan.h) picked, one of five, and counts it (dto_profile_get "sweep_gs",
"sweep_fused", "sweep_s64", "sweep_cluster", "sweep_step"): generator-stationary (k_sweep_gs, csrc/dto_sweep_gs.hip), fused
(k_sweep_fused), the 64-state fused form (k_sweep_s64), row-split cluster (k_sweep_cluster) and one launch per Taylor step
(k_sweep).  Every case below asserts, per callback, the form through those counters (the other forms 0), compares eval_constraint,
the Jacobian, the Hessian and, on whole handles, J'w with the oracle (1e-10 max(1,|ref|), Hessian 1e-8, sparsity bit-exact) and
with a handle of the same library forced onto the step form (sweep_form = 1: 1e-11, Hessian 1e-9), and repeats every callback
three times: every word must come back, from a sweep of its own each time.

The product library picks NT by its cost model -- NT = 1 for the short sweeps here, NT = 2 for long single-column sweeps.  The
other NT and every cluster shape are pinned in child processes on the TUNING library (libdto_engine_t.so), whose A/B switches are
read once per process: DTO_GS_NT, DTO_SWEEP_GS = 0 (the q == 1 multi-column sweeps of short horizons move to the cluster form),
DTO_CLUSTER_R, DTO_CLUSTER_NT.

k_sweep_gs<KU, MP, NT, HAS_SRC>: KU = npad / 32 cluster members, MP = 3 generator slots for m <= 2 drives, else 5; HAS_SRC = false
for single-column sweeps (eval_constraint, the Hessian's forward column, J'w's adjoint column), true for tangent columns (Jacobian,
the Hessian's adjoint sweep, J'w's forward sweep).  Every gs case runs both HAS_SRC values.

    instance        NT = 1 (product library)                           NT = 2 (child, DTO_GS_NT=2)
    <4, 3, *, F/T>  test_gs_instances[n65-m1], [n128-m2]              test_gs_instances_two_tiles
    <4, 5, *, F/T>  test_gs_instances[n100-m3], [n128-m4]             test_gs_instances_two_tiles
    <8, 3, *, F/T>  test_gs_instances[n200-m2], [n256-m1]             test_gs_instances_two_tiles
    <8, 5, *, F/T>  test_gs_instances[n193-m4], [n256-m3]             test_gs_instances_two_tiles,
                                                                      test_gs_coefficient_table_at_the_lds_limit (F, own pick)

Edges: one interval (one group, 7 of the 8 clusters idle), ragged last groups and sharded handles with k_lo > 1
(test_gs_edge_shapes); more groups than clusters (test_gs_rounds_and_ragged_groups, <8, 3, 1, F>); the coefficient table of a long
eval_constraint a few hundred bytes under the 160 KB LDS budget of sweep_gs_plan (test_gs_coefficient_table_at_the_lds_limit).
n = 65 and n = 193 leave whole cluster members holding only padding rows (n = 129 pads to 192 states, which no one-launch form
takes: test_gs_edge_shapes[n129-step]).

k_sweep_cluster<MT, NT, R> (npad = 64 MT R), in children with DTO_SWEEP_GS=0 and the shape pinned:

    112, 122        128 states      test_cluster_instances[R2-NT1], [R2-NT2]
    212, 222        256 states      test_cluster_instances[R2-NT1], [R2-NT2]
    114, 124        256 states      test_cluster_instances[R4-NT1], [R4-NT2]

The planner's own picks (q > 1) are in tests/test_gpu_cluster_sweep.py.  These six are every instance there is
(DTO_SWEEP_CLUSTER_INSTANCES, csrc/dto_sweep_plan.h; tests/test_sweep_plan_header.py holds the list against the planner)."""
import atexit
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dto_oracle as O
from helpers import SWEEP_FORMS, assert_sweep_form, rel_err, sub_problem, sweep_forms, to_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.9
CALLS = ("g", "J", "H", "JTw")


def _only(form):
    return form, tuple(f for f in SWEEP_FORMS if f != form)


# per callback: (the form that must have run, the forms that must not have)
GS = {c: _only("gs") for c in CALLS}
STEP = {c: _only("step") for c in CALLS}
# multi-column sweeps on the cluster form; single columns (eval_constraint, the Hessian's forward p column on the pairing path,
# J'w's adjoint column) are refused by it and take the step form
CLUSTER = {"g": _only("step"), "J": _only("cluster"), "H": ("cluster", ("gs", "fused", "s64")),
           "JTw": ("cluster", ("gs", "fused", "s64"))}
EXPECT = {"gs": GS, "step": STEP, "cluster": CLUSTER}

# oracle results by shape, shared with the child processes through files (the (u, u) terms at 256 states are the slow part)
_REFS = {}
_REF_DIR = []


def _ref_dir():
    if not _REF_DIR:
        d = os.environ.get("DTO_SWEEP_FORMS_REFS")
        if not d:
            d = tempfile.mkdtemp(prefix="dto_sweep_forms_")
            atexit.register(shutil.rmtree, d, True)
        _REF_DIR.append(d)
    return _REF_DIR[0]


def _reference(ev_o, key, Z, mu, w):
    if key not in _REFS:
        path = os.path.join(_ref_dir(), key + ".npz")
        if os.path.exists(path):
            with np.load(path) as f:
                _REFS[key] = {k: f[k] for k in f.files}
        else:
            _REFS[key] = {"g": ev_o.eval_constraint(Z), "J": ev_o.eval_constraint_jacobian(Z),
                          "H": ev_o.eval_hessian_lagrangian(Z, SIGMA, mu), "JTw": ev_o.eval_constraint_jacobian_transpose_product(Z, w)}
            np.savez(path, **_REFS[key])
    return _REFS[key]


def _call(ev, what, Z, mu, w):
    s = ev.shard
    if what == "g":
        out = np.full(s.cons_len, np.nan); ev.eval_constraint(out, Z)
    elif what == "J":
        out = np.full(s.jac_len, np.nan); ev.eval_constraint_jacobian(out, Z)
    elif what == "H":
        out = np.full(s.hess_len, np.nan); ev.eval_hessian_lagrangian(out, Z, SIGMA, mu)
    else:
        out = np.full(ev.n_variables, np.nan); ev.eval_constraint_jacobian_transpose_product(out, Z, w)
    return out


def _place(ev, what, out, whole):
    """A shard's output at its place in the whole vector."""
    s = ev.shard
    if what == "J":
        whole[s.jac_lo:s.jac_lo + s.jac_len] = out
    elif what == "H":
        whole[s.hess_lo:s.hess_lo + s.hess_len] = out
    elif what == "g":
        pos = 0
        for a, b in zip(*ev.shard_rows()):
            whole[a - 1:a - 1 + b] = out[pos:pos + b]
            pos += b
    else:
        whole[:] = out


def run_case(n, m, N, expect, scale=1.0, shards=None):
    """Callbacks of fresh handles of the loaded library on make_scaled_problem(N, n, m): the form each sweep took, three
    repetitions bit-identical, the oracle, and a sweep_form = 1 handle of the same library."""
    import dto_amd
    p = O.make_scaled_problem(N, n, m, seed=1000 + 10 * n + m, with_constraint=True)
    if scale != 1.0:   # larger steps: the sweeps need q > 1 rounds
        p.Z0[p.dt_idx:p.z * N:p.z] *= scale
    Z = p.Z0
    expect = EXPECT[expect]
    calls = CALLS if shards is None else ("g", "J", "H")   # (the products need a whole handle)
    ev_o = O.OracleEvaluator(p)
    rng = np.random.default_rng(n + m)
    mu = rng.standard_normal(ev_o.n_constraints)
    w = rng.standard_normal(ev_o.n_constraints)
    ref = _reference(ev_o, f"{n}-{m}-{N}-{scale}", Z, mu, w)
    got = {c: np.full_like(ref[c], np.nan) for c in calls}
    step = {c: np.full_like(ref[c], np.nan) for c in calls}
    ranges = [(0, 0)] if shards is None else list(dto_amd.distributed.shard_ranges(N, shards))
    tag = (n, m, N, scale, shards)
    for lo, hi in ranges:
        ev = dto_amd.Evaluator(to_engine(p), k_lo=lo, k_hi=hi)
        ev_s = dto_amd.Evaluator(to_engine(p), k_lo=lo, k_hi=hi)
        try:
            if shards is None:
                r, c = ev.jacobian_structure(); r1, c1 = ev_o.jacobian_structure1()
                assert np.array_equal(r, r1) and np.array_equal(c, c1), "Jacobian structure"
                r, c = ev.hessian_lagrangian_structure(); r1, c1 = ev_o.hessian_structure1()
                assert np.array_equal(r, r1) and np.array_equal(c, c1), "Hessian structure"
            ev_s.set_option("sweep_form", 1)
            ev.profile_enable(True)
            ev_s.profile_enable(True)
            for c in calls:
                ev.profile_reset()
                out = _call(ev, c, Z, mu, w)
                counts = sweep_forms(ev)
                form, zero = expect[c]
                assert_sweep_form(counts, form, zero, (tag, c, lo, hi))
                ev.profile_reset()
                for _ in range(3):   # no stale slice, norm slot or coefficient row: every word again, from a sweep of its own
                    assert np.array_equal(_call(ev, c, Z, mu, w), out), (tag, c, lo, hi, "repeat")
                assert sweep_forms(ev) == {f: 3 * v for f, v in counts.items()}, (tag, c, counts, sweep_forms(ev))
                ev_s.profile_reset()
                o_s = _call(ev_s, c, Z, mu, w)
                assert_sweep_form(sweep_forms(ev_s), "step", what=(tag, c, "sweep_form = 1"))
                _place(ev, c, out, got[c])
                _place(ev_s, c, o_s, step[c])
        finally:
            ev.close(); ev_s.close()
    for c in calls:
        tol_o, tol_s = (1e-8, 1e-9) if c == "H" else (1e-10, 1e-11)
        e_o, e_s = rel_err(got[c], ref[c]), rel_err(got[c], step[c])
        print(tag, c, "oracle", e_o, "step form", e_s)
        assert e_o <= tol_o and e_s <= tol_s, (tag, c, e_o, e_s)


# (n, m, N): npad = pad64(n) -> KU, m -> MP.  Every eval_constraint / Jacobian here leaves its last group part-filled or alone.
GS_CASES = [(65, 1, 9), (128, 2, 12), (100, 3, 10), (128, 4, 7), (200, 2, 11), (256, 1, 9), (193, 4, 5), (256, 3, 6)]
GS_IDS = [f"n{n}-m{m}" for n, m, _ in GS_CASES]


@pytest.mark.parametrize("n,m,N", GS_CASES, ids=GS_IDS)
def test_gs_instances(n, m, N):
    """Short horizons: every single-column sweep, and every tangent sweep the fused planner refuses, runs generator-stationary
    with one tile per group (the cost model's pick for a lone round)."""
    run_case(n, m, N, "gs")


@pytest.mark.parametrize("n,m,N,expect,shards", [
    (128, 2, 2, "gs", None),      # one interval: one group, 7 of the 8 clusters idle
    (256, 4, 2, "gs", None),
    (200, 2, 18, "gs", None),     # 17 intervals: eval_constraint 16 + 1, Jacobian (5 per group) 3 x 5 + 2
    (128, 2, 20, "gs", 3),        # three shards: first intervals 1, 7, 14 (k_lo > 1)
    (256, 1, 12, "gs", 2),
    (129, 2, 4, "step", None),    # npad 192: no one-launch form takes it
], ids=["n128-one-interval", "n256-one-interval", "ragged", "shards-128", "shards-256", "n129-step"])
def test_gs_edge_shapes(n, m, N, expect, shards):
    run_case(n, m, N, expect, shards=shards)


_CHILD = r"""
import json, os, sys
root = os.environ["DTO_ROOT"]
for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
    sys.path.insert(0, p)
import dto_amd
dto_amd.Evaluator.default_options = {"host_xfer_check": 1}   # as tests/conftest.py sets for the suite
import test_gpu_sweep_forms as T
for case in json.loads(sys.argv[1]):
    T.run_case(**case)
print("child-ok")
"""


def _in_child(env, cases, timeout=600):
    """run_case for each case in a fresh process on the TUNING library, with the switches in `env`."""
    env = dict(os.environ, DTO_ROOT=ROOT, DTO_ENGINE_LIB="libdto_engine_t.so", DTO_SWEEP_FORMS_REFS=_ref_dir(), **env)
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(cases)], env=env, capture_output=True, text=True,
                       timeout=timeout)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "child-ok" in r.stdout, (r.stdout + r.stderr)[-4000:]


def test_gs_instances_two_tiles():
    """The same shapes with two column tiles per group (DTO_GS_NT=2): the other eight instances."""
    _in_child({"DTO_GS_NT": "2"}, [dict(n=n, m=m, N=N, expect="gs") for n, m, N in GS_CASES])


@pytest.mark.parametrize("R,NT", [(2, 1), (2, 2), (4, 1), (4, 2)], ids=["R2-NT1", "R2-NT2", "R4-NT1", "R4-NT2"])
def test_cluster_instances(R, NT):
    """q == 1 short horizons with the generator-stationary form off: the Jacobian's and the Hessian's adjoint tangent sweeps
    (and J'w's forward sweep) on k_sweep_cluster<npad / (64 R), NT, R>.  R = 4 has no 128-state shape."""
    cases = [dict(n=200, m=2, N=11, expect="cluster"), dict(n=256, m=3, N=6, expect="cluster")]
    if R == 2:
        cases = [dict(n=128, m=2, N=12, expect="cluster"), dict(n=128, m=4, N=7, expect="cluster")] + cases
    _in_child({"DTO_SWEEP_GS": "0", "DTO_CLUSTER_R": str(R), "DTO_CLUSTER_NT": str(NT)}, cases)


# ---- long horizons

def _gs_lds_bytes(KU, MP, NT, cap):
    """gs_lds_bytes of dto_sweep_plan.h: the GsLds carve-up (doubles) and the coefficient table [(MP + 1)][cap]."""
    ncp, zs, max_types = 16 * NT, 32 * KU + 2, 36
    total = 2 * (ncp * zs + 8) + 2 * 3 * ncp + 5 * max_types + ncp + MP * ncp + (MP * ncp + 1) // 2 + 2
    return max((total + (MP + 1) * cap) * 8, 82 * 1024)


def _clusters(KU):
    """Clusters of a long sweep (sweep_gs_plan): as many as the chip holds with one workgroup per CU, a multiple of 8."""
    import torch
    return (torch.cuda.get_device_properties(0).multi_processor_count // KU) // 8 * 8


def _long_constraint(prob, ks, n, m):
    """eval_constraint of a long synthetic problem: the generator-stationary form alone, three repetitions bit-identical, the
    step form, and the defects of the sampled intervals against two-knot oracle problems."""
    import dto_amd
    Z = prob.trajectory.vec()
    ev = dto_amd.Evaluator(prob, eval_hessian=False)
    try:
        ev.profile_enable(True)
        ev.profile_reset()
        g = np.full(ev.n_constraints, np.nan); ev.eval_constraint(g, Z)
        assert_sweep_form(sweep_forms(ev), "gs")
        for _ in range(3):
            again = np.full_like(g, np.nan); ev.eval_constraint(again, Z)
            assert np.array_equal(again, g)
    finally:
        ev.close()
    ev = dto_amd.Evaluator(prob, eval_hessian=False)
    try:
        ev.set_option("sweep_form", 1)
        g_step = np.full_like(g, np.nan); ev.eval_constraint(g_step, Z)
    finally:
        ev.close()
    assert rel_err(g, g_step) <= 1e-11, rel_err(g, g_step)
    traj = prob.trajectory
    K, z, X = traj.N - 1, traj.dim, traj.data
    for k in ks:
        sub = sub_problem(prob.integrators[0].G, X[:, k:k + 2].T, n, m, z, traj.components[traj.timestep][0])
        ref = O.OracleEvaluator(sub).eval_constraint(sub.Z0)
        assert rel_err(g[k * n:(k + 1) * n], ref[:n]) <= 1e-10, ("bilinear defect", k)
        assert rel_err(g[K * n + k * m:K * n + (k + 1) * m], ref[n:]) <= 1e-10, ("derivative defect", k)
    return g


def test_gs_rounds_and_ragged_groups():
    """256 states, 600 intervals: eval_constraint's 38 groups of 16 on 32 clusters take two rounds (the round-robin software
    pipeline; the coefficient rows of a second round in LDS), its last group holds 8 intervals; the Hessian's forward column
    likewise.  Sampled Jacobian column blocks, Hessian diagonal blocks and defects against the oracle, whole vectors against the
    step form."""
    import dto_amd
    from helpers import host_getter, sampled_checks
    n, m, N = 256, 2, 601
    assert _clusters(8) == 32, "the group / round layout below is that of a 256-CU part"
    prob = dto_amd.host.synthetic.make_scaled_problem(N, n, m, seed=61)
    # group j = intervals 16 j .. 16 j + 15 on cluster j % 32: round boundary 511 | 512, last group 592..599 on cluster 5
    ks = (0, 15, 16, 511, 512, 591, 592, 599, 600)
    g = _long_constraint(prob, ks[:-1], n, m)
    Z = prob.trajectory.vec()
    mu = np.random.default_rng(3).standard_normal(g.size)
    out = {}
    for form in (0, 1):
        ev = dto_amd.Evaluator(prob)
        try:
            ev.set_option("sweep_form", form)
            ev.profile_enable(True)
            ev.profile_reset()
            h = np.full(ev.n_hessian_entries, np.nan); ev.eval_hessian_lagrangian(h, Z, SIGMA, mu)
            counts = sweep_forms(ev)
            if form == 0:
                assert counts["gs"] >= 1 and counts["cluster"] == counts["s64"] == 0, counts
            else:
                assert_sweep_form(counts, "step")
            j = np.full(ev.n_jacobian_entries, np.nan); ev.eval_constraint_jacobian(j, Z)
            out[form] = (j, h)
        finally:
            ev.close()
    assert rel_err(out[0][0], out[1][0]) <= 1e-11 and rel_err(out[0][1], out[1][1]) <= 1e-9
    j, h = out[0]
    sampled_checks(prob, None, n, m, ks, host_getter(j), host_getter(h), g, mu, SIGMA)


def test_gs_coefficient_table_at_the_lds_limit():
    """The longest eval_constraint whose two-tile plan still fits: 256 states, 4 drives (MP = 5), NT = 2 (32 intervals per group,
    the cost model's pick at this length) -- the coefficient table [(MP + 1)][rounds x 32] then leaves a few hundred bytes of the
    160 KB; one round more and the plan falls back to one tile.  Sampled at the first and last intervals, group and round
    boundaries and the last group of the last cluster."""
    import dto_amd
    n, m = 256, 4
    rounds = max(r for r in range(1, 65) if _gs_lds_bytes(8, 5, 2, 32 * r) <= 160 * 1024)
    assert 160 * 1024 - _gs_lds_bytes(8, 5, 2, 32 * rounds) < 1024, rounds
    per_round = _clusters(8) * 32
    K = rounds * per_round
    prob = dto_amd.host.synthetic.make_scaled_problem(K + 1, n, m, seed=17)
    last = (rounds - 1) * per_round
    ks = (0, 1, 31, 32, per_round - 1, per_round, last - 1, last, K - 33, K - 32, K - 1)
    _long_constraint(prob, ks, n, m)
