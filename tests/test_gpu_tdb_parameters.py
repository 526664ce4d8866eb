"""GPU: the device TimeDependentBilinearIntegrator over the parameters its kernels branch on and the other time-dependent tests keep
fixed -- 0..7 drives (p = 2 .. 16 parameters per interval, up to 136 second-derivative pairs), coefficient tables up to the
6144-entry cap, modulation lists that begin with a sin, repeat a kind and carry omega = 0 and a negative omega, and knot layouts with
the controls below the state, the timestep before the time, fillers in between, and the time variable naming the timestep (two
parameters on one entry).  k_tdb (1..64 states, csrc/dto_tdb.hip), k_tdb_mfma (65..256, csrc/dto_tdb_mfma.hip), k_tdb_kron (replicated
blocks, csrc/dto_tdb_kron.hip), and the matrix-free J w / J' w modes of the first two.

Reference: tests/tdb_large_cases.reference on the problems of tests/tdb_layout_cases.py; tests/test_tdb_layout_reference.py pins it to
`O.OracleEvaluator` on these layouts and at 7 drives.  Bars: helpers.TOL (1e-10 max(1, |ref|)) for values, Jacobian and products,
helpers.TOL_H (1e-8) for the Hessian; structure indices bit-equal; outputs filled with NaN beforehand.  N = 3 throughout (two
intervals: a persistent workgroup reuses its scratch slot once).  Case ids read kernel-drives-order-terms-layout.

Pair tables: TDBM_MAX_PAIRS = TDBK_MAX_PAIRS = 160 admit the 136 pairs of 7 drives at order 1
(tests/test_tdb_layout_reference.py reads them from the sources), so no kernel has a pair cap of its own below p = 16 and the
full-table cases below are the boundary."""
import functools

import numpy as np
import pytest

import dto_amd
import tdb_large_cases as L
import tdb_layout_cases as C
from helpers import TOL, TOL_H, rel_err, to_engine
from test_gpu_jacobian_products import host_products
from test_gpu_tdb_products import OPTION, _dense, _evaluator, check_built

pytestmark = pytest.mark.gpu

FULL = C.MIXED                  # 7 drives, order 1, the four mixed terms: (1 + 16 + 136) * 8 * 5 = 6120 entries
NEAR = C.mods_of_length(12)     # 7 drives, order 0: (1 + 9 + 45) * 8 * 13 = 5720 entries
TWO = C.MIXED[:2]               # sin omega_fast, sin 0.6


def D(n, m, order, substeps, mods, layout="default"):
    return ("dense", n, n, 1, m, order, substeps, tuple(mods), layout)


def K(b, r, m, order, substeps, mods, layout="default"):
    return ("kron", b * r, b, r, m, order, substeps, tuple(mods), layout)


def ident(spec):
    kind, n, b, r, m, order, substeps, mods, layout = spec
    kernel = "kron%dx%d" % (b, r) if kind == "kron" else ("tdb%d" % n if n <= 64 else "mfma%d" % n)
    terms = {NEAR: "near12", C.MIXED: "mixed4", TWO: "sin2", C.PLAIN: "plain2", (): "none"}[mods]
    p = m + 2 + (m if order else 0)
    return "%s-m%d-o%d-p%d-%s-table%d-%s" % (kernel, m, order, p, terms, (1 + p + p * (p + 1) // 2) * (m + 1) * (1 + len(mods)), layout)


@functools.lru_cache(maxsize=None)
def case(spec):
    """Problem, engine problem and the reference's values (tdb_large_cases.reference: shared, read-only)."""
    kind, n, b, r, m, order, substeps, mods, layout = spec
    if kind == "kron":
        po = C.kron_layout_problem(b, r, m, order, substeps, mods, layout)
    else:
        po = C.layout_problem(n, m, order, substeps, mods, layout)
    return po, to_engine(po), L.reference(po, ("parameters",) + spec)


def values(ev, Z, mu, sigma=0.6):
    g = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(g, Z)
    j = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(j, Z)
    h = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(h, Z, sigma, mu)
    return g, j, h


def check_values(spec, blocks=None, ran=None, idle=None, **kw):
    """Structure bit-equal, the three value callbacks at the bars; `blocks`: what integrator_blocks(0) reports; `ran` / `idle`: the
    profile names of the kernel that served each call and of the one that must not have run."""
    po, pe, (ev_r, mu, g_r, j_r, h_r) = case(spec)
    ev = dto_amd.Evaluator(pe, **kw)
    try:
        if blocks is not None:
            assert ev.integrator_blocks(0) == blocks
        for mine, ref in ((ev.jacobian_structure(), ev_r.jacobian_structure1()), (ev.hessian_lagrangian_structure(), ev_r.hessian_structure1())):
            assert np.array_equal(mine[0], ref[0]) and np.array_equal(mine[1], ref[1])
        if ran:
            ev.profile_enable(True); ev.profile_reset()
        g, j, h = values(ev, po.Z0, mu)
        if ran:
            assert ev.profile_get(ran)[1] >= 3 and ev.profile_get(idle)[1] == 0, (ev.profile_get(ran), ev.profile_get(idle))
        errs = (rel_err(g, g_r), rel_err(j, j_r), rel_err(h, h_r))
        print(ident(spec), kw, errs)
        assert errs[0] <= TOL and errs[1] <= TOL and errs[2] <= TOL_H, errs   # (NaN, a missing writer, fails the comparison)
    finally:
        ev.close()


MANY_DRIVES = [D(5, 7, 1, 2, FULL), D(64, 7, 1, 2, FULL), D(65, 7, 1, 2, FULL), D(72, 7, 1, 2, FULL)]
NEAR_CAP = [D(12, 7, 0, 2, NEAR), D(72, 7, 0, 2, NEAR), D(24, 5, 1, 2, C.PLAIN), D(128, 5, 1, 2, C.PLAIN)]
NO_DRIVES = [D(1, 0, 0, 3, ()), D(1, 0, 1, 3, C.PLAIN), D(6, 0, 1, 3, ()), D(6, 0, 0, 3, C.PLAIN), D(72, 0, 0, 2, ()), D(72, 0, 1, 2, C.PLAIN)]
MIXED_LIST = [D(6, 2, 1, 4, C.MIXED), D(72, 1, 1, 2, C.MIXED)]
LAYOUT_CASES = [D(n, 2, 1, 2, TWO, lay) for n in (6, 72) for lay in C.LAYOUTS]


@pytest.mark.parametrize("spec", MANY_DRIVES, ids=ident)
def test_seven_drives_with_the_full_coefficient_table(spec):
    check_values(spec)


def test_seven_drives_with_the_full_coefficient_table_on_replicated_blocks():
    """136 pairs fit TDBK_MAX_PAIRS: the structured path keeps the handle."""
    check_values(K(12, 6, 7, 1, 2, FULL), blocks=(12, 6, 1), ran="tdb_kron", idle="tdb_mfma", block_generators=True)


@pytest.mark.parametrize("spec", NEAR_CAP, ids=ident)
def test_order_0_near_the_cap_and_five_drives(spec):
    check_values(spec)


@pytest.mark.parametrize("spec", NO_DRIVES, ids=ident)
def test_no_drives(spec):
    check_values(spec)


def test_no_drives_on_replicated_blocks():
    check_values(K(12, 6, 0, 1, 2, C.PLAIN), blocks=(12, 6, 1), ran="tdb_kron", idle="tdb_mfma", block_generators=True)


@pytest.mark.parametrize("spec", MIXED_LIST, ids=ident)
def test_mixed_modulation_list(spec):
    check_values(spec)


def test_mixed_modulation_list_on_replicated_blocks():
    check_values(K(12, 6, 1, 1, 2, C.MIXED), blocks=(12, 6, 1), ran="tdb_kron", idle="tdb_mfma", block_generators=True)


@pytest.mark.parametrize("spec", LAYOUT_CASES, ids=ident)
def test_layouts(spec):
    check_values(spec)


@pytest.mark.parametrize("layout", ["default", "u_first", "dt_before_t", "gap"])
def test_layouts_that_keep_the_structured_path(layout):
    check_values(K(12, 6, 2, 1, 2, TWO, layout), blocks=(12, 6, 1), ran="tdb_kron", idle="tdb_mfma", block_generators=True)


def test_aliased_time_falls_back_to_the_dense_path_on_a_flagged_handle():
    """t_off == dt_idx: the structured kernel assigns its entries, two of which would share a position; build_tdb keeps the blocks it
    found in the report and routes the integrator to k_tdb_mfma."""
    check_values(K(12, 6, 2, 1, 2, TWO, "t_is_dt"), blocks=(12, 6, 0), ran="tdb_mfma", idle="tdb_kron", block_generators=True)


@pytest.mark.parametrize("n", [4, 72])
def test_an_overflowing_table_is_refused_and_a_valid_handle_still_evaluates(n):
    """7 drives, order 1, five terms: 153 * 8 * 6 = 7344 entries."""
    po = C.layout_problem(n, 7, 1, 2, C.mods_of_length(5), "default")
    with pytest.raises(dto_amd.EngineError, match="coefficient table"):
        dto_amd.Evaluator(to_engine(po)).close()
    check_values(D(6, 2, 1, 2, TWO) if n == 4 else D(72, 2, 1, 2, TWO))


def test_eight_drives_are_refused():
    po = C.layout_problem(4, 8, 0, 2, (), "default")
    with pytest.raises(dto_amd.EngineError, match="0..7 drives"):
        dto_amd.Evaluator(to_engine(po)).close()


# ---- matrix-free J w / J' w (option tdb_matrix_free_products = 1) on the same cases

PRODUCTS = [D(5, 7, 1, 2, FULL), D(64, 7, 1, 2, FULL), D(72, 7, 1, 2, FULL), D(6, 0, 0, 3, C.PLAIN)] + LAYOUT_CASES


@functools.lru_cache(maxsize=None)
def product_case(spec):
    """The keys of test_gpu_tdb_products.case: expected J w / J' w contracted from the reference's Jacobian values."""
    po, pe, (ev_r, _, _, j_r, _) = case(spec)
    rng = np.random.default_rng(31)
    w, wt = rng.standard_normal(po.n_vars), rng.standard_normal(ev_r.n_constraints)
    r, c = ev_r.jacobian_structure1()
    ref = _dense(np.asarray(r), np.asarray(c), j_r, w, wt, ev_r.n_constraints, po.n_vars)
    Z = po.Z0.copy()
    for a in (Z, w, wt) + tuple(ref):
        a.setflags(write=False)
    return dict(p=po, pe=pe, Z=Z, w=w, wt=wt, Jw=ref[0], JTw=ref[1])


@pytest.mark.parametrize("spec", PRODUCTS, ids=ident)
def test_products(spec):
    check_built(product_case(spec), ident(spec))


@pytest.mark.parametrize("spec", [D(5, 7, 1, 2, FULL), D(72, 7, 1, 2, FULL), D(6, 2, 1, 2, TWO, "t_is_dt"), D(72, 2, 1, 2, TWO, "t_is_dt")], ids=ident)
def test_slab_route_agrees(spec):
    c = product_case(spec)
    out = []
    for option in (0, 1):
        ev = _evaluator(c["pe"], option)
        try:
            out.append(host_products(ev, c["Z"], c["w"], c["wt"]))
        finally:
            ev.close()
    errs = (rel_err(out[0][0], c["Jw"]), rel_err(out[0][1], c["JTw"]), rel_err(out[1][0], out[0][0]), rel_err(out[1][1], out[0][1]))
    print(ident(spec), "slab route vs reference, matrix-free vs slab route", errs)
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("n", [6, 72])
def test_transpose_product_sums_both_terms_at_the_aliased_entry(n):
    """t_is_dt: entry dt_k of J' w is -(w_k' dPhi/dt_k x_k) - (w_k' dPhi/d(dt_k) x_k), the two parameters kept apart
    (FastTdb._flows differentiates theta = [u_k, t_k, dt_k, u_{k+1}] entry by entry); nothing else lands there.  Each term alone is
    far above the bar, so a placement that kept one of them fails here whatever the other entries do."""
    spec = D(n, 2, 1, 2, TWO, "t_is_dt")
    c = product_case(spec)
    po = c["p"]
    it = L.fast_problem(po).integrators[0]
    z, m = po.z, it.u_dim
    want, parts = [], []
    for k in range(po.N - 1):
        zz = po.Z0[k * z:(k + 2) * z]
        idx, th, Phi, dPhi = it._flows(zz)
        assert idx[m] == idx[m + 1] == po.dt_idx
        x, wk = zz[it.x_off:it.x_off + n], c["wt"][k * n:(k + 1) * n]
        parts.append((-(wk @ dPhi[m] @ x), -(wk @ dPhi[m + 1] @ x)))
        want.append(parts[-1][0] + parts[-1][1])
    assert min(abs(v) for pr in parts for v in pr) > 1e3 * TOL, parts
    ev = _evaluator(c["pe"])
    try:
        _, t = host_products(ev, c["Z"], c["w"], c["wt"])
    finally:
        ev.close()
    got = [t[k * z + po.dt_idx] for k in range(po.N - 1)]
    print(ident(spec), "aliased entry", got, want, parts)
    assert rel_err(got, want) <= TOL
    assert t[(po.N - 1) * z + po.dt_idx] == 0.0   # the last knot's timestep enters no interval
