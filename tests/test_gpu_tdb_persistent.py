"""GPU: the persistent grid of the time-dependent kernels beyond its first trip, and the group launch at its limits (k_tdb_mfma, its
group and product forms in csrc/dto_tdb_mfma.hip, k_tdb_kron in csrc/dto_tdb_kron.hip; DESIGN sections 4.11 and 4.22).

Every launch starts `resident` = min(owned knots + 1, two per compute unit) workgroups; workgroup b walks intervals b, b + grid, ...
in one scratch slot.  Below 513 knots on 256 compute units no workgroup takes a second interval.  Two ways past that:

  * option "tdb_resident" caps the grid, so seven intervals are walked by 1, 2, 3 or 7 workgroups (parts a, f): small shapes with
    the reference of tests/tdb_large_cases.py beside them;
  * the default grid at 4 CUs + 7 knots (part b), where that reference needs minutes: a period-3 trajectory, whose values are
    copies of a five-knot problem's (tests/tdb_periodic_cases.py, pinned by tests/test_tdb_periodic_reference.py).

Bars against the reference (tdb_large_cases.reference, the oracle's evaluator with the integrator's blocks from step-matrix products
and complex steps): 1e-10 relative for g and the Jacobian, 1e-8 for the Hessian, the project's bars (helpers.TOL, TOL_H).  Everything
else is compared bit for bit: an interval's bits depend on its data alone.  Outputs are filled with NaN beforehand, so an entry
without a writer fails; the handles run with "host_xfer_check" on (conftest.py).

What part a would catch, from the kernels' code (k_tdb_mfma, for one integrator and for a group; k_tdb_kron has the same loop):
  * the loop body starts by writing all np * Ctot entries of Y -- x_k, the identity of the Phi block, zeros in the parameter
    columns and in the padding ("initial values: ...").  Without it an interval's second trip would start its RK4 steps from the
    Y the slot's previous interval ended with: x and Phi of interval it - grid instead of x_k and I, and padding columns that are no
    longer zero.  Every defect, Jacobian and Hessian entry of trips two and three would differ from the reference in its leading
    digits and from the run with grid 7, which has first trips only.
  * the barrier that ends the loop body ("the slot is reused by this workgroup's next interval") separates the output pass, which
    reads Y (defect: `zk1 - Y[r]`, the Jacobian's -Phi and parameter columns, the Hessian's `mu' x_ab` and the adjoint's W = TA),
    from the next trip's initial values written to the same addresses by other threads.  Without it a wavefront that has finished
    its share of the outputs overwrites Y while another still reads it; the entries read late come out as x_{k'} or 0 / 1 instead
    of the propagated values.  That is a race, so it need not show in every run; where it shows, it shows against both the reference
    and the grid-7 run.
  None of these variants is run here."""
import functools

import numpy as np
import pytest

import dto_oracle as O
import tdb_block_cases as B
import tdb_large_cases as L
import tdb_periodic_cases as PC
import tdb_share_cases as S
from helpers import TOL, TOL_H, rel_err, to_engine

pytestmark = pytest.mark.gpu

SIGMA = 0.6


def _all(ev, Z, mu, hessian=True):
    """g, Jacobian and Hessian values into buffers that hold NaN beforehand."""
    g = np.full(ev.shard.cons_len, np.nan); ev.eval_constraint(g, Z)
    j = np.full(ev.shard.jac_len, np.nan); ev.eval_constraint_jacobian(j, Z)
    if not hessian:
        return g, j
    h = np.full(ev.shard.hess_len, np.nan); ev.eval_hessian_lagrangian(h, Z, SIGMA, mu)
    return g, j, h


def _launches(ev, Z, mu, name="tdb_mfma", hessian=True):
    """Launches under profile name `name` of one eval_constraint, one Jacobian and (with `hessian`) one Hessian call."""
    calls = [lambda: ev.eval_constraint(np.empty(ev.shard.cons_len), Z), lambda: ev.eval_constraint_jacobian(np.empty(ev.shard.jac_len), Z)]
    if hessian:
        calls.append(lambda: ev.eval_hessian_lagrangian(np.empty(ev.shard.hess_len), Z, SIGMA, mu))
    out = []
    ev.profile_enable(True)
    for call in calls:
        ev.profile_reset()
        call()
        out.append(ev.profile_get(name)[1])
    ev.profile_enable(False)
    return out


def _same_structure(ev, ev_r):
    r, c = ev.jacobian_structure()
    assert np.array_equal(r, ev_r.jacobian_structure1()[0]) and np.array_equal(c, ev_r.jacobian_structure1()[1])
    r, c = ev.hessian_lagrangian_structure()
    assert np.array_equal(r, ev_r.hessian_structure1()[0]) and np.array_equal(c, ev_r.hessian_structure1()[1])


def _close_to(tag, got, ref):
    errs = tuple(rel_err(a, b) for a, b in zip(got, ref))
    print(tag, "vs reference (g, J, H)", errs)
    assert errs[0] <= TOL and errs[1] <= TOL and (len(errs) < 3 or errs[2] <= TOL_H), (tag, errs)   # (NaN fails the comparison)


def _same_bits(tag, got, want):
    diff = [int((a != b).sum()) if a.shape == b.shape else -1 for a, b in zip(got, want)]
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), (tag, "entries that differ (g, J, H)", diff)


def _check_grids(tag, ev, Z, mu, ref, first, others):
    """`first` workgroups against the reference, then the same handle at the grids `others` bit for bit."""
    ev.set_option("tdb_resident", first)
    got = _all(ev, Z, mu)
    _close_to("%s tdb_resident=%d" % (tag, first), got, ref)
    for v in others:
        ev.set_option("tdb_resident", v)
        _same_bits("%s tdb_resident=%d against %d" % (tag, v, first), _all(ev, Z, mu), got)


# ---- a. second and third trips at a reduced grid: N = 8, seven intervals, three workgroups (trips 3 / 2 / 2), then the default grid
# (one trip each), one workgroup (seven trips) and two (4 / 3)

# (n, m, order, substeps, n_mods, N, tdb_resident): 31 padded rows on the 32-row tile; ragged 64-row tiles at order 1; 200 states
# (224 padded, 32-row tile); the cap of 256 states at N = 6 (five intervals on two workgroups, trips 3 / 2: the reference takes
# about a second per interval there)
LONE = [(65, 1, 0, 2, 2, 8, 3), (72, 2, 1, 2, 2, 8, 3), (200, 1, 0, 2, 2, 8, 3), (256, 2, 1, 2, 2, 6, 2)]


@pytest.mark.parametrize("shape", LONE, ids=lambda s: "%dx%d" % (s[0], s[5]))
def test_a_lone_kernel_second_and_third_trips(shape):
    import dto_amd
    n, m, order, substeps, n_mods, N, first = shape
    po = S.lone(n, m, order, substeps, n_mods, N)
    ev_r, mu, g_r, j_r, h_r = S.reference(po, ("persistent-lone",) + shape)
    ev = dto_amd.Evaluator(to_engine(po))
    try:
        _same_structure(ev, ev_r)
        _check_grids("k_tdb_mfma %s" % (shape,), ev, po.Z0, mu, (g_r, j_r, h_r), first, [v for v in (0, 1, 2, 3) if v != first])
        assert _launches(ev, po.Z0, mu) == [1, 1, 1]
    finally:
        ev.close()


@pytest.mark.parametrize("case", S.CASES[:2], ids=lambda c: "%dx%d" % c[:2])
def test_a_group_kernel_second_and_third_trips(case):
    import dto_amd
    po = S.case(*case, N=8)
    ev_r, mu, g_r, j_r, h_r = S.reference(po, ("persistent-group",) + tuple(case))
    ev = dto_amd.Evaluator(to_engine(po), shared_generators=True)
    try:
        tdb = [i for i, it in enumerate(po.integrators) if isinstance(it, O.TimeDependentBilinearIntegrator)]
        assert [ev.integrator_share(i) for i in tdb] == [(tdb[0], case[1], 1)] * case[1]
        _same_structure(ev, ev_r)
        _check_grids("k_tdb_mfma, group %s" % (case,), ev, po.Z0, mu, (g_r, j_r, h_r), 3, (0, 1, 2))
        ev.set_option("tdb_resident", 3)
        assert _launches(ev, po.Z0, mu) == [1, 1, 1]
    finally:
        ev.close()


def test_a_structured_kernel_second_and_third_trips():
    import dto_amd
    po = B.kron_tdb_problem(12, 6, 2, 1, 2, 2, N=8)
    ev_r, mu, g_r, j_r, h_r = L.reference(po, ("persistent-kron", 12, 6))
    ev = dto_amd.Evaluator(to_engine(po), block_generators=True)
    try:
        assert ev.integrator_blocks(0) == (12, 6, 1)
        _same_structure(ev, ev_r)
        _check_grids("k_tdb_kron 12 x 6", ev, po.Z0, mu, (g_r, j_r, h_r), 3, (0, 1, 2))
        ev.set_option("tdb_resident", 3)
        assert _launches(ev, po.Z0, mu, name="tdb_kron") == [1, 1, 1] and _launches(ev, po.Z0, mu) == [0, 0, 0]
    finally:
        ev.close()


@pytest.mark.parametrize("flagged", [False, True], ids=["unflagged", "shared_generators"])
def test_a_matrix_free_products_second_and_third_trips(flagged):
    """J w and J' w (option "tdb_matrix_free_products" = 1: one launch per member and product, flagged or not) against the dense
    products of the reference Jacobian, three workgroups on seven intervals; the default grid gives the same bits."""
    import dto_amd
    case = S.CASES[1]   # 72 states, three kets, a DerivativeIntegrator between them
    po = S.case(*case, N=8)
    ev_r, _, _, j_r, _ = S.reference(po, ("persistent-group",) + tuple(case))
    rng = np.random.default_rng(31)
    w, wt = rng.standard_normal(po.n_vars), rng.standard_normal(ev_r.n_constraints)
    r, c = (np.asarray(a) - 1 for a in ev_r.jacobian_structure1())
    y_ref = np.zeros(ev_r.n_constraints); np.add.at(y_ref, r, j_r * w[c])
    t_ref = np.zeros(po.n_vars); np.add.at(t_ref, c, j_r * wt[r])
    ev = dto_amd.Evaluator(to_engine(po), shared_generators=flagged)
    try:
        ev.set_option("tdb_matrix_free_products", 1)

        def products():
            y = np.full(ev.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, po.Z0, w)
            t = np.full(ev.n_variables, np.nan); ev.eval_constraint_jacobian_transpose_product(t, po.Z0, wt)
            return y, t

        ev.set_option("tdb_resident", 3)
        ev.profile_enable(True); ev.profile_reset()
        y3, t3 = products()
        assert ev.profile_get("tdb_product")[1] == 2 * case[1] and ev.profile_get("tdb_mfma")[1] == 0   # matrix-free, no value call
        ev.profile_enable(False)
        errs = (rel_err(y3, y_ref), rel_err(t3, t_ref))
        print("matrix-free products, tdb_resident=3, flagged", flagged, errs)
        assert errs[0] <= TOL and errs[1] <= TOL, errs
        ev.set_option("tdb_resident", 0)
        y0, t0 = products()
        assert np.array_equal(y0, y3) and np.array_equal(t0, t3)
    finally:
        ev.close()


# ---- b. the real grid


def _n_long():
    import torch
    return PC.n_long(torch.cuda.get_device_properties(0).multi_processor_count)


def _periodic_on_device(short, N_L, mu_s, **kw):
    """(short handle, long handle, the short handle's vectors, the long handle's); the caller closes the handles."""
    import dto_amd
    long = PC.long_problem(short, N_L)
    ev_s, ev_l = dto_amd.Evaluator(to_engine(short), **kw), dto_amd.Evaluator(to_engine(long), **kw)
    return ev_s, ev_l, _all(ev_s, short.Z0, mu_s), _all(ev_l, long.Z0, PC.long_mu(short, mu_s, N_L))


def test_b_lone_kernel_at_the_real_grid():
    """k_tdb_mfma at the default grid with more intervals than two trips cover.  N_L = tdb_periodic_cases.n_long(CUs): 1031 knots,
    1030 intervals on 256 compute units, where the grid is 512 workgroups -- workgroups 0..5 make three trips, the other 506 two.  65
    states, one drive, order 1, 2 sub-steps, 2 modulations, and the DerivativeIntegrator's rows beside the integrator's.

    The short (five-knot) device handle is held to the reference at the bars; the long handle's g, J and H must be the tiling of the
    short DEVICE handle's vectors bit for bit -- every entry, the Hessian's knot-diagonal entries included: a long knot adds its two
    intervals' blocks and the objective's in the order the short knot does -- and the tiling of the reference's vectors at the bars.
    The tests named test_a_* walk the same loop at a reduced grid with the reference beside every interval."""
    N_L = _n_long()
    short = PC.short_problem(S.lone(65, 1, 1, 2, 2, 5))
    ev_o = O.OracleEvaluator(L.fast_problem(short))
    mu_s = PC.short_mu(short, np.random.default_rng(1).standard_normal(ev_o.n_constraints))
    ref_s = (ev_o.eval_constraint(short.Z0), ev_o.eval_constraint_jacobian(short.Z0), ev_o.eval_hessian_lagrangian(short.Z0, SIGMA, mu_s))
    ev_s, ev_l, got_s, got_l = _periodic_on_device(short, N_L, mu_s)
    try:
        assert ev_l.n_constraints == (N_L - 1) * 66
        _same_structure(ev_s, ev_o)
        _close_to("k_tdb_mfma, five knots", got_s, ref_s)
        _same_bits("k_tdb_mfma, %d knots against the tiled five-knot handle" % N_L, got_l, PC.tile(ev_s, ev_l, *got_s))
        _close_to("k_tdb_mfma, %d knots against the tiled reference" % N_L, got_l, PC.tile(ev_o, ev_l, *ref_s))
    finally:
        ev_s.close(); ev_l.close()


def test_b_group_kernel_at_the_real_grid():
    """k_tdb_mfma's group launch at the default grid, N_L knots as above (two and three trips per workgroup): 65 states x 2 kets of the same
    family, bit for bit the unflagged handle, whose kernel test_b_lone_kernel_at_the_real_grid holds to the reference."""
    import dto_amd
    N_L = _n_long()
    short = PC.short_problem(S.problem(65, 2, m=1, order=1, N=5))
    long = PC.long_problem(short, N_L)
    p = to_engine(long)
    ev, plain = dto_amd.Evaluator(p, shared_generators=True), dto_amd.Evaluator(p)
    try:
        assert ev.integrator_share(1) == (0, 2, 1)
        mu = np.random.default_rng(2).standard_normal(ev.n_constraints)
        _same_bits("k_tdb_mfma, group, %d knots against the unflagged handle" % N_L, _all(ev, long.Z0, mu), _all(plain, long.Z0, mu))
        assert _launches(ev, long.Z0, mu) == [1, 1, 1] and _launches(plain, long.Z0, mu) == [2, 2, 2]
    finally:
        ev.close(); plain.close()


def test_b_structured_kernel_at_the_real_grid():
    """k_tdb_kron (72 states as six 12 x 12 blocks) at the default grid, N_L knots: the tiling of its five-knot handle bit for bit."""
    N_L = _n_long()
    short = PC.short_problem(B.kron_tdb_problem(12, 6, 2, 1, 2, 2, N=5))
    mu_s = PC.short_mu(short, np.random.default_rng(1).standard_normal(4 * 72))
    ev_s, ev_l, got_s, got_l = _periodic_on_device(short, N_L, mu_s, block_generators=True)
    try:
        assert ev_s.integrator_blocks(0) == (12, 6, 1) and ev_l.integrator_blocks(0) == (12, 6, 1)
        _same_bits("k_tdb_kron, %d knots against the tiled five-knot handle" % N_L, got_l, PC.tile(ev_s, ev_l, *got_s))
    finally:
        ev_s.close(); ev_l.close()


# ---- c, d. group sizes and the scratch cap.  Expected caps: S.launch_cap, the slot formula of DESIGN 4.22 restated in Python
# (tests/test_tdb_persistent_host.py pins its figures); nothing is read back from the engine.


def _launch_count(P, cap):
    return len(range(0, P, cap)) if cap >= 2 else P


@functools.lru_cache(maxsize=None)
def _sized(key):
    """(problem, engine problem, reference) of c / d / e's cases, built once."""
    po = {"P8": lambda: S.problem(65, 8, m=1, order=0, N=3, derivative=False),
          "P5": lambda: S.problem(65, 5, m=2, order=1, N=3),
          "cap": lambda: S.problem(160, 5, m=3, order=1, substeps=2, n_mods=10, N=3),
          "two": lambda: S.problem(72, 4, m=1, members=[{}, {"u": 1}, {}, {"u": 1}])}[key]()
    return po, to_engine(po), S.reference(po, ("persistent", key))


def _reference_and_unflagged(key, share, launches):
    """The flagged handle of `_sized(key)` against the reference at the bars and the unflagged handle bit for bit; `share`: the
    expected integrator_share of every time-dependent member in list order; `launches`: per callback under "tdb_mfma"."""
    import dto_amd
    po, p, (ev_r, mu, g_r, j_r, h_r) = _sized(key)
    ev, plain = dto_amd.Evaluator(p, shared_generators=True), dto_amd.Evaluator(p)
    try:
        tdb = [i for i, it in enumerate(po.integrators) if isinstance(it, O.TimeDependentBilinearIntegrator)]
        assert [ev.integrator_share(i) for i in tdb] == share
        _same_structure(ev, ev_r)
        got = _all(ev, po.Z0, mu)
        _close_to("group %s" % key, got, (g_r, j_r, h_r))
        _same_bits("group %s against the unflagged handle" % key, got, _all(plain, po.Z0, mu))
        assert _launches(ev, po.Z0, mu) == [launches] * 3 and _launches(plain, po.Z0, mu) == [len(tdb)] * 3
        return ev
    except BaseException:
        ev.close()
        raise
    finally:
        plain.close()


def test_c_a_group_of_eight_is_one_launch():
    """65 states, order 0: TDB_SHARE_MAX members -- every lane of the unrolled vector pass, vsh[7 * 256 + r], 8 x 32 adjoint columns.
    Eight members are the handle's eight integrators (dto_create takes no more), so this problem has no DerivativeIntegrator.  For
    the same reason there is no group of nine: a launch of eight followed by a lone launch cannot be built, and the path that leaves
    a launch with one member is reached through the scratch cap instead (3 + 1, test_d_the_cap_follows_eval_hessian;
    tests/test_tdb_persistent_host.py pins the refusal of a ninth integrator)."""
    assert S.launch_cap(65, 1, 0, 2, 8, True) == 8
    _reference_and_unflagged("P8", [(0, 8, 1)] * 8, 1).close()


def test_c_five_members_at_order_one_with_two_drives():
    """p = 6 parameters, 21 pairs: 28 meaningful Hessian columns per member on a stride of 32, five members (160 columns)."""
    assert S.launch_cap(65, 2, 1, 2, 5, True) == 5
    _reference_and_unflagged("P5", [(0, 5, 1)] * 5, 1).close()


CAP_SHAPE = (160, 3, 1, 10)   # (n, m, order, n_mods): the Hessian slot passes 8 MiB at four members, the Jacobian's never up to eight


def test_d_the_scratch_cap_splits_five_members_into_three_and_two():
    cap = S.launch_cap(*CAP_SHAPE, 5, True)
    assert cap == 3 and _launch_count(5, cap) == 2
    ev = _reference_and_unflagged("cap", [(0, 5, 1)] * 5, 2)
    try:
        with pytest.raises(Exception, match=r"tdb_share_members.*\b3\b"):
            ev.set_option("tdb_share_members", cap + 1)
        ev.set_option("tdb_share_members", cap)
    finally:
        ev.close()


def test_d_the_cap_follows_eval_hessian():
    """Four members: with the Hessian 3 + 1 (the last one as a group of one), without it one launch of four; the unflagged
    handle's bits either way."""
    import dto_amd
    assert S.launch_cap(*CAP_SHAPE, 4, True) == 3 and S.launch_cap(*CAP_SHAPE, 4, False) == 4
    po = S.problem(160, 4, m=3, order=1, substeps=2, n_mods=10, N=3)
    p = to_engine(po)
    with_h, without, plain = (dto_amd.Evaluator(p, shared_generators=True), dto_amd.Evaluator(p, shared_generators=True, eval_hessian=False),
                              dto_amd.Evaluator(p))
    try:
        assert [e.integrator_share(3) for e in (with_h, without, plain)] == [(0, 4, 1), (0, 4, 1), (3, 1, 0)]
        mu = np.random.default_rng(6).standard_normal(plain.n_constraints)
        want = _all(plain, po.Z0, mu)
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
        _same_bits("3 + 1 members", _all(with_h, po.Z0, mu), want)
        _same_bits("4 members, no Hessian", _all(without, po.Z0, mu, hessian=False), want[:2])
        assert _launches(with_h, po.Z0, mu) == [2, 2, 2]
        assert _launches(without, po.Z0, mu, hessian=False) == [1, 1]
        with pytest.raises(Exception, match=r"tdb_share_members.*\b3\b"):
            with_h.set_option("tdb_share_members", 4)
        without.set_option("tdb_share_members", 4)
    finally:
        with_h.close(); without.close(); plain.close()


def test_d_a_group_the_cap_leaves_inactive():
    """256 states, 7 drives, 12 modulations: two members already take 14.7 MiB, so the group is reported and evaluated member by
    member (a lone integrator at this shape is tests/test_gpu_tdb_parameters.py's business: no reference here)."""
    import dto_amd
    assert S.launch_cap(256, 7, 0, 12, 2, True) == 1
    po = S.problem(256, 2, m=7, order=0, substeps=2, n_mods=12, N=3)
    p = to_engine(po)
    ev, plain = dto_amd.Evaluator(p, shared_generators=True), dto_amd.Evaluator(p)
    try:
        assert ev.integrator_share(0) == (0, 2, 0) and ev.integrator_share(1) == (0, 2, 0)
        mu = np.random.default_rng(7).standard_normal(ev.n_constraints)
        want = _all(plain, po.Z0, mu)
        assert all(np.isfinite(a).all() for a in want)
        _same_bits("inactive group", _all(ev, po.Z0, mu), want)
        assert _launches(ev, po.Z0, mu) == [2, 2, 2]
        with pytest.raises(Exception, match="tdb_share_members"):
            ev.set_option("tdb_share_members", 2)
    finally:
        ev.close(); plain.close()


# ---- e. two active groups in one handle


def test_e_two_interleaved_groups_each_with_its_leader_and_scratch():
    """Members 0 and 2 are driven by u, members 1 and 3 by v: groups {0, 2} and {1, 3}, interleaved in list order."""
    _reference_and_unflagged("two", [(0, 2, 1), (1, 2, 1), (0, 2, 1), (1, 2, 1)], 2).close()


# ---- f. call history


def test_f_results_do_not_depend_on_the_calls_before():
    """72 states x 3 kets, flagged: Z0, a perturbed point, Z0 again with other launch sizes and grids in between (two intervals on
    one workgroup: a second trip in a slot that last held another point's columns) -- the third result is a fresh handle's first."""
    import dto_amd
    case = S.CASES[1]
    po = S.case(*case)
    p = to_engine(po)
    mu = np.random.default_rng(8).standard_normal(S.reference(po, case)[1].size)
    Z1 = po.Z0 + 0.05 * np.random.default_rng(9).standard_normal(po.Z0.size)
    fresh = dto_amd.Evaluator(p, shared_generators=True)
    try:
        want = _all(fresh, po.Z0, mu)
    finally:
        fresh.close()
    ev = dto_amd.Evaluator(p, shared_generators=True)
    try:
        first = _all(ev, po.Z0, mu)
        ev.set_option("tdb_share_members", 2); ev.set_option("tdb_resident", 1)
        other = _all(ev, Z1, mu)
        assert not np.array_equal(other[0], first[0])
        ev.set_option("tdb_share_members", 1); ev.set_option("tdb_resident", 2)
        _all(ev, Z1, mu)
        ev.set_option("tdb_share_members", 3); ev.set_option("tdb_resident", 1)
        third = _all(ev, po.Z0, mu)
        _same_bits("first call", first, want)
        _same_bits("third call", third, want)
        ev.set_option("tdb_resident", 0)
        _same_bits("default grid again", _all(ev, po.Z0, mu), want)
    finally:
        ev.close()


# ---- g. the option's range


def test_g_tdb_resident_takes_zero_to_the_largest_grid():
    import dto_amd
    po = S.lone(65, 1, 0, 2, 2, 3)          # three knots: resident = min(3 + 1, two per compute unit) = 4
    ev = dto_amd.Evaluator(to_engine(po))
    try:
        for bad in (-1, 5, 1 << 40):
            with pytest.raises(dto_amd.EngineError, match=r"tdb_resident takes 0 .*\b4\b"):
                ev.set_option("tdb_resident", bad)
        for ok in (4, 1, 0):
            ev.set_option("tdb_resident", ok)
    finally:
        ev.close()
    # k_tdb (24 states) has no persistent grid: 0 only
    ev = dto_amd.Evaluator(to_engine(S.lone(24, 1, 0, 2, 2, 3)))
    try:
        for bad in (1, -1):
            with pytest.raises(dto_amd.EngineError, match=r"tdb_resident takes 0 .*\b0\b"):
                ev.set_option("tdb_resident", bad)
        ev.set_option("tdb_resident", 0)
    finally:
        ev.close()
