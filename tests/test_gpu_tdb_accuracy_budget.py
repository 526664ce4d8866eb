"""GPU: the accuracy of the device TimeDependentBilinearIntegrator's kernels (csrc/dto_tdb.hip, dto_tdb_mfma.hip, dto_tdb_kron.hip),
held to the 320-bit fixtures tests/golden/tdbhp_*.npz (tests/tdb_hp_reference.py: the discrete map alone, every derivative a
difference of it) and not to another fp64 code.

The metric is the normwise error per interval and quantity class (tests/tdbhp_cases.py).  Every bar is read from the fixture: 16 x
the measured error of the repository's fp64 restatement of the scheme (tests/tdb_large_cases.py) against the same 320-bit values,
floored at 64 2^-53 -- between 7.1e-15 and 3.2e-14, fixed on the CPU by tests/golden/make_tdbhp_golden.py and checked by
tests/test_tdb_hp_reference.py, which also shows that a weight off by 1e-9, a missing step, a carrier at the wrong stage time, a
control held instead of interpolated and a dropped dt factor each land over one of them.  No bar is derived from engine output.

One handle per fixture; every callback runs once into NaN-filled outputs (the matrix-free products with the handle's option
"tdb_matrix_free_products" on, the slab route on a handle of its own).  Errors print per interval beside ||dt_k G(u_k, t_k)||_2
(0.05, 1 and 3 in shuffled order) and the launch counters, so a failure names its interval and the kernel that ran.

Fixtures: 4 states (k_tdb, forward Hessian form), 16 states (k_tdb, discrete-adjoint Hessian), 16 states at order 0 without a
carrier, 72 states (k_tdb_mfma on the 32-row tile, 96 padded rows; once more as a DTO_FLAG_SHARED_GENERATORS group of two), 128
states (the 64-row tile) and 12 x 3 blocks (k_tdb_kron).  With 16 sampled Phi columns above 64 states."""
import functools
import os
import re

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
import tdbhp_cases as C
from helpers import to_engine

pytestmark = pytest.mark.gpu

NAMES = list(C.CASES)
KERNEL = {"tdbhp_n4": "k_tdb", "tdbhp_n16": "k_tdb", "tdbhp_n16_o0": "k_tdb", "tdbhp_n72": "tdb_mfma", "tdbhp_n128": "tdb_mfma",
          "tdbhp_kron": "tdb_kron"}
COUNTERS = ("tdb_mfma", "tdb_kron", "tdb_product", "zero_fill", "all")


def _counts(ev):
    return {k: ev.profile_get(k)[1] for k in COUNTERS}


def _values(ev, d):
    """eval_constraint, the Jacobian and the Hessian (sigma = 0), each once into NaN; the launch counters of each call."""
    got, launches = {}, {}
    for key, size, call in (("cons", ev.shard.cons_len, lambda o: ev.eval_constraint(o, d["Z"])),
                            ("jac", ev.shard.jac_len, lambda o: ev.eval_constraint_jacobian(o, d["Z"])),
                            ("hess", ev.shard.hess_len, lambda o: ev.eval_hessian_lagrangian(o, d["Z"], 0.0, d["mu"]))):
        ev.profile_reset()
        got[key] = np.full(size, np.nan)
        call(got[key])
        launches[key] = _counts(ev)
    return got, launches


def _products(ev, d, pad=0):
    """J w and J' w, host-pointer forms; `pad` extra constraint rows of the handle take weight 0 and are cut off."""
    ev.profile_reset()
    y = np.full(ev.n_constraints, np.nan); ev.eval_constraint_jacobian_product(y, d["Z"], d["w"])
    wt = np.concatenate([d["wt"], np.zeros(pad)])
    t = np.full(ev.n_variables, np.nan); ev.eval_constraint_jacobian_transpose_product(t, d["Z"], wt)
    return dict(Jw=y[:y.size - pad] if pad else y, JTw=t), _counts(ev)


def _run(name, problem, d, resident=0, **kw):
    """Every callback of a fresh handle on `problem` at the inputs d: (vectors, {callback: launch counters})."""
    ev = dto_amd.Evaluator(to_engine(problem), **C.ENGINE_KW.get(name, {}), **kw)
    try:
        ev.set_option("tdb_matrix_free_products", 1)
        if resident:
            ev.set_option("tdb_resident", resident)
        ev.profile_enable(True)
        got, launches = _values(ev, d)
        prod, launches["products"] = _products(ev, d)
        got.update(prod)
        share = [ev.integrator_share(i) for i in range(len(problem.integrators))] if kw.get("shared_generators") else None
    finally:
        ev.close()
    return got, launches, share


@functools.lru_cache(maxsize=None)
def run(name, resident=0):
    """(fixture, vectors, {(class, k): error}, text, launch counters) of the fixture's one-member handle."""
    fix = C.load(name)
    p, _ = C.at_point(name, fix["Z"])
    got, launches, _ = _run(name, p, fix, resident)
    errs = C.errors(name, fix, got)
    text = C.report(name, fix, errs, f"engine vs fixture ({KERNEL[name]}{', tdb_resident=1' if resident else ''}): launches={launches}")
    print(text)
    return fix, got, errs, text, launches


def _assert_within(name, fix, errs, text, classes):
    seen = {cls for cls, _ in errs}
    assert classes <= seen, (name, sorted(classes - seen))
    bad = [(cls, k, v, C.bar_for(fix, cls)) for (cls, k), v in sorted(errs.items()) if cls in classes and not v <= C.bar_for(fix, cls)]
    assert not bad, f"{name}: over the bar (class, interval, error, bar): {bad}\n{text}"


def _jacobian_classes(name):
    c = C.CASES[name]
    cls = {"defect", "Phi", "t", "dt", "const"} | {f"u{j}" for j in range(c["m"])}
    return cls | ({f"un{j}" for j in range(c["m"])} if c["order"] == 1 else set())


@pytest.mark.parametrize("name", NAMES)
def test_values_and_jacobian_classes_stay_within_the_bars(name):
    fix, got, errs, text, _ = run(name)
    _assert_within(name, fix, errs, text, _jacobian_classes(name))


@pytest.mark.parametrize("name", NAMES)
def test_matrix_free_products_stay_within_the_bars(name):
    fix, got, errs, text, launches = run(name)
    assert launches["products"]["tdb_product"] == 2 and launches["products"]["zero_fill"] == 0, text    # no slab was formed
    _assert_within(name, fix, errs, text, {"Jw", "JTw"})


@pytest.mark.parametrize("name", NAMES)
def test_hessian_blocks_stay_within_the_bars(name):
    fix, got, errs, text, _ = run(name)
    _assert_within(name, fix, errs, text, {"hess", "hess_outside_blocks"})


def _with_external_row(p):
    """The same problem with one closure constraint row behind the dynamics rows: an external constraint keeps a handle's
    J w / J' w on the value-slab route (include/dto_engine.h), as tests/test_gpu_accuracy_budget.py chooses it."""
    u0 = p.integrators[0].u_off
    con = O.ClosureKnotConstraint(lambda v, q: np.array([v[0] * v[0] - 1.0]), lambda v, q: np.array([[2.0 * v[0]]]),
                                  lambda v, q, mu: np.array([[2.0 * mu[0]]]), [u0], [2], 1, equality=False)
    p.constraints = [con]
    return p


@pytest.mark.parametrize("name", NAMES)
def test_slab_route_products_stay_within_the_bars(name):
    fix = C.load(name)
    p, _ = C.at_point(name, fix["Z"])
    ev = dto_amd.Evaluator(to_engine(_with_external_row(p), closure_derivatives="analytic"), **C.ENGINE_KW.get(name, {}))
    try:
        ev.profile_enable(True)
        got, route = _products(ev, fix, pad=1)
    finally:
        ev.close()
    errs = C.errors(name, fix, got)
    text = C.report(name, fix, errs, f"engine (slab route) vs fixture: launches={route}")
    print(text)
    assert route["tdb_product"] == 0 and route["zero_fill"] >= 1, route   # the slab was formed and contracted
    _assert_within(name, fix, errs, text, {"Jw", "JTw"})


def test_shared_group_of_two_at_72_states():
    """tdbhp_n72 as a DTO_FLAG_SHARED_GENERATORS group of two (the MAXM = 8 instantiation of k_tdb_mfma's group form): one launch
    per callback, and each member -- its own x and mu -- against its own 320-bit values; the theta entries of J' w and the
    (theta, theta) entries of the Hessian, to which both members add, against the sums."""
    name = "tdbhp_n72"
    fix = C.load(name)
    pg, dg = C.group_problem(name, fix)
    got, launches, share = _run(name, pg, dg, shared_generators=True)
    assert share == [(0, 2, 1), (0, 2, 1)], share
    for cb in ("cons", "jac", "hess"):
        assert launches[cb]["tdb_mfma"] == 1 and launches[cb]["tdb_kron"] == 0, launches
    for q in range(2):
        mfix = C.member_fix(fix, q)
        errs = C.errors(name, mfix, C.member_got(name, fix, got, q))
        text = C.report(name, fix, errs, f"engine, group of two, member {q}: launches={launches}")
        print(text)
        _assert_within(name, fix, errs, text, _jacobian_classes(name) | {"Jw", "JTw", "hess", "hess_outside_blocks"})


@pytest.mark.parametrize("name", ["tdbhp_n72", "tdbhp_kron"])
def test_resident_grid_of_one_returns_the_default_grids_bits(name):
    """tdb_resident = 1: one workgroup walks the three intervals in one scratch slot."""
    fix, got, errs, text, launches = run(name)
    fix1, got1, errs1, text1, launches1 = run(name, resident=1)
    for key in got:
        assert np.array_equal(got[key], got1[key]), (name, key, int((got[key] != got1[key]).sum()))
    assert launches1 == launches, (launches, launches1)


def _source(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(dto_amd.__file__)), "directtrajopt.jl_amd", "csrc", name)) as f:
        return f.read()


def adjoint_threshold():
    """The state count from which k_tdb's Hessian runs the discrete adjoint, read from `tdb_uses_adjoint` in csrc/dto_tdb.hip."""
    return int(re.search(r"bool tdb_uses_adjoint\(int n\) \{ return n >= (\d+); \}", _source("dto_tdb.hip")).group(1))


def mfma_tile_rows(n):
    """The row tile k_tdb_mfma's launcher instantiates for n states: 64 where n padded to 32 is a multiple of 64, else 32 -- the
    rule as csrc/dto_tdb_mfma.hip states it (the test fails if the launcher's line reads otherwise)."""
    assert re.search(r"if \(tdbm_pad32\(a\.T\.n\) % 64 == 0\) hipLaunchKernelGGL\(\(k_tdb_mfma<64, MAXM, PROD>\).*\n\s*else hipLaunchKernelGGL\(\(k_tdb_mfma<32, MAXM, PROD>\)",
                     _source("dto_tdb_mfma.hip"))
    return 64 if (n + 31) // 32 * 32 % 64 == 0 else 32


@pytest.mark.parametrize("name", NAMES)
def test_each_fixture_ran_the_kernel_it_is_there_for(name):
    fix, got, errs, text, launches = run(name)
    n = C.CASES[name]["n"]
    for cb in ("cons", "jac", "hess"):
        L = launches[cb]
        if KERNEL[name] == "k_tdb":       # k_tdb has no counter of its own: up to 64 states, and neither of the others ran
            assert n <= 64 and L["tdb_mfma"] == 0 and L["tdb_kron"] == 0, text
        else:
            other = "tdb_kron" if KERNEL[name] == "tdb_mfma" else "tdb_mfma"
            assert L[KERNEL[name]] == 1 and L[other] == 0, text
        assert L["tdb_product"] == 0, text
    if KERNEL[name] == "k_tdb":           # ... and k_tdb alone has no persistent grid: its handle takes tdb_resident = 0 only
        ev = dto_amd.Evaluator(to_engine(C.at_point(name, fix["Z"])[0]))
        try:
            with pytest.raises(dto_amd.EngineError, match=r"tdb_resident takes 0 .*\b0\b"):
                ev.set_option("tdb_resident", 1)
        finally:
            ev.close()
    if name == "tdbhp_kron":
        assert n >= 33     # a family of blocks runs on its blocks from 33 states
    assert mfma_tile_rows(C.CASES["tdbhp_n72"]["n"]) == 32 and mfma_tile_rows(C.CASES["tdbhp_n128"]["n"]) == 64
    thr = adjoint_threshold()
    assert C.CASES["tdbhp_n4"]["n"] < thr <= C.CASES["tdbhp_n16"]["n"]
