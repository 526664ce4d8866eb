"""CPU checks of the augmented-Lagrangian boundary (include/dto_engine.h, "Augmented-Lagrangian terms"): the ten entry points are
declared, exported and typed alike in the header, the ctypes table and the Julia file; a structure-only handle, which needs no GPU,
refuses with text and stays usable; a handle with a host-evaluated constraint, a negative or NaN penalty (naming the row), a bad argument
of the step and every overlap of an output with an input are refused with text; and the penalty helper of the problem mirror expands
penalties over the rows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import to_engine
from test_newton_abi import BAD, c_kind, header_source, header_text, julia_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = ["handle", "ptr", "double", "ptr", "ptr", "ptr", "ptr", "ptr", "double", "double", "double", "double", "int32", "ptr", "ptr", "ptr", "ptr", "ptr"]
KINDS = {
    "dto_auglag_rows": ["handle", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"],                                  # Z, mu, rho, mu_eff, weight, info
    "dto_auglag_merit": ["handle", "ptr", "double", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"],               # Z, sigma, mu, rho, phi, Zf, g, info
    "dto_auglag_gradient": ["handle", "ptr", "double", "ptr", "ptr", "ptr", "ptr", "ptr"],                    # Z, sigma, mu, rho, grad, lam, mu_eff
    "dto_auglag_hessian_products": ["handle", "ptr", "double", "ptr", "ptr", "int32", "ptr", "ptr"],          # Z, sigma, mu, rho, n_cols, V, Y
    "dto_auglag_newton_step": STEP,          # Z, sigma, mu, rho, free_mask, lo, hi, radius, shift, rtol, atol, max_iter, p, info, trace, entry_state, Zp
}
NAMES = [n + s for n in KINDS for s in ("", "_dev")]


def kinds_of(name):
    return KINDS[name[:-4]] + ["stream"] if name.endswith("_dev") else KINDS[name]


def test_the_ten_names_are_declared_and_typed():
    src = header_source()
    for n in NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{n} is not declared"
        assert [c_kind(a) for a in m.group(1).split(",")] == kinds_of(n), n
    assert re.search(r"#define\s+DTO_ABI_VERSION\s+8\b", src) and dto_amd.capi.DTO_ABI_VERSION == 8, "additions only: the version stays"


def test_the_ctypes_prototypes_are_typed_like_the_header():
    host = {"handle": C.c_void_p, "ptr": dto_amd.capi.c_double_p, "double": C.c_double, "int32": C.c_int32}
    dev = dict(host, ptr=C.c_void_p, stream=C.c_void_p)
    for n in NAMES:
        res, args = dto_amd.capi.SYMBOLS[n]
        assert res is C.c_int
        table = dev if n.endswith("_dev") else host
        assert list(args) == [table[k] for k in kinds_of(n)], n


def test_the_julia_file_names_every_entry_point_typed_like_the_header():
    src = julia_source()
    jl = {"handle": "Ptr{Cvoid}", "ptr": "Ptr{Float64}", "double": "Float64", "int32": "Int32", "stream": "Ptr{Cvoid}"}
    for n in NAMES:
        m = re.search(r"@ccall\s+lib\." + n + r"\((.*?)\)::Cint", src, flags=re.S)
        assert m, f"{n} has no @ccall"
        types = [a.strip().split("::")[-1] for a in m.group(1).split(",")]
        assert types == [jl[k] for k in kinds_of(n)], (n, types)
    for f in ("auglag_rows", "auglag_merit", "auglag_gradient", "auglag_hessian_products", "auglag_hessian_product", "auglag_newton_step",
              "penalty_vector"):
        assert re.search(r"^(function )?" + f + r"\(", src, flags=re.M), f


def test_the_header_section_the_plan_header_and_the_profile_name():
    text = header_text()
    a, b, c = text.index("---- Bound-constrained truncated-Newton step"), text.index("---- Augmented-Lagrangian terms"), text.index("---- Multi-GPU")
    assert a < b < c
    section = text[b:c]
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", section), n
    for word in ("Powell", "mult", "weight", "inactive", "rho == NULL", "Refused with text", "rounded on its own", "info [8]", "max viol",
                 "host-evaluated", "naming the row", "overlap", "bit for bit", "J_c' W J_c", "al_row"):
        assert word in section, word
    assert '"auglag"' in text[text.index("int dto_profile_enable"):]
    plan = open(os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_auglag_plan.h")).read()
    assert '#include "dto_newton_plan.h"' in plan and "hip" not in re.sub(r"//.*", "", plan).lower().replace("__hipcc__", "")
    assert "dto_auglag.$(O)" in open(os.path.join(ROOT, "Makefile")).read()


def test_the_library_exports_them(engine_lib):
    lib = os.path.join(ROOT, "directtrajopt.jl_amd", "libdto_engine.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NAMES:
        assert n in exported, f"{n} is not exported"
        assert hasattr(engine_lib, n)


@pytest.fixture()
def structure_only():
    p = O.make_scaled_problem(5, 6, 2, seed=4, with_constraint=True)
    p.constraints.append(O.KnotConstraint("sqnorm", [6, 7], 0.01, [3], equality=True))
    ev = dto_amd.Evaluator(to_engine(p), device=-1)
    yield ev
    ev.close()


def calls(ev, rho):
    """every host-pointer call with good arguments"""
    n, m = ev.n_variables, ev.n_constraints
    Z, mu = np.zeros(n), np.zeros(m)
    return {"dto_auglag_rows": lambda: ev.auglag_rows(Z, mu, rho),
            "dto_auglag_merit": lambda: ev.auglag_merit(Z, 0.7, mu, rho, info=True),
            "dto_auglag_gradient": lambda: ev.auglag_gradient(Z, 0.7, mu, rho, multipliers=True),
            "dto_auglag_hessian_products": lambda: ev.auglag_hessian_products(Z, np.ones((2, n)), 0.7, mu, rho),
            "dto_auglag_newton_step": lambda: ev.auglag_newton_step(Z, 0.7, mu, rho, lo=np.full(n, -1.0), hi=np.ones(n), radius=1.0, max_iter=3,
                                                                    trace=True, states=True, trajectory=True)}


def test_a_structure_only_handle_refuses_with_text_and_stays_usable(structure_only):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    for rho in (np.full(m, 10.0), None):
        for name, call in calls(ev, rho).items():
            with pytest.raises(dto_amd.EngineError, match="structure-only"):
                call()
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.auglag_newton_step_dev(8, 1.0, 0, 8 + 8 * n, 0, 0, 0, 0.0, 0.0, 1e-6, 0.0, 5, 8 + 16 * n, 8 + 32 * n)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.auglag_rows_dev(8, 0, 8 + 8 * n)
    rows, cols = ev.jacobian_structure()
    assert rows.size == ev.n_jacobian_entries == cols.size
    with pytest.raises(ValueError, match="rho"):
        ev.auglag_rows(np.zeros(n), rho=np.ones(3))
    with pytest.raises(ValueError, match="mu"):
        ev.auglag_gradient(np.zeros(n), mu=np.ones(3), rho=np.ones(m))


@pytest.mark.parametrize("bad", [-1.0, -1e-300, np.nan, -np.inf])
def test_a_negative_or_nan_penalty_is_refused_naming_the_row(structure_only, bad):
    ev = structure_only
    m, n_dyn = ev.n_constraints, ev.n_dynamics_constraints
    row = n_dyn + 2
    rho = np.full(m, 10.0)
    rho[row] = bad
    for name, call in calls(ev, rho).items():
        with pytest.raises(dto_amd.EngineError, match=rf"rho\[{row}\]") as e:
            call()
        assert f"(row {row})" in str(e.value) and name in str(e.value) and "structure-only" not in str(e.value)
    rho = np.full(m, 10.0)
    rho[:n_dyn] = bad                             # the dynamics rows are not read
    rho[-1] = 0.0                                 # 0 is a penalty: the row is not penalised
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.auglag_rows(np.zeros(ev.n_variables), None, rho)


def test_a_handle_with_a_host_evaluated_constraint_is_refused_with_text():
    for make in (O.make_closure_problem, O.make_global_problem):
        ev = dto_amd.Evaluator(to_engine(make()), device=-1)
        try:
            for rho in (np.zeros(ev.n_constraints), None):
                for name, call in calls(ev, rho).items():
                    with pytest.raises(dto_amd.EngineError, match="host-evaluated constraint") as e:
                        call()
                    assert name in str(e.value) and "global constraints are among these" in str(e.value)
        finally:
            ev.close()


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in BAD])
def test_what_the_box_step_refuses_is_refused_with_text(structure_only, kw, word):
    ev = structure_only
    n = ev.n_variables
    with pytest.raises(dto_amd.EngineError, match=word) as e:
        ev.auglag_newton_step(np.zeros(n), rho=np.full(ev.n_constraints, 10.0), **kw)
    assert "structure-only" not in str(e.value) and "dto_auglag_newton_step" in str(e.value)
    with pytest.raises(dto_amd.EngineError, match=word):
        ev.auglag_newton_step_dev(8, 1.0, 0, 8 + 8 * n, 0, 0, 0, kw.get("radius", 0.0), kw.get("shift", 0.0), kw.get("rtol", 1e-6),
                                  kw.get("atol", 0.0), kw.get("max_iter", 5), 8 + 16 * n, 8 + 32 * n)


def dp(a):
    return None if a is None else a.ctypes.data_as(dto_amd.capi.c_double_p)


def test_overlapping_outputs_are_refused_with_text(structure_only):
    """every output against every input it could share memory with, the whole vector and a single shared entry"""
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    lib, h = ev._lib, ev._h
    pool = np.zeros(12 * (n + m))
    cut = lambda k, size: pool[k * (n + m):k * (n + m) + size]
    Z, V, mu, rho = cut(0, n), cut(10, n), cut(2, m), cut(3, m)          # (behind V lies nothing: an alias of its last entry meets V alone)
    rho[:] = 10.0
    pool_before = pool.copy()

    def last_entry_of(a):
        start = (a.ctypes.data - pool.ctypes.data) // 8
        return pool[start + a.size - 1:][:a.size]

    def refused(rc, out_name, in_name):
        text = lib.dto_last_error(h).decode()
        assert rc != 0 and f"{out_name} overlaps {in_name}" in text and "structure-only" not in text, (out_name, in_name, text)

    for in_name, a in (("mu", mu), ("rho", rho)):
        for alias in (a, last_entry_of(a)):
            refused(lib.dto_auglag_rows(h, dp(Z), dp(mu), dp(rho), dp(alias), None, None), "mu_eff", in_name)
            refused(lib.dto_auglag_rows(h, dp(Z), dp(mu), dp(rho), None, dp(alias), None), "weight", in_name)
            refused(lib.dto_auglag_rows(h, dp(Z), dp(mu), dp(rho), None, None, dp(alias)), "info", in_name)
            refused(lib.dto_auglag_merit(h, dp(Z), 1.0, dp(mu), dp(rho), dp(cut(4, 1)), None, dp(alias), None), "g", in_name)
            refused(lib.dto_auglag_merit(h, dp(Z), 1.0, dp(mu), dp(rho), dp(alias), None, None, None), "phi", in_name)
            refused(lib.dto_auglag_gradient(h, dp(Z), 1.0, dp(mu), dp(rho), dp(cut(4, n)), None, dp(alias)), "mu_eff", in_name)
            refused(lib.dto_auglag_newton_step(h, dp(Z), 1.0, dp(mu), dp(rho), None, None, None, 0.0, 0.0, 1e-6, 0.0, 5, dp(cut(4, n)), dp(alias),
                                               None, None, None), "info", in_name)
    for alias in (Z, last_entry_of(Z)):
        refused(lib.dto_auglag_rows(h, dp(Z), dp(mu), dp(rho), None, None, dp(alias)), "info", "Z")
        refused(lib.dto_auglag_merit(h, dp(Z), 1.0, dp(mu), dp(rho), dp(cut(4, 1)), dp(alias), None, None), "Zf", "Z")
        refused(lib.dto_auglag_gradient(h, dp(Z), 1.0, dp(mu), dp(rho), dp(alias), None, None), "grad", "Z")
        refused(lib.dto_auglag_hessian_products(h, dp(Z), 1.0, dp(mu), dp(rho), 1, dp(V), dp(alias)), "Y", "Z")
        refused(lib.dto_auglag_newton_step(h, dp(Z), 1.0, dp(mu), dp(rho), None, None, None, 0.0, 0.0, 1e-6, 0.0, 5, dp(alias), dp(cut(4, 12)),
                                           None, None, None), "p", "Z")
    refused(lib.dto_auglag_hessian_products(h, dp(Z), 1.0, dp(mu), dp(rho), 1, dp(V), dp(last_entry_of(V))), "Y", "V")
    refused(lib.dto_auglag_newton_step(h, dp(Z), 1.0, dp(mu), dp(rho), None, None, None, 0.0, 0.0, 1e-6, 0.0, 5, dp(cut(4, n)), dp(cut(5, 12)),
                                       None, None, dp(rho)), "Zp", "rho")        # (judged by the addresses; nothing is written)
    assert np.array_equal(pool, pool_before), "nothing was written"
    base = 1 << 20
    assert lib.dto_auglag_rows_dev(h, base, None, base + 8 * n, base + 8 * (n + m - 1), None, None, None) != 0
    assert "dmu_eff overlaps drho" in lib.dto_last_error(h).decode()
    assert lib.dto_auglag_rows(h, dp(Z), dp(mu), dp(rho), dp(cut(4, m)), dp(cut(5, m)), dp(cut(6, 8))) != 0
    assert "structure-only" in lib.dto_last_error(h).decode(), "disjoint buffers: the handle is judged next"


def test_null_pointers_are_refused_with_text(structure_only):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    lib, h = ev._lib, ev._h
    rho, p, info = np.full(m, 10.0), np.full(n, np.nan), np.full(12, np.nan)
    assert lib.dto_auglag_rows(h, None, None, dp(rho), None, None, None) != 0 and "NULL" in lib.dto_last_error(h).decode()
    for z_, p_, i_ in ((None, p, info), (np.zeros(n), None, info), (np.zeros(n), p, None)):
        assert lib.dto_auglag_newton_step(h, dp(z_), 1.0, None, dp(rho), None, None, None, 0.0, 0.0, 1e-6, 0.0, 5, dp(p_), dp(i_), None, None, None) != 0
        text = lib.dto_last_error(h).decode()
        assert "NULL" in text and "dto_auglag_newton_step" in text
    assert np.isnan(p).all() and np.isnan(info).all()


def test_the_docstrings_exist():
    E = dto_amd.Evaluator
    for f in (E.auglag_rows, E.auglag_merit, E.auglag_gradient, E.auglag_hessian_products, E.auglag_hessian_product, E.auglag_newton_step,
              E.auglag_rows_dev, E.auglag_merit_dev, E.auglag_gradient_dev, E.auglag_hessian_products_dev, E.auglag_newton_step_dev,
              dto_amd.DirectTrajOptProblem.penalty_vector):
        assert f.__doc__ and len(f.__doc__) > 60, f.__name__


# ------------------------------------------------------------------------------------------------------ the penalty helper
def test_the_penalty_helper_expands_over_the_rows():
    p = O.make_scaled_problem(5, 6, 2, seed=4, with_constraint=True)
    p.constraints.append(O.KnotConstraint("sqnorm", [6, 7], 0.01, [3, 4], equality=True))
    pe = to_engine(p)
    ev = dto_amd.Evaluator(pe, device=-1)
    try:
        n_dyn, m = ev.n_dynamics_constraints, ev.n_constraints
    finally:
        ev.close()
    rho = pe.penalty_vector(10.0)
    assert rho.shape == (m,) and np.all(rho[:n_dyn] == 0.0) and np.all(rho[n_dyn:] == 10.0)
    rho = pe.penalty_vector({1: 3.0})
    assert np.all(rho[:m - 2] == 0.0) and np.array_equal(rho[m - 2:], [3.0, 3.0]), "constraints a dict does not name are not penalised"
    rho = pe.penalty_vector({0: [1.0, 2.0, 3.0], 1: 0.5})
    assert np.array_equal(rho[n_dyn:], [1.0, 2.0, 3.0, 0.5, 0.5])
    with pytest.raises(ValueError, match="rows"):
        pe.penalty_vector({0: [1.0, 2.0]})
    with pytest.raises(ValueError, match=">= 0"):
        pe.penalty_vector(-1.0)
    with pytest.raises(ValueError, match=">= 0"):
        pe.penalty_vector({1: np.nan})
    with pytest.raises(KeyError, match="no constraint"):
        pe.penalty_vector({2: 1.0})
