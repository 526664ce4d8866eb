"""CPU checks of the block products' boundary (include/dto_engine.h, "Block products"): the four entry points are declared, exported,
prototyped for ctypes and bound in the Julia file with matching argument counts; the ABI version is unchanged; the option
"reduced_block_width" and the refusals work on a structure-only handle, which needs no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["dto_eval_hessian_products", "dto_eval_hessian_products_dev", "dto_projected_hessian_products", "dto_projected_hessian_products_dev"]
N_ARGS = {n: 8 if n.endswith("_dev") else 7 for n in NAMES}   # handle, Z, sigma, mu, n_cols, V, Y (, stream)


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dto_engine.h")).read(), flags=re.S)


def test_the_four_names_are_declared_with_an_int32_column_count():
    src = header_source()
    for n in NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{n} is not declared"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == N_ARGS[n], (n, args)
        assert args[4] == "int32_t n_cols", (n, args)
        assert args[0] == "dto_handle* h" and args[2] == "double sigma"
    assert re.search(r"#define\s+DTO_ABI_VERSION\s+8\b", src) and dto_amd.capi.DTO_ABI_VERSION == 8


def test_the_library_exports_them(engine_lib):
    lib = os.path.join(ROOT, "directtrajopt.jl_amd", "libdto_engine.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NAMES:
        assert n in exported, f"{n} is not exported"
        assert hasattr(engine_lib, n)


def test_the_ctypes_prototypes():
    for n in NAMES:
        res, args = dto_amd.capi.SYMBOLS[n]
        assert res is C.c_int and len(args) == N_ARGS[n], n
        assert args[4] is C.c_int32 and args[2] is C.c_double, n
        assert sum(1 for a in args if a is C.c_int32) == 1, n


def test_the_julia_file_binds_them_with_matching_argument_counts():
    src = open(os.path.join(ROOT, "integration", "DTOEngine.jl")).read()
    assert "ABI version 8" in src.splitlines()[0]
    assert '"reduced_block_width"' in src
    for n in NAMES:
        m = re.search(r"@ccall\s+lib\." + n + r"\((.*?)\)::Cint", src, flags=re.S)
        assert m, f"{n} has no @ccall"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == N_ARGS[n], (n, args)
        assert args[4].endswith("::Int32") and args[2].endswith("::Float64"), (n, args)
        assert sum(1 for a in args if a.endswith("::Int32")) == 1


@pytest.fixture()
def structure_only():
    ev = dto_amd.Evaluator(to_engine(O.make_scaled_problem(5, 6, 2, seed=4, with_constraint=True)), device=-1)
    yield ev
    ev.close()


def test_the_option_on_a_structure_only_handle(structure_only):
    ev = structure_only
    for value in (0, 1, 64):
        ev.set_option("reduced_block_width", value)
    for value in (-1, 65, 1 << 40):
        with pytest.raises(dto_amd.EngineError, match="reduced_block_width takes 0 .* 1 .. 64"):
            ev.set_option("reduced_block_width", value)
    ev.set_option("reduced_block_width", 3)   # still usable


def test_a_structure_only_handle_refuses_all_four_with_text_and_stays_usable(structure_only):
    ev = structure_only
    n, m = ev.n_variables, ev.n_constraints
    Z, mu, V, Y = np.zeros(n), np.zeros(m), np.zeros((2, n)), np.zeros((2, n))
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.eval_hessian_lagrangian_products(Y, Z, V, 1.0, mu)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_hessian_products(Z, V, 1.0, mu)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.eval_hessian_products_dev(0, 1.0, 0, 2, 0, 0)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_hessian_products_dev(0, 1.0, 0, 2, 0, 0)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_hessian_matrix(Z)
    rows, cols = ev.jacobian_structure()
    assert rows.size == ev.n_jacobian_entries == cols.size
    with pytest.raises(ValueError, match="expected \\(n_cols"):
        ev.reduced_hessian_products(Z, np.zeros(n))
    C_ = ev.independent_entries()
    assert C_.size < n and np.all(np.diff(C_) > 0) and np.array_equal(C_[:ev.trajectory.dim], np.arange(ev.trajectory.dim))


def test_the_docstrings_exist():
    E = dto_amd.Evaluator
    for f in (E.eval_hessian_lagrangian_products, E.reduced_hessian_products, E.eval_hessian_products_dev, E.reduced_hessian_products_dev,
              E.reduced_hessian_matrix):
        assert f.__doc__ and len(f.__doc__) > 80, f.__name__
    assert "reduced_block_width" in E.set_option.__doc__
    assert "Block products" in open(os.path.join(ROOT, "include", "dto_engine.h")).read()
