"""CPU checks of the feasible-trajectory boundary (include/dto_engine.h, "Feasible trajectory"): the four entry points are declared,
exported, prototyped for ctypes and bound in the Julia file with matching argument counts; the ABI version is unchanged; a
structure-only handle, which needs no GPU, refuses all four with text and stays usable."""
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
# handle, Z, Zf (, stream) and handle, Z, sigma, mu, phi, Zf, g (, stream)
N_ARGS = {"dto_feasible_trajectory": 3, "dto_feasible_trajectory_dev": 4, "dto_feasible_merit": 7, "dto_feasible_merit_dev": 8}
NAMES = list(N_ARGS)


def header_text():
    return open(os.path.join(ROOT, "include", "dto_engine.h")).read()


def header_source():
    return re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)


def test_the_four_names_are_declared():
    src = header_source()
    for n in NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{n} is not declared"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == N_ARGS[n], (n, args)
        assert args[0] == "dto_handle* h"
        if "merit" in n:
            assert args[2] == "double sigma", (n, args)
        if n.endswith("_dev"):
            assert args[-1] == "void* stream", (n, args)
        # none of the words the other boundaries' tests collect their names by
        assert not any(w in n for w in ("reduced", "input", "tdb")), n
    assert re.search(r"#define\s+DTO_ABI_VERSION\s+8\b", src) and dto_amd.capi.DTO_ABI_VERSION == 8


def test_the_header_section_sits_between_the_block_products_and_multi_gpu():
    text = header_text()
    a, b, c = text.index("---- Block products"), text.index("---- Feasible trajectory"), text.index("---- Multi-GPU")
    assert a < b < c
    section = text[b:c]
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", section), n
    for word in ("halving", "in place", "Refused with text", "Kept points"):
        assert word in section, word
    assert '"feasible"' in text[text.index("int dto_profile_enable"):]


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
        assert sum(1 for a in args if a is C.c_double) == (1 if "merit" in n else 0), n
        if "merit" in n:
            assert args[2] is C.c_double, n
        assert not any(a is C.c_int32 for a in args), n


def test_the_julia_file_binds_them_with_matching_argument_counts():
    src = open(os.path.join(ROOT, "integration", "DTOEngine.jl")).read()
    assert "ABI version 8" in src.splitlines()[0]
    for n in NAMES:
        m = re.search(r"@ccall\s+lib\." + n + r"\((.*?)\)::Cint", src, flags=re.S)
        assert m, f"{n} has no @ccall"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == N_ARGS[n], (n, args)
        assert args[0].endswith("::Ptr{Cvoid}")
        if "merit" in n:
            assert args[2].endswith("::Float64"), (n, args)
        assert not any(a.endswith("::Int32") for a in args), (n, args)


@pytest.fixture()
def structure_only():
    ev = dto_amd.Evaluator(to_engine(O.make_scaled_problem(5, 6, 2, seed=4, with_constraint=True)), device=-1)
    yield ev
    ev.close()


def test_a_structure_only_handle_refuses_all_four_with_text_and_stays_usable(structure_only):
    ev = structure_only
    Z, mu = np.zeros(ev.n_variables), np.zeros(ev.n_constraints)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.feasible_trajectory_engine(Z)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.feasible_merit(Z, 1.0, mu, trajectory=True, constraints=True)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.feasible_trajectory_dev(0, 0)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.feasible_merit_dev(0, 1.0, 0, 0)
    rows, cols = ev.jacobian_structure()
    assert rows.size == ev.n_jacobian_entries == cols.size
    D, n_levels, offset, level = ev.dynamics_layout()   # the schedule's input needs no device
    assert D == 8 and n_levels == 2 and list(level) == [1, 0]   # the ket reads the controls the DerivativeIntegrator integrates
    with pytest.raises(ValueError, match="wrong length"):
        ev.feasible_merit(Z[:-1])


def test_the_docstrings_exist():
    E = dto_amd.Evaluator
    for f in (E.feasible_trajectory_engine, E.feasible_trajectory_dev, E.feasible_merit, E.feasible_merit_dev):
        assert f.__doc__ and len(f.__doc__) > 80, f.__name__
    assert E.feasible_trajectory.__doc__ and "Host vectors" in E.feasible_trajectory.__doc__   # the yardstick stays
    assert "Feasible trajectory" in header_text()
