"""CPU: the device-pointer Jacobian-vector product entry points (dto_eval_jacobian_product_dev, dto_eval_jacobian_transpose_product_dev)
at the boundary -- exported, five arguments typed alike in the header, ctypes and the Julia binding, ABI version still 8, and refused
with text where no GPU evaluates."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dto_amd
import dto_oracle as O
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
H_NOCOMMENT = re.sub(r"/\*.*?\*/", "", H, flags=re.S)
JL = open(os.path.join(ROOT, "integration", "DTOEngine.jl"), encoding="utf-8").read()
NAMES = ("dto_eval_jacobian_product_dev", "dto_eval_jacobian_transpose_product_dev")
JL_TYPE = {"dto_handle*": "Ptr{Cvoid}", "const double*": "Ptr{Float64}", "double*": "Ptr{Float64}", "void*": "Ptr{Cvoid}"}


def _prototype(name):
    m = re.search(r"^int\s+%s\((.*?)\);" % name, H_NOCOMMENT, flags=re.S | re.M)
    assert m, name
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    return [re.sub(r"\s+", " ", re.match(r"(.*?)(\w+)$", a).group(1).strip()).replace(" *", "*") for a in args]


def test_symbols_are_exported_and_the_abi_version_stays_8():
    lib = dto_amd.capi.library_path()
    assert os.path.exists(lib), lib
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dto_\w+)$", out, flags=re.M))
    for n in NAMES:
        assert n in exported, n
        assert n in dto_amd.capi.SYMBOLS, n
    v = int(re.search(r"#define DTO_ABI_VERSION (\d+)", H).group(1))
    assert v == dto_amd.capi.DTO_ABI_VERSION == 8
    assert int(re.search(r"const DTO_ABI_VERSION = Int32\((\d+)\)", JL).group(1)) == 8
    assert re.match(r"# DTOEngine\.jl .*ABI version 8\)", JL.splitlines()[0]), JL.splitlines()[0]


def test_header_declares_five_arguments_and_ctypes_follows():
    want = ["dto_handle*", "const double*", "const double*", "double*", "void*"]
    for n in NAMES:
        assert _prototype(n) == want, (n, _prototype(n))
        res, py_args = dto_amd.capi.SYMBOLS[n]
        assert res is C.c_int
        assert list(py_args) == [dto_amd.capi.H] + [C.c_void_p] * 4, (n, py_args)  # device form: opaque addresses


def test_julia_ccalls_have_the_header_signature():
    calls = re.findall(r"@ccall\(?\s*lib\.(dto_\w+)\((.*?)\)::(\w+)", JL, flags=re.S)
    seen = set()
    for name, args, ret in calls:
        if name not in NAMES:
            continue
        seen.add(name)
        assert ret == "Cint", name
        jl = [a.strip() for a in re.split(r",(?![^{]*\})", args) if a.strip()]
        c_args = _prototype(name)
        assert len(jl) == len(c_args) == 5, (name, jl, c_args)
        for a, c in zip(jl, c_args):
            assert a.split("::")[-1].strip() == JL_TYPE[c], (name, a, c)
    assert seen == set(NAMES), seen
    assert "eval_constraint_jacobian_product_dev!" in JL and "eval_constraint_jacobian_transpose_product_dev!" in JL


def test_python_mirror_has_both_forms():
    assert callable(getattr(dto_amd.Evaluator, "eval_jacobian_product_dev", None))
    assert callable(getattr(dto_amd.Evaluator, "eval_jacobian_transpose_product_dev", None))


def test_structure_only_handle_refuses_both_forms_with_text():
    ev = dto_amd.Evaluator(to_engine(O.make_readme_problem()), device=-1)
    try:
        for n in NAMES:
            rc = getattr(ev._lib, n)(ev.handle, None, None, None, None)
            assert rc != 0
            assert b"structure-only" in ev._lib.dto_last_error(ev.handle)
        with pytest.raises(dto_amd.EngineError, match="structure-only"):
            ev.eval_constraint_jacobian_product(np.empty(ev.n_constraints), np.zeros(ev.n_variables), np.ones(ev.n_variables))
    finally:
        ev.close()
