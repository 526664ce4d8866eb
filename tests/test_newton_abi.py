"""CPU checks of the truncated-Newton boundary (include/dto_engine.h, "Truncated-Newton step"): the two entry points are declared,
exported and typed alike in the header, the ctypes table and the Julia file; the status constants are equal in all three; the set the
header declares is the set capi.SYMBOLS prototypes; a structure-only handle, which needs no GPU, refuses with text and stays usable; and
every bad argument is refused with text naming it."""
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
NAMES = ["dto_projected_newton_step", "dto_projected_newton_step_dev"]
# handle, Z, sigma, mu, free_mask, radius, shift, rtol, atol, max_iter, p, info, trace (, stream)
KINDS = ["handle", "ptr", "double", "ptr", "ptr", "double", "double", "double", "double", "int32", "ptr", "ptr", "ptr"]
STATUS = {"CONVERGED": 0, "BOUNDARY": 1, "NEG_CURVATURE": 2, "MAX_ITER": 3, "NOT_FINITE": 4}


def header_text():
    return open(os.path.join(ROOT, "include", "dto_engine.h")).read()


def header_source():
    return re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)


def julia_source():
    return open(os.path.join(ROOT, "integration", "DTOEngine.jl")).read()


def kinds_of(name):
    return KINDS + (["stream"] if name.endswith("_dev") else [])


def c_kind(arg):
    arg = " ".join(arg.split())
    if arg == "dto_handle* h":
        return "handle"
    if arg == "void* stream":
        return "stream"
    if re.fullmatch(r"(const )?double\* \w+", arg):
        return "ptr"
    if re.fullmatch(r"double \w+", arg):
        return "double"
    if re.fullmatch(r"int32_t \w+", arg):
        return "int32"
    return "?" + arg


def test_the_two_names_are_declared_and_typed():
    src = header_source()
    for n in NAMES:
        m = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{n} is not declared"
        assert [c_kind(a) for a in m.group(1).split(",")] == kinds_of(n), n
        # none of the words the other boundaries' tests collect their names by
        assert not any(w in n for w in ("reduced", "input", "tdb")), n
    assert re.search(r"#define\s+DTO_ABI_VERSION\s+8\b", src) and dto_amd.capi.DTO_ABI_VERSION == 8


def test_the_ctypes_prototypes_are_typed_like_the_header():
    host = {"handle": C.c_void_p, "ptr": dto_amd.capi.c_double_p, "double": C.c_double, "int32": C.c_int32}
    dev = dict(host, ptr=C.c_void_p, stream=C.c_void_p)
    for n in NAMES:
        res, args = dto_amd.capi.SYMBOLS[n]
        assert res is C.c_int
        table = dev if n.endswith("_dev") else host
        assert list(args) == [table[k] for k in kinds_of(n)], n


def test_the_julia_file_binds_them_typed_like_the_header():
    src = julia_source()
    assert "ABI version 8" in src.splitlines()[0]
    jl = {"handle": "Ptr{Cvoid}", "ptr": "Ptr{Float64}", "double": "Float64", "int32": "Int32", "stream": "Ptr{Cvoid}"}
    for n in NAMES:
        m = re.search(r"@ccall\s+lib\." + n + r"\((.*?)\)::Cint", src, flags=re.S)
        assert m, f"{n} has no @ccall"
        types = [a.strip().split("::")[-1] for a in m.group(1).split(",")]
        assert types == [jl[k] for k in kinds_of(n)], (n, types)


def test_the_status_constants_are_equal_in_all_three():
    defs = dict(re.findall(r"#define (DTO_NEWTON_\w+) (\d+)", header_source()))
    consts = dict(re.findall(r"const (DTO_NEWTON_\w+) = Int32\((\d+)\)", julia_source()))
    assert set(defs) == set(consts) == {"DTO_NEWTON_" + k for k in STATUS}
    for k, v in STATUS.items():
        assert int(defs["DTO_NEWTON_" + k]) == int(consts["DTO_NEWTON_" + k]) == getattr(dto_amd.capi, "NEWTON_" + k) == v, k


def test_the_declared_set_is_the_prototyped_set():
    declared = set(re.findall(r"^(?:const )?\w+\*?\s+\*?(dto_\w+)\(", header_source(), flags=re.M))
    assert declared == set(dto_amd.capi.SYMBOLS), declared ^ set(dto_amd.capi.SYMBOLS)


def test_the_header_section_and_the_profile_name():
    text = header_text()
    a, b, c = text.index("---- Feasible trajectory"), text.index("---- Truncated-Newton step"), text.index("---- Multi-GPU")
    assert a < b < c
    section = text[b:c]
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", section), n
    for word in ("halving", "chunks of 256", "newton_decide", "Refused with text", "tau = ", "rounded on its own"):
        assert word in section, word
    assert '"newton"' in text[text.index("int dto_profile_enable"):]


def test_the_library_exports_them(engine_lib):
    lib = os.path.join(ROOT, "directtrajopt.jl_amd", "libdto_engine.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NAMES:
        assert n in exported, f"{n} is not exported"
        assert hasattr(engine_lib, n)


@pytest.fixture()
def structure_only():
    ev = dto_amd.Evaluator(to_engine(O.make_scaled_problem(5, 6, 2, seed=4, with_constraint=True)), device=-1)
    yield ev
    ev.close()


def test_a_structure_only_handle_refuses_with_text_and_stays_usable(structure_only):
    ev = structure_only
    Z, mu = np.zeros(ev.n_variables), np.zeros(ev.n_constraints)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_newton_step(Z)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_newton_step(Z, 0.7, mu, free=np.ones(ev.n_variables), radius=1.0, shift=2.0, max_iter=3, trace=True)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):
        ev.reduced_newton_step_dev(8, 1.0, 0, 0, 0.0, 0.0, 1e-6, 0.0, 5, 8, 8)
    rows, cols = ev.jacobian_structure()
    assert rows.size == ev.n_jacobian_entries == cols.size
    with pytest.raises(ValueError, match="wrong length"):
        ev.reduced_newton_step(Z[:-1])
    with pytest.raises(ValueError, match="free"):
        ev.reduced_newton_step(Z, free=np.ones(3))


BAD = [
    (dict(max_iter=0), "max_iter"), (dict(max_iter=-3), "max_iter"),
    (dict(radius=-1.0), "radius"), (dict(radius=np.nan), "radius"), (dict(radius=np.inf), "radius"),
    (dict(rtol=-1e-3), "rtol"), (dict(rtol=np.nan), "rtol"), (dict(rtol=np.inf), "rtol"),
    (dict(atol=-1e-3), "atol"), (dict(atol=np.nan), "atol"), (dict(atol=np.inf), "atol"),
    (dict(shift=np.nan), "shift"), (dict(shift=np.inf), "shift"), (dict(shift=-np.inf), "shift"),
]


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in BAD])
def test_bad_arguments_are_refused_with_text(structure_only, kw, word):
    """the arguments are judged before the handle is: a structure-only handle names the bad one (a good call says "structure-only")"""
    ev = structure_only
    Z = np.zeros(ev.n_variables)
    with pytest.raises(dto_amd.EngineError, match=word) as e:
        ev.reduced_newton_step(Z, **kw)
    assert "structure-only" not in str(e.value)
    with pytest.raises(dto_amd.EngineError, match=word):
        ev.reduced_newton_step_dev(8, 1.0, 0, 0, kw.get("radius", 0.0), kw.get("shift", 0.0), kw.get("rtol", 1e-6), kw.get("atol", 0.0),
                                   kw.get("max_iter", 5), 8, 8)
    with pytest.raises(dto_amd.EngineError, match="structure-only"):   # usable, and a negative shift is no error
        ev.reduced_newton_step(Z, shift=-2.0)


def test_null_pointers_are_refused_with_text(structure_only):
    ev = structure_only
    lib, h = ev._lib, ev._h
    Z, p, info = np.zeros(ev.n_variables), np.full(ev.n_variables, np.nan), np.full(8, np.nan)
    dp = lambda a: a.ctypes.data_as(dto_amd.capi.c_double_p)
    for z_, p_, i_ in ((None, dp(p), dp(info)), (dp(Z), None, dp(info)), (dp(Z), dp(p), None)):
        assert lib.dto_projected_newton_step(h, z_, 1.0, None, None, 0.0, 0.0, 1e-6, 0.0, 5, p_, i_, None) != 0
        assert "NULL" in lib.dto_last_error(h).decode()
    for z_, p_, i_ in ((None, 8, 8), (8, None, 8), (8, 8, None)):
        assert lib.dto_projected_newton_step_dev(h, z_, 1.0, None, None, 0.0, 0.0, 1e-6, 0.0, 5, p_, i_, None, None) != 0
        assert "NULL" in lib.dto_last_error(h).decode()
    assert np.isnan(p).all() and np.isnan(info).all()
    assert ev.jacobian_structure()[0].size == ev.n_jacobian_entries


def test_the_docstrings_exist():
    E = dto_amd.Evaluator
    for f in (E.reduced_newton_step, E.reduced_newton_step_dev):
        assert f.__doc__ and len(f.__doc__) > 80, f.__name__
