"""CPU: the handle option "tdb_matrix_free_products" at the boundary -- accepted by a handle (structure-only: no device), values other
than 0 and 1 refused with text, no new entry point and ABI version still 8, dto_set_option typed alike in the header, ctypes and the
Julia binding, and the option documented where each of them lists options."""
import ctypes as C
import os
import re

import pytest

import dto_amd
import dto_oracle as O
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
H_NOCOMMENT = re.sub(r"/\*.*?\*/", "", H, flags=re.S)
JL = open(os.path.join(ROOT, "integration", "DTOEngine.jl"), encoding="utf-8").read()
OPTION = "tdb_matrix_free_products"


@pytest.fixture()
def handle():
    ev = dto_amd.Evaluator(to_engine(O.make_tdb_problem()), device=-1)
    yield ev
    ev.close()


def test_a_handle_accepts_the_option(handle):
    handle.set_option(OPTION, 1)
    handle.set_option(OPTION, 0)


@pytest.mark.parametrize("value", [2, -1, 1 << 40])
def test_other_values_are_refused_with_text(handle, value):
    with pytest.raises(dto_amd.EngineError, match=OPTION + " takes 0 .* or 1"):
        handle.set_option(OPTION, value)
    handle.set_option(OPTION, 1)   # the handle stays usable


def test_unknown_names_are_still_refused(handle):
    with pytest.raises(dto_amd.EngineError, match="unknown option"):
        handle.set_option(OPTION + "_", 1)


def test_the_abi_version_stays_8_and_no_entry_point_was_added():
    v = int(re.search(r"#define DTO_ABI_VERSION (\d+)", H).group(1))
    assert v == dto_amd.capi.DTO_ABI_VERSION == 8
    assert int(re.search(r"const DTO_ABI_VERSION = Int32\((\d+)\)", JL).group(1)) == 8
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(dto_\w+)\(", H_NOCOMMENT, flags=re.M))
    assert declared == set(dto_amd.capi.SYMBOLS), declared ^ set(dto_amd.capi.SYMBOLS)
    assert not [n for n in declared if "tdb" in n]


def test_set_option_is_typed_alike_in_header_ctypes_and_julia():
    m = re.search(r"^int\s+dto_set_option\((.*?)\);", H_NOCOMMENT, flags=re.S | re.M)
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["dto_handle* h", "const char* name", "int64_t value"], args
    res, py_args = dto_amd.capi.SYMBOLS["dto_set_option"]
    assert res is C.c_int and list(py_args) == [dto_amd.capi.H, C.c_char_p, C.c_int64]
    jl = re.search(r"@ccall\(?\s*lib\.dto_set_option\((.*?)\)::(\w+)", JL, flags=re.S)
    assert jl.group(2) == "Cint"
    assert [a.split("::")[-1].strip() for a in jl.group(1).split(",")] == ["Ptr{Cvoid}", "Cstring", "Int64"]


def test_the_option_and_its_profile_name_are_documented():
    assert '"%s" (default 0)' % OPTION in H
    assert '"tdb_product"' in H
    assert OPTION in dto_amd.Evaluator.set_option.__doc__
    assert OPTION in JL
