"""CPU: the handle option "reduced_input_store" at the boundary -- accepted by a handle (structure-only: no device) as 0 and 1, other
values refused with text while the handle stays usable, no new entry point and ABI version still 8, and the option with its profile
name documented where each binding lists options."""
import os
import re

import pytest

import dto_amd
from elim_cases import three_level_problem
from helpers import to_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
H_NOCOMMENT = re.sub(r"/\*.*?\*/", "", H, flags=re.S)
JL = open(os.path.join(ROOT, "integration", "DTOEngine.jl"), encoding="utf-8").read()
DESIGN = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
OPTION = "reduced_input_store"


@pytest.fixture()
def handle():
    ev = dto_amd.Evaluator(to_engine(three_level_problem(n=6, N=4)), device=-1)
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
    rows, cols = handle.jacobian_structure()
    assert rows.size == handle.n_jacobian_entries


def test_unknown_names_are_still_refused(handle):
    with pytest.raises(dto_amd.EngineError, match="unknown option"):
        handle.set_option(OPTION + "_", 1)


def test_the_abi_version_stays_8_and_no_entry_point_was_added():
    v = int(re.search(r"#define DTO_ABI_VERSION (\d+)", H).group(1))
    assert v == dto_amd.capi.DTO_ABI_VERSION == 8
    assert int(re.search(r"const DTO_ABI_VERSION = Int32\((\d+)\)", JL).group(1)) == 8
    declared = set(re.findall(r"^\w[\w\s\*]*?\b(dto_\w+)\(", H_NOCOMMENT, flags=re.M))
    assert declared == set(dto_amd.capi.SYMBOLS), declared ^ set(dto_amd.capi.SYMBOLS)
    assert not [n for n in declared if "input" in n]
    assert sorted(n for n in declared if "reduced" in n) == ["dto_reduced_gradient", "dto_reduced_gradient_dev", "dto_reduced_hessian_product",
                                                             "dto_reduced_hessian_product_dev"]


def test_the_option_and_its_profile_name_are_documented():
    paragraph = H[H.index("Reduced-space operators"):H.index("int dto_reduced_gradient(")]
    assert '"%s" (default 0' % OPTION in paragraph
    for word in ("halving tree", "stale", "bytes"):
        assert word in paragraph, word
    assert '"reduced_input"' in H
    assert OPTION in dto_amd.Evaluator.set_option.__doc__
    assert OPTION in JL
    assert OPTION in DESIGN and "4.28" in DESIGN
