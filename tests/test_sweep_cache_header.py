"""csrc/dto_sweep_cache.h from plain C++: a stand-alone program is compiled with g++ (address and undefined-behaviour sanitizers on)
against the header alone (no HIP, no engine header), run without a GPU, and what it prints is checked: the record is driven through
every producer's recorder, and after each one every query is answered through at(true) and through at(false).

The expected answers are written out below from the field assignments the host driver made before the record existed (seven loose
fields on BilHost: cache_kind 0..3, cache_steps, plan_q, plan_dub, p_terms, p_steps, p_nblk), each read valid only together with the
call's `same` flag:
    holds p sums = cache_kind >= 1, tangent sums = cache_kind >= 2, all terms = cache_kind == 3 (steps: cache_steps),
    p column = p_terms (steps: p_steps, nblk: p_nblk), plan = plan_q > 0 (plan_q, plan_dub)
A count that belongs to something not held is answered as 0."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "dto_sweep_cache.h"
using namespace dto;

static void show(const char* label, const SweepCache& c) {
    for (int same = 1; same >= 0; --same) {
        const auto v = c.at(same != 0);
        printf("%s %d %d %d %d %d %d %d %d %d %d %d\n", label, same, (int)v.has_p_sums(), (int)v.has_tangent_sums(), (int)v.has_all_terms(),
               v.all_terms_steps(), (int)v.has_p_column(), v.p_column_steps(), v.p_column_nblk(), (int)v.has_plan(), v.plan_rounds(),
               v.plan_budget());
    }
}

int main() {
    SweepCache c;
    show("fresh", c);
    // option on, one record carried through the producers
    c.constraint_swept(true, true, 17, 4);            show("constraint_kept_p", c);
    c.jacobian_swept_frozen();                        show("frozen_after_constraint", c);
    c.chain_planned(1, 23);                           show("chain_planned", c);
    c.jacobian_swept(true, true, 1, 19);              show("jacobian_kept_all", c);
    c.hessian_swept_p_column(true, 21, 8);            show("hessian_p_column", c);
    c.jacobian_swept_frozen();                        show("frozen_after_hessian", c);
    c.jacobian_swept(true, false, 1, 15);             show("jacobian_one_round", c);
    c.jacobian_swept(true, false, 2, 15);             show("jacobian_two_rounds", c);
    c.hessian_swept_p_column(true, 21, 8);
    c.hessian_swept_second_order();                   show("hessian_second_order", c);
    c.constraint_swept(true, false, 12, 4);           show("constraint_no_store", c);
    c.hessian_swept_p_column(true, 21, 8);
    c.products_swept();                               show("products", c);
    c.hessian_swept_p_column(true, 21, 8);
    c.constraint_swept_on_device_plan(4);             show("constraint_device_plan", c);
    c.jacobian_swept(true, true, 1, 19);
    c.invalidate();                                   show("invalidated", c);
    // option off: the same producers leave nothing to read
    SweepCache off;
    off.constraint_swept(false, false, 17, 4);        show("off_constraint", off);
    off.jacobian_swept(false, false, 1, 15);          show("off_jacobian", off);
    off.hessian_swept_p_column(false, 21, 8);         show("off_hessian_p_column", off);
    return 0;
}
"""

# label -> (p sums, tangent sums, all terms, its steps, p column, its steps, its nblk, plan, q, d_ub) with same = true
NOTHING = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
EXPECTED = [
    ("fresh",                   NOTHING),
    ("constraint_kept_p",       (1, 0, 0, 0, 1, 17, 4, 0, 0, 0)),    # kind 1; p terms with the sweep's steps and nblk
    ("frozen_after_constraint", (1, 1, 0, 0, 1, 17, 4, 0, 0, 0)),    # kind 2; the p terms stay
    ("chain_planned",           (1, 1, 0, 0, 1, 17, 4, 1, 1, 23)),
    ("jacobian_kept_all",       (1, 1, 1, 19, 0, 0, 0, 1, 1, 23)),   # kind 3, cache_steps; the store overwrote the p terms
    ("hessian_p_column",        (1, 0, 0, 0, 1, 21, 8, 1, 1, 23)),   # kind 1; p terms stored
    ("frozen_after_hessian",    (1, 1, 0, 0, 1, 21, 8, 1, 1, 23)),   # the Hessian's steps and nblk survive a frozen Jacobian
    ("jacobian_one_round",      (1, 1, 0, 0, 1, 21, 8, 1, 1, 23)),   # kind 2 without store, q = 1: the p terms stay
    ("jacobian_two_rounds",     (1, 1, 0, 0, 0, 0, 0, 1, 1, 23)),    # q > 1: the scale factors changed, p terms dropped
    ("hessian_second_order",    (0, 0, 0, 0, 0, 0, 0, 1, 1, 23)),    # kind 0, p terms dropped; the plan is not touched
    ("constraint_no_store",     (1, 0, 0, 0, 0, 0, 0, 1, 1, 23)),
    ("products",                (0, 0, 0, 0, 0, 0, 0, 1, 1, 23)),
    ("constraint_device_plan",  (0, 0, 0, 0, 0, 0, 0, 1, 1, 23)),
    ("invalidated",             NOTHING),
    ("off_constraint",          NOTHING),
    ("off_jacobian",            NOTHING),
    ("off_hessian_p_column",    NOTHING),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("sweep_cache")
    src, exe = str(tmp / "cache.cpp"), str(tmp / "cache")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        label, same, *vals = line.split()
        rows[(label, int(same))] = tuple(int(v) for v in vals)
    return rows


def test_every_producer_is_shown_with_and_without_same(answers):
    assert sorted(answers) == sorted((label, same) for label, _ in EXPECTED for same in (0, 1))


@pytest.mark.parametrize("label,expected", EXPECTED, ids=[e[0] for e in EXPECTED])
def test_answers_after_each_producer(answers, label, expected):
    print(label, "same:", answers[(label, 1)], "not same:", answers[(label, 0)])
    assert answers[(label, 1)] == expected
    assert answers[(label, 0)] == NOTHING


def test_header_includes_nothing_of_the_engine():
    with open(os.path.join(CSRC, "dto_sweep_cache.h")) as f:
        includes = [l for l in f if l.lstrip().startswith("#include")]
    assert includes == [], includes
