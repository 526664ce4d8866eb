"""csrc/dto_feasible_plan.h from plain C++: a stand-alone program (its own main) is compiled with g++ (address and undefined-behaviour
sanitizers on) against the plan headers alone (no HIP, no engine header) and run without a GPU.  For a list of integrator layouts it
takes the levels from dto_elim_plan.h, builds the schedule of the feasible-trajectory rollout, checks its invariants itself (a
failed check ends it with a non-zero status) and prints the steps, which are compared with a restatement here and spelled out by hand
for the list order [ket, (u, du), ket, (du, ddu)] of three_level_problem."""
import os
import shutil
import subprocess

import pytest

from elim_cases import plan
from test_elim_plan_header import KIND, B, Dv, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")

# name -> (integrators, dt_idx)
LAYOUTS = {
    "three_level": ([B(0, 4, 8, 2), Dv(8, 2, 10), B(4, 4, 8, 2), Dv(10, 2, 12)], 14),     # levels 2, 1, 2, 0
    "benchmark": ([B(0, 8, 8, 2), Dv(8, 2, 10)], 12),
    "between": ([B(0, 3, 6, 2), Dv(6, 2, 8), B(3, 3, 6, 2)], 10),                        # two kets on one level
    "derivatives_only": ([Dv(0, 70, 70)], 140),
    "derivative_chain": ([Dv(0, 2, 2), Dv(2, 2, 4)], 6),                                  # (u, du) before (du, ddu)
    "level_zero_mix": ([B(0, 4, 4, 0), Dv(4, 2, 6), T(8, 4, 12, 2, 14)], 15),             # a ket without drives beside a derivative
    "none": ([], 0),
}

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "dto_elim_plan.h"
#include "dto_feasible_plan.h"
using namespace dto;

#define REQUIRE(c) do { if (!(c)) { printf("FAILED %s: %s\n", name, #c); exit(1); } } while (0)

static void show(const char* name, const std::vector<ElimIntegrator>& its, int dt_idx) {
    const ElimPlan e = elim_plan(its, dt_idx, 5);
    REQUIRE(e.refusal.empty());
    std::vector<int> prop;
    for (const ElimIntegrator& it : its) prop.push_back(it.kind != ELIM_DERIVATIVE);
    const FeasiblePlan p = feasible_plan(e.level, prop);
    printf("case %s\n", name);
    const int I = (int)its.size();
    std::vector<int> seen(I, 0), jac_of_level(e.n_levels, 0), prop_of_level(e.n_levels, 0);
    int last_level = -1, n_jac = 0, n_deriv = 0, n_roll = 0;
    for (const FeasibleStep& s : p.steps) {
        printf("step %d %d %d\n", s.kind, s.integrator, s.level);
        REQUIRE(s.level >= last_level);          // levels ascending
        last_level = s.level;
        if (s.kind == FEAS_JACOBIAN) {
            REQUIRE(s.integrator == -1);
            REQUIRE(jac_of_level[s.level] == 0);  // one per level
            jac_of_level[s.level] = 1;
            ++n_jac;
            continue;
        }
        REQUIRE(s.integrator >= 0 && s.integrator < I);
        REQUIRE(e.level[s.integrator] == s.level);
        REQUIRE(seen[s.integrator] == 0);         // every integrator once
        seen[s.integrator] = 1;
        if (s.kind == FEAS_ROLL) {
            REQUIRE(prop[s.integrator]);
            REQUIRE(jac_of_level[s.level] == 1);  // preceded by the JACOBIAN of its level
            ++n_roll;
        } else {
            REQUIRE(s.kind == FEAS_DERIV);
            REQUIRE(!prop[s.integrator]);
            REQUIRE(jac_of_level[s.level] == 0);  // the derivatives of a level run before its Jacobian
            ++n_deriv;
        }
    }
    for (int i = 0; i < I; ++i) {
        REQUIRE(seen[i] == 1);
        if (prop[i]) prop_of_level[e.level[i]] = 1;
    }
    for (int l = 0; l < e.n_levels; ++l) REQUIRE(jac_of_level[l] == prop_of_level[l]);   // exactly the levels that hold a propagator
    REQUIRE(n_jac == p.n_jacobians && n_deriv == p.n_deriv && n_roll == p.n_roll);
    printf("counts %d %d %d\n", p.n_jacobians, p.n_deriv, p.n_roll);
}

int main() {
@BODY@
    return 0;
}
"""


def _program():
    body = []
    for name, (its, dt_idx) in LAYOUTS.items():
        rows = ", ".join("ElimIntegrator{%d, %d, %d, %d, %d, %d}" % (KIND[i["kind"]], i["x_off"], i["x_dim"], i["in_off"], i["in_dim"], i["t_off"])
                         for i in its)
        body.append('    show("%s", {%s}, %d);' % (name, rows, dt_idx))
    return PROGRAM.replace("@BODY@", "\n".join(body))


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("feasible_plan")
    src, exe = str(tmp / "plan.cpp"), str(tmp / "plan")
    with open(src, "w") as f:
        f.write(_program())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out, cur = {}, None
    for line in run.stdout.splitlines():
        if line.startswith("case "):
            cur = out.setdefault(line[5:], dict(steps=[], counts=None))
        elif line.startswith("step "):
            cur["steps"].append(tuple(int(v) for v in line.split()[1:]))
        elif line.startswith("counts "):
            cur["counts"] = tuple(int(v) for v in line.split()[1:])
    return out


DERIV, JACOBIAN, ROLL = 0, 1, 2


def restated(its, dt_idx):
    """the schedule from elim_cases.plan's levels, as the header's comment states it"""
    level = plan(its, dt_idx, 5)["level"] if its else []
    steps = []
    for lv in range(max(level, default=-1) + 1):
        here = [i for i in range(len(its)) if level[i] == lv]
        steps += [(DERIV, i, lv) for i in here if its[i]["kind"] == "derivative"]
        rolls = [(ROLL, i, lv) for i in here if its[i]["kind"] != "derivative"]
        if rolls:
            steps += [(JACOBIAN, -1, lv)] + rolls
    return steps


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_header_and_the_restatement_agree(printed, name):
    its, dt_idx = LAYOUTS[name]
    want = restated(its, dt_idx)
    assert printed[name]["steps"] == want
    assert printed[name]["counts"] == tuple(sum(1 for s in want if s[0] == k) for k in (JACOBIAN, DERIV, ROLL))


def test_answers_spelled_out(printed):
    # list order [ket, (u, du), ket, (du, ddu)]: levels 2, 1, 2, 0 -- both kets behind ONE Jacobian
    assert printed["three_level"]["steps"] == [(DERIV, 3, 0), (DERIV, 1, 1), (JACOBIAN, -1, 2), (ROLL, 0, 2), (ROLL, 2, 2)]
    assert printed["three_level"]["counts"] == (1, 2, 2)
    assert printed["benchmark"]["steps"] == [(DERIV, 1, 0), (JACOBIAN, -1, 1), (ROLL, 0, 1)]
    assert printed["between"]["counts"] == (1, 1, 2), "two kets on one level share one Jacobian evaluation"
    assert printed["derivatives_only"]["steps"] == [(DERIV, 0, 0)] and printed["derivatives_only"]["counts"] == (0, 1, 0)
    assert printed["derivative_chain"]["steps"] == [(DERIV, 1, 0), (DERIV, 0, 1)], "list order is not dependency order"
    assert printed["level_zero_mix"]["steps"] == [(DERIV, 1, 0), (JACOBIAN, -1, 0), (ROLL, 0, 0), (ROLL, 2, 0)]
    assert printed["none"]["steps"] == [] and printed["none"]["counts"] == (0, 0, 0)
