"""csrc/dto_elim_plan.h from plain C++: a stand-alone program is compiled with g++ (address and undefined-behaviour sanitizers on)
against the header alone (no HIP, no engine header), run without a GPU, and prints for a list of integrator layouts the refusal or the
levels, the processing order, the dependencies with their column offsets, the dependents, the widths and the offsets of the compact
coupling store.  Everything is compared with the Python restatement in elim_cases.py, and a few answers are spelled out by hand."""
import os
import shutil
import subprocess

import pytest

from elim_cases import plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
KIND = {"bilinear": 0, "derivative": 1, "time_dependent": 2}


def B(x_off, x_dim, u_off, u_dim):
    return dict(kind="bilinear", x_off=x_off, x_dim=x_dim, in_off=u_off, in_dim=u_dim, t_off=-1)


def Dv(x_off, x_dim, xdot_off):
    return dict(kind="derivative", x_off=x_off, x_dim=x_dim, in_off=xdot_off, in_dim=x_dim, t_off=-1)


def T(x_off, x_dim, u_off, u_dim, t_off):
    return dict(kind="time_dependent", x_off=x_off, x_dim=x_dim, in_off=u_off, in_dim=u_dim, t_off=t_off)


# name -> (integrators, dt_idx, K)
LAYOUTS = {
    "benchmark": ([B(0, 8, 8, 2), Dv(8, 2, 10)], 12, 5),
    "single": ([B(0, 5, 5, 2)], 7, 3),
    "derivative_first": ([Dv(8, 2, 10), B(0, 8, 8, 2)], 12, 4),
    "three_levels_mixed": ([B(0, 4, 8, 2), Dv(8, 2, 10), B(4, 4, 8, 2), Dv(10, 2, 12)], 14, 6),
    "between": ([B(0, 3, 6, 2), Dv(6, 2, 8), B(3, 3, 6, 2)], 10, 2),
    "time_dependent_chain": ([T(0, 4, 4, 2, 8), Dv(4, 2, 6)], 9, 5),
    "t_integrated": ([T(0, 4, 4, 2, 8), Dv(8, 1, 6)], 9, 5),            # the time component is somebody's state
    "dt_integrated": ([B(0, 4, 4, 2), Dv(7, 1, 6)], 7, 5),              # ... and the timestep: that integrator reads its own state
    "unread_state": ([B(0, 4, 4, 2), Dv(6, 1, 8)], 7, 5),               # a state nobody reads: two level-0 integrators
    "no_drives": ([B(0, 4, 4, 0), Dv(4, 2, 6)], 8, 3),
    "cycle": ([Dv(0, 2, 2), Dv(2, 2, 0)], 4, 3),
    "cycle_of_three": ([B(0, 3, 3, 2), Dv(3, 2, 5), Dv(5, 2, 0)], 8, 3),
    "overlap": ([B(0, 4, 6, 2), B(3, 4, 6, 2)], 8, 3),
    "own_inputs": ([B(0, 4, 3, 2)], 6, 3),
    "single_knot": ([B(0, 8, 8, 2), Dv(8, 2, 10)], 12, 0),
}


def _program():
    body = []
    for name, (its, dt_idx, K) in LAYOUTS.items():
        rows = ", ".join("ElimIntegrator{%d, %d, %d, %d, %d, %d}" % (KIND[i["kind"]], i["x_off"], i["x_dim"], i["in_off"], i["in_dim"], i["t_off"])
                         for i in its)
        body.append('    show("%s", {%s}, %d, %d);' % (name, rows, dt_idx, K))
    return r"""
#include <cstdio>
#include "dto_elim_plan.h"
using namespace dto;

static void show(const char* name, const std::vector<ElimIntegrator>& its, int dt_idx, long K) {
    const ElimPlan p = elim_plan(its, dt_idx, K);
    printf("case %s\n", name);
    if (!p.refusal.empty()) { printf("refusal %s\n", p.refusal.c_str()); return; }
    printf("sizes %d %d\n", p.n_states, p.n_levels);
    for (size_t a = 0; a < its.size(); ++a) {
        printf("integrator %zu pre %d level %d width %d store %ld deps", a, p.pre[a], p.level[a], p.width[a], (long)p.store_off[a]);
        for (const ElimDep& d : p.deps[a]) printf(" %d:%d", d.b, d.col);
        printf(" dependents");
        for (int b : p.dependents[a]) printf(" %d", b);
        printf("\n");
    }
    printf("order");
    for (int a : p.order) printf(" %d", a);
    printf("\nstore_end %ld\n", (long)p.store_off[its.size()]);
    printf("pos %ld %ld\n", (long)elim_interval_doubles(3, 5), (long)elim_block_pos(3, 5, 2, 1, 2));
}

int main() {
""" + "\n".join(body) + "\n    return 0;\n}\n"


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("elim_plan")
    src, exe = str(tmp / "plan.cpp"), str(tmp / "plan")
    with open(src, "w") as f:
        f.write(_program())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    out, cur = {}, None
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        if line.startswith("case "):
            cur = out.setdefault(line[5:], [])
        else:
            cur.append(line)
    return out


def _parse(lines):
    if lines[0].startswith("refusal "):
        return dict(refusal=lines[0][8:])
    p = dict(refusal=None, pre=[], level=[], width=[], store_off=[], deps=[], dependents=[])
    p["n_states"], p["n_levels"] = (int(v) for v in lines[0].split()[1:])
    for l in lines:
        w = l.split()
        if w[0] == "integrator":
            p["pre"].append(int(w[3])); p["level"].append(int(w[5])); p["width"].append(int(w[7])); p["store_off"].append(int(w[9]))
            i = w.index("dependents")
            p["deps"].append([tuple(int(v) for v in d.split(":")) for d in w[11:i]])
            p["dependents"].append([int(v) for v in w[i + 1:]])
        elif w[0] == "order":
            p["order"] = [int(v) for v in w[1:]]
        elif w[0] == "store_end":
            p["store_off"].append(int(w[1]))
        elif w[0] == "pos":
            p["pos"] = (int(w[1]), int(w[2]))
    return p


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_header_and_the_restatement_agree(printed, name):
    its, dt_idx, K = LAYOUTS[name]
    got, want = _parse(printed[name]), plan(its, dt_idx, K)
    assert got["refusal"] == want["refusal"]
    if want["refusal"] is None:
        for key in ("n_states", "n_levels", "pre", "level", "order", "deps", "dependents", "width", "store_off"):
            assert got[key] == want[key], key
        assert got["pos"] == (2 * 3 * 5, (2 * 2 + 1) * 3 * 5 + 2 * 5)


def test_answers_spelled_out(printed):
    bench = _parse(printed["benchmark"])
    assert bench["level"] == [1, 0] and bench["order"] == [1, 0], "list order is not dependency order"
    assert bench["deps"] == [[(1, 0)], []] and bench["dependents"] == [[], [0]]
    assert bench["store_off"] == [0, 5 * 2 * 2 * 8, 5 * 2 * 2 * 8]
    mixed = _parse(printed["three_levels_mixed"])
    assert mixed["level"] == [2, 1, 2, 0] and mixed["n_levels"] == 3 and mixed["order"] == [3, 1, 0, 2]
    assert mixed["dependents"][1] == [0, 2] and mixed["pre"] == [0, 4, 6, 10] and mixed["n_states"] == 12
    assert _parse(printed["between"])["order"] == [1, 0, 2]
    t = _parse(printed["t_integrated"])
    assert t["deps"][0] == [(1, 0)] and t["level"] == [1, 0], "the time component is an input of the time-dependent kind"
    assert _parse(printed["unread_state"])["level"] == [0, 0]
    assert _parse(printed["no_drives"])["level"] == [0, 0]
    assert _parse(printed["single_knot"])["store_off"] == [0, 0, 0]


@pytest.mark.parametrize("name,text", [("cycle", "depend on each other in a cycle"), ("cycle_of_three", "depend on each other in a cycle"),
                                       ("overlap", "the states of integrators 0 and 1 overlap"),
                                       ("own_inputs", "the inputs of integrator 0 meet its own states"),
                                       ("dt_integrated", "the inputs of integrator 1 meet its own states")])
def test_refusals(printed, name, text):
    assert text in _parse(printed[name])["refusal"]
