"""csrc/dto_input_plan.h from plain C++: a stand-alone program is compiled with g++ (address and undefined-behaviour sanitizers on)
against the header alone (no HIP, no engine header), run without a GPU, and prints for a list of integrator layouts every
integrator's free inputs, width and store offset and every knot component's class and terms.  Everything is compared with a Python
restatement; every non-state component is classified once, a component read by several integrators has one term per reader in list
order, the stores are disjoint and end at the sum of K 2 Wf_a x_dim_a, and an integrator without free inputs has no store and no term."""
import os
import shutil
import subprocess

import pytest

from test_elim_plan_header import B, Dv, KIND, LAYOUTS as ELIM_LAYOUTS, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
REFUSED = ("cycle", "cycle_of_three", "overlap", "own_inputs", "dt_integrated")   # the elimination plan refuses them first

# name -> (integrators, dt_idx, K, z, gd)
def _z(its, dt_idx):
    """the smallest knot that holds every component the layout names"""
    return 1 + max([dt_idx] + [max(i["x_off"] + i["x_dim"], i["in_off"] + i["in_dim"], i["t_off"] + 1) - 1 for i in its])


LAYOUTS = {name: (its, dt_idx, K, _z(its, dt_idx), 0) for name, (its, dt_idx, K) in ELIM_LAYOUTS.items() if name not in REFUSED}
# the three odd layouts of test_reduced_plan_header.py, with inputs: globals behind the knots and two integrators reading the SAME
# controls (3, 4) and the timestep, component 7 read by nobody
LAYOUTS["with_globals"] = ([B(0, 3, 3, 2), Dv(5, 2, 3)], 8, 3, 9, 3)
# list order is the reverse of the x_off order, with gaps; the middle integrator's controls are the last one's states
LAYOUTS["x_off_descending"] = ([B(7, 2, 9, 1), B(3, 4, 0, 2), B(0, 2, 2, 1)], 10, 4, 11, 0)
LAYOUTS["filler_first"] = ([B(2, 3, 0, 1)], 5, 2, 6, 2)              # the first component is no state: a control
# an integrator WITHOUT free inputs: no drives, and the timestep is another integrator's state.  (The elimination plan refuses this
# layout -- whoever integrates the timestep reads its own state -- so no handle reaches it; the header's answer is defined all the same.)
LAYOUTS["no_free_inputs"] = ([B(0, 4, 4, 0), Dv(4, 1, 5)], 4, 3, 6, 0)
LAYOUTS["time_and_step_shared"] = ([T(0, 4, 8, 2, 10), T(4, 4, 8, 2, 10)], 11, 4, 12, 0)   # controls, time and timestep read by both


def _inputs(a, dt_idx):
    s = set(range(a["in_off"], a["in_off"] + a["in_dim"])) | {dt_idx}
    if a["kind"] == "time_dependent":
        s.add(a["t_off"])
    return s


def restate(its, dt_idx, K, z):
    state = set()
    for i in its:
        state |= set(range(i["x_off"], i["x_off"] + i["x_dim"]))
    fin = [sorted(c for c in _inputs(a, dt_idx) if c not in state and 0 <= c < z) for a in its]
    width = [len(f) for f in fin]
    store = [0]
    for a, i in enumerate(its):
        store.append(store[-1] + max(K, 0) * 2 * width[a] * i["x_dim"])
    kind, terms = [], []
    for c in range(z):
        t = [(a, fin[a].index(c)) for a in range(len(its)) if c in fin[a]]
        kind.append(0 if c in state else 1 if t else 2)
        terms.append([] if c in state else t)
    return dict(fin=fin, width=width, store_off=store, kind=kind, terms=terms)


def _program():
    body = []
    for name, (its, dt_idx, K, z, _) in LAYOUTS.items():
        rows = ", ".join("ElimIntegrator{%d, %d, %d, %d, %d, %d}" % (KIND[i["kind"]], i["x_off"], i["x_dim"], i["in_off"], i["in_dim"], i["t_off"])
                         for i in its)
        body.append('    show("%s", {%s}, %d, %d, %d);' % (name, rows, dt_idx, z, K))
    return r"""
#include <cstdio>
#include "dto_input_plan.h"
using namespace dto;

static void show(const char* name, const std::vector<ElimIntegrator>& its, int dt_idx, int z, long K) {
    const InputPlan p = input_plan(its, dt_idx, z, K);
    printf("case %s\n", name);
    for (size_t a = 0; a < its.size(); ++a) {
        printf("integrator %zu width %d store %ld fin", a, p.width[a], (long)p.store_off[a]);
        for (int c : p.fin[a]) printf(" %d", c);
        printf("\n");
    }
    printf("store_end %ld\n", (long)p.store_off[its.size()]);
    for (int c = 0; c < z; ++c) {
        printf("component %d kind %d state %d terms", c, p.kind[c], input_is_state(its, c) ? 1 : 0);
        for (const InputTerm& t : p.terms[c]) printf(" %d:%d", t.a, t.j);
        printf("\n");
    }
}

int main() {
""" + "\n".join(body) + "\n    return 0;\n}\n"


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("input_plan")
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
            cur.append(line.split())
    return out


def _parse(lines):
    p = dict(fin=[], width=[], store_off=[], kind=[], terms=[], state=[], comps=[])
    for w in lines:
        if w[0] == "integrator":
            p["width"].append(int(w[3])); p["store_off"].append(int(w[5])); p["fin"].append([int(v) for v in w[7:]])
        elif w[0] == "store_end":
            p["store_off"].append(int(w[1]))
        elif w[0] == "component":
            p["comps"].append(int(w[1])); p["kind"].append(int(w[3])); p["state"].append(int(w[5]))
            p["terms"].append([tuple(int(v) for v in t.split(":")) for t in w[7:]])
    return p


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_header_and_the_restatement_agree(printed, name):
    its, dt_idx, K, z, gd = LAYOUTS[name]
    got, want = _parse(printed[name]), restate(its, dt_idx, K, z)
    for key in ("fin", "width", "store_off", "kind", "terms"):
        assert got[key] == want[key], key
    assert got["comps"] == list(range(z)), "every knot component is classified once"
    for c in range(z):
        assert (got["kind"][c] == 0) == bool(got["state"][c]), c
        assert (got["kind"][c] == 1) == bool(got["terms"][c]), c
        if got["kind"][c] == 0:
            assert not got["terms"][c], "a state is nobody's free input"
    # the terms are the transpose of the lists fin_a: each (a, j) once, j the position of the component in fin_a
    seen = sorted((a, j, c) for c in range(z) for a, j in got["terms"][c])
    assert seen == sorted((a, j, c) for a, f in enumerate(got["fin"]) for j, c in enumerate(f))
    for a, f in enumerate(got["fin"]):
        assert f == sorted(set(f)), "ascending, each component once"
    for c in range(z):
        assert [a for a, _ in got["terms"][c]] == sorted(a for a, _ in got["terms"][c]), "list order"
    # disjoint stores, one behind the other, K 2 Wf_a x_dim_a doubles each
    sizes = [max(K, 0) * 2 * got["width"][a] * its[a]["x_dim"] for a in range(len(its))]
    assert got["store_off"][0] == 0 and [b - a for a, b in zip(got["store_off"], got["store_off"][1:])] == sizes
    assert got["store_off"][-1] == sum(sizes)
    # the entries of a Z-layout vector: per knot the z components, then gd globals that no integrator reads
    n_free = sum(1 for k in got["kind"] if k != 0)
    assert n_free + sum(i["x_dim"] for i in its) == z


def test_answers_spelled_out(printed):
    bench = _parse(printed["benchmark"])     # B(0, 8, 8, 2), Dv(8, 2, 10), dt 12, K 5: the controls are the derivative's states
    assert bench["fin"] == [[12], [10, 11, 12]] and bench["width"] == [1, 3]
    assert bench["terms"][12] == [(0, 0), (1, 2)], "the timestep: one term per reader, in list order"
    assert bench["terms"][10] == [(1, 0)] and bench["terms"][8] == [] and bench["kind"][8] == 0
    assert bench["store_off"] == [0, 5 * 2 * 1 * 8, 5 * 2 * 1 * 8 + 5 * 2 * 3 * 2]
    g = _parse(printed["with_globals"])
    assert g["fin"] == [[3, 4, 8], [3, 4, 8]] and g["terms"][3] == [(0, 0), (1, 0)] and g["terms"][8] == [(0, 2), (1, 2)]
    assert g["kind"] == [0, 0, 0, 1, 1, 0, 0, 2, 1], "component 7 is read by nobody"
    d = _parse(printed["x_off_descending"])
    assert d["fin"] == [[9, 10], [10], [2, 10]] and d["terms"][10] == [(0, 1), (1, 0), (2, 1)]
    assert d["store_off"] == [0, 4 * 2 * 2 * 2, 4 * 2 * 2 * 2 + 4 * 2 * 1 * 4, 4 * 2 * 2 * 2 + 4 * 2 * 1 * 4 + 4 * 2 * 2 * 2]
    f = _parse(printed["filler_first"])
    assert f["kind"] == [1, 2, 0, 0, 0, 1] and f["terms"][0] == [(0, 0)] and f["terms"][5] == [(0, 1)]
    n = _parse(printed["no_free_inputs"])
    assert n["width"] == [0, 1] and n["fin"] == [[], [5]] and n["store_off"] == [0, 0, 3 * 2 * 1 * 1], "Wf = 0: no store, no terms"
    assert all(a != 0 for t in n["terms"] for a, _ in t)
    t = _parse(printed["t_integrated"])      # the time component is the derivative's state: no free input of the time-dependent one
    assert t["fin"][0] == [4, 5, 9] and t["kind"][8] == 0
    s = _parse(printed["time_and_step_shared"])
    assert s["fin"] == [[8, 9, 10, 11], [8, 9, 10, 11]] and s["terms"][10] == [(0, 2), (1, 2)]
    assert _parse(printed["single_knot"])["store_off"] == [0, 0, 0]
