"""csrc/dto_reduced_plan.h from plain C++: a stand-alone program is compiled with g++ (address and undefined-behaviour sanitizers on)
against the header alone (no HIP, no engine header), run without a GPU, and prints for a list of layouts the class of every entry of
Z, the pack index of every (knot, D position), the unpack index of every state entry and the dynamics row of every (interval, D
position).  Everything is compared with a Python restatement: every entry of Z is classified exactly once, pack followed by unpack
is the identity on the states, and the rows are those of Evaluator._integrator_row0 (row0_i = (N - 1) pre_i)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_elim_plan_header import LAYOUTS as ELIM_LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
REFUSED = ("cycle", "cycle_of_three", "overlap", "own_inputs", "dt_integrated")   # no plan: the elimination plan refuses them first

# name -> ([(x_off, x_dim)] in list order, z, N, gd)
LAYOUTS = {name: ([(i["x_off"], i["x_dim"]) for i in its], dt_idx + 1, K + 1, 0)
           for name, (its, dt_idx, K) in ELIM_LAYOUTS.items() if name not in REFUSED}
LAYOUTS["with_globals"] = ([(0, 3), (5, 2)], 9, 4, 3)            # gd > 0: three entries behind the knots
LAYOUTS["x_off_descending"] = ([(7, 2), (3, 4), (0, 2)], 11, 5, 0)   # list order is the reverse of the x_off order, with gaps
LAYOUTS["filler_first"] = ([(2, 3)], 6, 3, 2)                        # the first component is no state


def restate(its, z, N, gd):
    """the same answers from NumPy"""
    K, n_vars = N - 1, N * z + gd
    pre = [sum(d for _, d in its[:i]) for i in range(len(its))]
    D = sum(d for _, d in its)
    cls = np.zeros(n_vars, dtype=int)       # 0 free, 1 state of knot 0, 2 dependent
    pos = np.full(n_vars, -1)
    knot = np.full(n_vars, N)
    unpack = np.full(n_vars, -1)
    pack = np.full((N, D), -1)
    row = np.full((max(K, 0), D), -1)
    for c in range(N * z):
        knot[c] = c // z
    for i, (x_off, x_dim) in enumerate(its):
        for k in range(N):
            for r in range(x_dim):
                c = k * z + x_off + r
                cls[c] = 1 if k == 0 else 2
                pos[c] = pre[i] + r
                unpack[c] = k * D + pre[i] + r
                pack[k, pre[i] + r] = c
                if k < K:
                    row[k, pre[i] + r] = K * pre[i] + k * x_dim + r      # _integrator_row0[i] + k x_dim + r
    return dict(D=D, cls=cls, pos=pos, knot=knot, unpack=unpack, pack=pack, row=row)


def _program():
    body = []
    for name, (its, z, N, gd) in LAYOUTS.items():
        K, pre, rows = N - 1, 0, []
        for x_off, x_dim in its:
            rows.append("ReducedIntegrator{%d, %d, %d, %d}" % (x_off, x_dim, pre, K * pre))
            pre += x_dim
        body.append('    show("%s", {%s}, %d, %d, %d);' % (name, ", ".join(rows), z, N, gd))
    return r"""
#include <cstdio>
#include "dto_reduced_plan.h"
using namespace dto;

static void show(const char* name, const std::vector<ReducedIntegrator>& its, int z, long N, int gd) {
    const ReducedPlan p = reduced_plan(its, z);
    const long n_vars = N * z + gd, K = N - 1;
    const KReduced R = reduced_view(p, z, N, n_vars, K * p.D, K * p.D);
    printf("case %s\nD %d\n", name, R.D);
    for (long c = 0; c < n_vars; ++c) {
        int states = 0;   // of how many knots is c a state?  (0 or 1)
        for (long k = 0; k <= N; ++k) states += reduced_is_state_of(R, c, k) ? 1 : 0;
        const int pos = reduced_state_pos(R, c);
        const int cls = reduced_is_dependent(R, c) ? 2 : pos >= 0 ? 1 : 0;
        printf("entry %ld %d %d %ld %ld %d\n", c, cls, pos, (long)reduced_knot(R, c), pos >= 0 ? (long)reduced_unpack_index(R, c) : -1L, states);
    }
    for (long k = 0; k < N; ++k)
        for (int d = 0; d < R.D; ++d) printf("pack %ld %d %ld\n", k, d, (long)reduced_pack_index(R, k, d));
    for (long k = 0; k < K; ++k)
        for (int d = 0; d < R.D; ++d) printf("row %ld %d %ld\n", k, d, (long)reduced_dyn_row(R, k, d));
}

int main() {
""" + "\n".join(body) + "\n    return 0;\n}\n"


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("reduced_plan")
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


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_header_and_the_restatement_agree(printed, name):
    its, z, N, gd = LAYOUTS[name]
    want = restate(its, z, N, gd)
    lines = printed[name]
    assert int(lines[0][1]) == want["D"]
    entries = [[int(v) for v in w[1:]] for w in lines if w[0] == "entry"]
    assert [e[0] for e in entries] == list(range(N * z + gd)), "every entry of Z is classified once"
    for c, cls, pos, knot, unpack, states in entries:
        assert (cls, pos, knot, unpack) == (want["cls"][c], want["pos"][c], want["knot"][c], want["unpack"][c]), c
        assert states == (1 if cls else 0), c
    pack = {(int(w[1]), int(w[2])): int(w[3]) for w in lines if w[0] == "pack"}
    assert len(pack) == N * want["D"]
    for (k, d), c in pack.items():
        assert c == want["pack"][k, d]
        assert entries[c][4] == k * want["D"] + d, "pack followed by unpack is the identity on the states"
    assert sorted(pack.values()) == [e[0] for e in entries if e[1]], "the packed entries are exactly the states, each once"
    row = {(int(w[1]), int(w[2])): int(w[3]) for w in lines if w[0] == "row"}
    assert len(row) == (N - 1) * want["D"]
    for (k, d), r in row.items():
        assert r == want["row"][k, d]
    assert sorted(row.values()) == list(range((N - 1) * want["D"])), "the dynamics rows are the first (N - 1) D rows, each once"


def test_answers_spelled_out(printed):
    lines = printed["x_off_descending"]   # integrators (7, 2), (3, 4), (0, 2): pre 0, 2, 6; z = 11, N = 5, K = 4
    entry = {int(w[1]): [int(v) for v in w[2:]] for w in lines if w[0] == "entry"}
    assert entry[7][:2] == [1, 0] and entry[3][:2] == [1, 2] and entry[0][:2] == [1, 6] and entry[2][:2] == [0, -1]
    assert entry[11 + 8][:4] == [2, 1, 1, 8 + 1], "component 8 of knot 1 is position 1, [N][D] index D + 1"
    row = {(int(w[1]), int(w[2])): int(w[3]) for w in lines if w[0] == "row"}
    assert row[(0, 0)] == 0 and row[(1, 0)] == 2 and row[(0, 2)] == 4 * 2 and row[(3, 7)] == 4 * 6 + 3 * 2 + 1
    glob = {int(w[1]): [int(v) for v in w[2:]] for w in printed["with_globals"] if w[0] == "entry"}
    assert all(glob[c][:3] == [0, -1, 4] for c in (36, 37, 38)), "globals are free and belong to no knot"
