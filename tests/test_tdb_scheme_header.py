"""csrc/dto_tdb_scheme.h from plain C++: a stand-alone program is compiled with g++ against the header alone (no HIP, no engine
header), run without a GPU, and its printed figures are checked: the pair ranking and its inverse, the parameter and table counts
at the table's limit, and the forward RK4 tableau against the adjoint tableau on a scalar linear ODE.

Tolerance of the tableau check: forward and adjoint evaluate the same step polynomial 1 + h/6 (m1 + 2 m2 + 2 m2 + m4) + ... in
different association orders, |h m| <= 1/3, three steps: a few roundings of a value near 1 each way, so 4 ulp of the result."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "dto_tdb_scheme.h"
using namespace dto;

// y' = M(tau) y on [0, 1], `steps` steps; m[3 * step + (0, 1, 2)] = M at the step's start, middle and end
static double forward(const double* m, int steps) {
    const double h = 1.0 / steps;
    double Y = 1.0, ACC = 0.0, TA = 0.0, TB = 0.0, M = 0.0;
    for (int step = 0; step < steps; ++step)
        for (int stage = 0; stage < 4; ++stage) {
            const TdbFwdStage s = tdb_fwd_stage(step, stage, h);
            const double* IN = tdb_fwd_in<const double>(stage, &Y, &TA, &TB);
            if (tdb_fwd_new_jets(stage)) M = m[3 * step + (stage == 0 ? 0 : (stage == 3 ? 2 : 1))];
            double* OUT = tdb_fwd_out(stage, &Y, &TA, &TB);
            const double K = M * *IN;
            tdb_fwd_update(stage, s.w_acc, s.w_tmp, Y, K, ACC, *OUT);
        }
    return Y;
}

// lambda(0) for lambda(1) = 1: the kernels' recursion (kbar from w and the previous ubar, ubar = M' kbar, w- = w + sum ubar)
static double backward(const double* m, int steps) {
    const double h = 1.0 / steps;
    double W = 1.0, WN, KB, UB = 0.0, M = 0.0;
    for (int step = steps - 1; step >= 0; --step) {
        WN = W;
        for (int stage = 3; stage >= 0; --stage) {
            const TdbBwdStage s = tdb_bwd_stage(step, stage, h);
            if (tdb_bwd_new_jets(stage)) M = m[3 * step + (stage == 0 ? 0 : (stage == 3 ? 2 : 1))];
            KB = tdb_bwd_kbar(s.cw, s.cu, W, UB);
            UB = M * KB;
            WN += UB;
        }
        W = WN;
    }
    return W;
}

int main(int argc, char** argv) {
    for (int p = 2; p <= 16; ++p) {
        int next = 0, ok = 1;
        for (int a = 0; a < p; ++a)
            for (int b = a; b < p; ++b, ++next) {
                int ua, ub;
                tdb_pair_unrank(next, p, &ua, &ub);
                ok &= tdb_pair_rank(a, b, p) == next && ua == a && ub == b;
            }
        printf("pairs %d %d %d %d\n", p, next, tdb_num_pairs(p), ok);
    }
    printf("counts %d %ld %d\n", tdb_num_params(7, 1), tdb_table_entries(7, 1, 4), (int)tdb_table_fits(7, 1, 4));
    printf("counts %d %ld %d\n", tdb_num_params(7, 1), tdb_table_entries(7, 1, 5), (int)tdb_table_fits(7, 1, 5));
    printf("counts %d %ld %d\n", tdb_num_params(0, 0), tdb_table_entries(0, 0, 0), (int)tdb_table_fits(0, 0, 0));
    printf("limit %d\n", TDB_MAX_COEFS);
    double m[9];
    for (int i = 0; i < 9; ++i) m[i] = atof(argv[1 + i]);
    printf("tableau %.17g %.17g\n", forward(m, 3), backward(m, 3));
    for (int i = 0; i < 9; ++i) m[i] = atof(argv[10]);
    printf("constant %.17g %.17g\n", forward(m, 3), backward(m, 3));
    return 0;
}
"""


@pytest.fixture(scope="module")
def scheme(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("tdb_scheme")
    src, exe = str(tmp / "scheme.cpp"), str(tmp / "scheme")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, src, "-o", exe], check=True)
    rng = np.random.default_rng(20)
    m = rng.uniform(-1.0, 1.0, 9)   # m1, m2, m4 of three substeps
    a = 0.7
    out = subprocess.run([exe] + [repr(float(v)) for v in m] + [repr(a)], check=True, capture_output=True, text=True).stdout
    rows = [l.split() for l in out.splitlines()]
    return {"rows": rows, "m": m, "a": a}


def _ulps(x, y):
    return abs(x - y) / np.spacing(max(abs(x), abs(y)))


def test_pair_unrank_inverts_pair_rank_in_row_major_order(scheme):
    pairs = [[int(v) for v in r[1:]] for r in scheme["rows"] if r[0] == "pairs"]
    assert [r[0] for r in pairs] == list(range(2, 17))
    for p, count, P2, ok in pairs:
        assert count == P2 == p * (p + 1) // 2 and ok == 1, (p, count, P2, ok)


def test_parameter_and_table_counts_at_the_limit(scheme):
    counts = [[int(v) for v in r[1:]] for r in scheme["rows"] if r[0] == "counts"]
    limit = [int(r[1]) for r in scheme["rows"] if r[0] == "limit"]
    assert limit == [6144]
    assert counts[0] == [16, 153 * 8 * 5, 1] and 153 * 8 * 5 == 6120   # (7, 1, 4): accepted
    assert counts[1][1:] == [7344, 0]                                   # (7, 1, 5): refused
    assert counts[2][0] == 2                                            # (0, 0, 0)


def test_forward_and_adjoint_tableau_agree(scheme):
    (fwd, bwd), = [[float(v) for v in r[1:]] for r in scheme["rows"] if r[0] == "tableau"]
    (cf, cb), = [[float(v) for v in r[1:]] for r in scheme["rows"] if r[0] == "constant"]
    # the step polynomial in the stage values, in exact-ish arithmetic (longdouble), as the yardstick of the random case
    h = np.longdouble(1) / 3
    ref = np.longdouble(1)
    for m1, m2, m4 in np.asarray(scheme["m"], dtype=np.longdouble).reshape(3, 3):
        k1 = m1
        k2 = m2 * (1 + h / 2 * k1)
        k3 = m2 * (1 + h / 2 * k2)
        k4 = m4 * (1 + h * k3)
        ref *= 1 + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    print("forward", fwd, "adjoint", bwd, "ulps", _ulps(fwd, bwd), "to reference", _ulps(fwd, float(ref)), _ulps(bwd, float(ref)))
    assert _ulps(fwd, bwd) <= 4
    assert _ulps(fwd, float(ref)) <= 4 and _ulps(bwd, float(ref)) <= 4
    ah = np.longdouble(scheme["a"]) * h
    poly = float((1 + ah + ah ** 2 / 2 + ah ** 3 / 6 + ah ** 4 / 24) ** 3)
    print("constant", cf, cb, poly, _ulps(cf, poly), _ulps(cb, poly))
    assert _ulps(cf, poly) <= 4 and _ulps(cb, poly) <= 4 and _ulps(cf, cb) <= 4
