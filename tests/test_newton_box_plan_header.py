"""csrc/dto_newton_box_plan.h from plain C++: a stand-alone program (its own main) is compiled with g++ (address and undefined-behaviour
sanitizers on) against the header alone and run without a GPU.  It runs the header's entry rules (newton_box_classify,
newton_box_breakpoint, newton_box_update, newton_box_point, newton_box_direction), its decision (newton_box_decide), its tree of minima
and its whole loop (newton_box_solve, on a dense symmetric matrix of 300 entries: two chunks, the second ragged) and prints the bits,
which are compared with the restatements in NumPy of newton_box_cases.py -- what include/dto_engine.h, "Bound-constrained truncated-Newton
step", states.  The dot order, the decision of the unbounded step and the halving tree are test_newton_plan_header.py's restatements."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import newton_box_cases as B
from test_newton_plan_header import BOUNDARY, CONTINUE, CONVERGED, MAX_ITER, NEG_CURVATURE, NOT_FINITE, decide_restated, grid, lanes, tree64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
INF, NAN = math.inf, math.nan
N_LOOP = 300

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dto_newton_box_plan.h"
using namespace dto;

static unsigned long long bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }
static void must_read(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { printf("FAILED short file\n"); exit(1); } }
static long long count_of(FILE* f) { long long n = 0; must_read(&n, 8, f); return n; }
static void print_vector(const char* what, const std::vector<double>& v) {
    printf("%s", what);
    for (double x : v) printf(" %016llx", bits(x));
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    for (long long c = count_of(f); c > 0; --c) {
        double v[8];
        must_read(v, sizeof v, f);
        const NewtonDecision D = newton_box_decide(v[0], v[1], v[2], v[3], v[4], v[5], v[6], (int)v[7]);
        printf("decide %d %016llx\n", D.status, bits(D.s));
    }
    for (long long c = count_of(f); c > 0; --c) {
        double v[5];
        must_read(v, sizeof v, f);
        printf("breakpoint %016llx\n", bits(newton_box_breakpoint(v[0], v[1], v[2], v[3], v[4])));
    }
    for (long long c = count_of(f); c > 0; --c) {
        double v[4];
        must_read(v, sizeof v, f);
        printf("classify %d\n", newton_box_classify(v[0], v[1], v[2], v[3]));
    }
    for (long long c = count_of(f); c > 0; --c) {   // state, z, lo, hi, d, w, s, t, p, r
        double v[10];
        must_read(v, sizeof v, f);
        double p = v[8], r = v[9];
        const int s = newton_box_update((int)v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], &p, &r);
        printf("update %d %016llx %016llx %016llx\n", s, bits(p), bits(r), bits(newton_box_point(s, v[1], p, v[2], v[3])));
    }
    for (long long c = count_of(f); c > 0; --c) {
        double a[64];
        must_read(a, sizeof a, f);
        double m = newton_box_inf();
        for (int l = 0; l < 64; ++l) m = newton_box_min(m, a[l]);
        for (int l = 0; l < 64; ++l) a[l] = newton_box_min(newton_box_inf(), a[l]);   // a lane's minimum starts from +inf: it never holds a NaN
        printf("mintree %016llx %016llx\n", bits(newton_box_mintree64(a)), bits(m));
    }
    for (long long c = count_of(f); c > 0; --c) {   // state, restart, beta, d, r
        double v[5];
        must_read(v, sizeof v, f);
        printf("direction %016llx\n", bits(newton_box_direction((int)v[0], v[1] != 0.0, v[2], v[3], v[4])));
    }
    const long long n = count_of(f);
    std::vector<double> A((size_t)(n * n)), Z((size_t)n), g((size_t)n), fx((size_t)n);
    must_read(A.data(), 8 * A.size(), f);
    must_read(Z.data(), 8 * Z.size(), f);
    must_read(g.data(), 8 * g.size(), f);
    must_read(fx.data(), 8 * fx.size(), f);
    std::vector<unsigned char> fixed((size_t)n);
    for (long long i = 0; i < n; ++i) fixed[(size_t)i] = fx[(size_t)i] != 0.0;
    std::vector<double> P((size_t)newton_chunks(n));
    auto apply = [&](const double* d, double* y) {   // every row in the dot's own order, so that NumPy can state it again
        for (long long i = 0; i < n; ++i) y[i] = newton_dot(A.data() + (size_t)(i * n), d, n, P.data());
    };
    for (long long c = count_of(f); c > 0; --c) {
        double k[7];   // has_lo, has_hi, radius, shift, rtol, atol, max_iter
        must_read(k, sizeof k, f);
        std::vector<double> lo((size_t)n), hi((size_t)n);
        must_read(lo.data(), 8 * lo.size(), f);
        must_read(hi.data(), 8 * hi.size(), f);
        const int max_iter = (int)k[6];
        std::vector<double> p((size_t)n), info(NEWTON_BOX_INFO), trace((size_t)(NEWTON_BOX_TRACE * max_iter), -7.0), es((size_t)n), zp((size_t)n);
        newton_box_solve(n, Z.data(), g.data(), fixed.data(), k[0] != 0.0 ? lo.data() : nullptr, k[1] != 0.0 ? hi.data() : nullptr, k[2], k[3],
                         k[4], k[5], max_iter, apply, p.data(), info.data(), trace.data(), es.data(), zp.data());
        print_vector("loop_p", p);
        print_vector("loop_info", info);
        print_vector("loop_trace", trace);
        print_vector("loop_states", es);
        print_vector("loop_zp", zp);
        double i2[NEWTON_BOX_INFO];   // the optional outputs left out: the same step
        std::vector<double> p2((size_t)n);
        newton_box_solve(n, Z.data(), g.data(), fixed.data(), k[0] != 0.0 ? lo.data() : nullptr, k[1] != 0.0 ? hi.data() : nullptr, k[2], k[3],
                         k[4], k[5], max_iter, apply, p2.data(), i2, nullptr, nullptr, nullptr);
        printf("loop_again %d\n", memcmp(p2.data(), p.data(), 8 * p.size()) == 0 && memcmp(i2, info.data(), sizeof i2) == 0 ? 1 : 0);
    }
    fclose(f);
    printf("sizes %d %d %d %d %lld\n", NEWTON_BOX_SLOTS, NEWTON_BOX_STATE, NEWTON_BOX_INFO, NEWTON_BOX_TRACE, (long long)newton_box_workspace_doubles(11610));
    printf("codes %d %d %d %d %d %d\n", NBOX_FIXED, NBOX_FREE, NBOX_HELD_LO, NBOX_HELD_HI, NBOX_HIT_LO, NBOX_HIT_HI);
    return 0;
}
"""


# ---------------------------------------------------------------------------------------------------------------- the grids
def decide_grid():
    """the unbounded step's grid under tau_box = 0, finite values (one of them the unbounded s itself) and +inf; NaN / inf inputs are in
    the grid already, a NaN tau_box is added"""
    rows = []
    for row in grid():
        _, s0 = decide_restated(*row[:6], int(row[6]))
        taus = [0.0, 0.25, 1.0, 1e3, INF]
        if math.isfinite(s0) and s0 > 0:
            taus += [s0, float(np.nextafter(s0, 0.0)), float(np.nextafter(s0, INF))]     # s0 == tau_box, and one ulp to either side
        for tau_box in taus:
            rows.append(row[:6] + (tau_box, row[6]))
    rows.append((1.0, 1.0, 0.0, 0.0, 4.0, 0.0, NAN, 2.0))
    rows.append((-1.0, 1.0, 0.0, 0.0, 4.0, 0.0, NAN, 1.0))
    return rows


def breakpoint_grid():
    rows = []
    for z, p in ((0.3, 0.0), (0.3, 0.2), (-1.0, 0.5), (0.0, 0.0)):
        for d in (0.0, -0.0, 0.7, -0.7, 1e-300, -1e300, INF, NAN):
            for lo, hi in ((-INF, INF), (-1.0, 1.0), (0.3, 0.5), (0.5, 0.5), (0.9, 0.1), (NAN, NAN), (-INF, 0.5), (0.5, INF)):
                rows.append((z, p, d, lo, hi))
    rows.append((INF, 0.0, 1.0, -INF, INF))         # inf - inf: a NaN, which is skipped
    rows.append((0.5, 0.0, 1.0, -INF, 0.5))         # on the bound: t = 0
    rows.append((0.5, 0.0, -1.0, 0.5, INF))         # (0.5 - 0.5) / -1 = -0: returned as +0
    return rows


def classify_grid():
    return [(z, lo, hi, g) for z in (0.0, 0.5, 1.0, 1.5, NAN) for lo, hi in ((0.5, 1.0), (-INF, INF), (1.0, 1.0), (1.5, 0.0), (NAN, NAN))
            for g in (-2.0, -0.0, 0.0, 3.0, NAN)]


def update_grid():
    rows = []
    for state in (B.FIXED, B.FREE, B.HELD_LO, B.HELD_HI, B.HIT_LO, B.HIT_HI):
        for z, lo, hi in ((0.2, -1.0, 1.0), (0.2, -INF, INF), (0.2, 0.2, 0.2), (0.2, 0.3, 0.1)):
            for d in (0.0, 0.8, -0.8):
                for s in (0.0, 0.5, 1.0, 1.5, 4.0, INF):
                    for p in (0.0, 0.3):
                        t = B.breakpoints_restated(np.array([z]), np.array([p]), np.array([d]), np.array([lo]), np.array([hi]),
                                                   np.array([True]))[0]
                        rows.append((float(state), z, lo, hi, d, 0.7, s, float(t), p, -0.4))
    # the clamp by the second condition: t a shade above s, but the rounded Z + p reaches the bound
    rows.append((1.0, 0.1, -INF, 0.3, 0.2, 0.0, 1.0, float(np.nextafter(1.0, 2.0)), 0.0, 0.0))
    rows.append((1.0, 0.1, -INF, 0.3, 0.2, 0.0, 1.0, NAN, 0.0, 0.0))
    return rows


def min_grid():
    rng = np.random.default_rng(9)
    rows = [rng.random(64) * 10.0 ** rng.integers(-3, 4, 64) for _ in range(4)]
    rows[1][rng.integers(0, 64, 20)] = NAN
    rows[2][:] = INF
    rows[3][:] = NAN
    rows[3][17] = 2.5
    rows.append(np.full(64, NAN))
    rows.append(np.concatenate([np.full(63, INF), [0.0]]))
    return rows


def direction_grid():
    return [(float(s), float(restart), beta, d, r) for s in range(6) for restart in (0, 1) for beta in (0.0, 0.37) for d, r in ((0.0, 0.0), (-0.0, 0.0), (0.6, -1.1))]


# ----------------------------------------------------------------------------------------------------------------- the loop
def loop_problem():
    rng = np.random.default_rng(300)
    n = N_LOOP
    A = rng.standard_normal((n, n))
    A = 0.5 * (A + A.T) / math.sqrt(n)        # eigenvalues in about -1.4 .. 1.4: indefinite
    Z, g = rng.standard_normal(n), rng.standard_normal(n)
    fixed = np.zeros(n)
    fixed[rng.choice(n, 40, replace=False)] = 1.0
    return A, Z, g, fixed


def loop_runs():
    """(has_lo, has_hi, radius, shift, rtol, atol, max_iter, lo, hi)"""
    A, Z, g, fixed = loop_problem()
    n = N_LOOP
    rng = np.random.default_rng(301)
    none = (np.full(n, -INF), np.full(n, INF))
    wide = (Z - 0.05 - rng.random(n), Z + 0.05 + rng.random(n))
    on = (Z - 0.3, Z + 0.3)
    on[0][:20], on[1][20:40] = Z[:20], Z[20:40]         # entries ON a bound: held or free by the sign of g
    return [
        (0, 0, 0.0, 3.0, 1e-8, 0.0, 40) + none,          # no bounds, convex
        (1, 1, 0.0, 3.0, 1e-8, 0.0, 80) + wide,          # convex, a box that is hit: restarts
        (1, 1, 0.0, 3.0, 1e-8, 0.0, 3) + wide,           # MAX_ITER
        (1, 1, 0.0, 0.0, 1e-8, 0.0, 80) + wide,          # indefinite, no radius: along d to a face, and on
        (1, 1, 1.0, 0.0, 1e-8, 0.0, 80) + wide,          # indefinite with a radius
        (1, 0, 0.0, 3.0, 1e-8, 0.0, 80) + on,            # lower bounds only, entries held from the start
        (0, 1, 0.5, 3.0, 1e-8, 0.0, 80) + on,            # upper bounds only, a radius
        (1, 1, 0.0, 3.0, 1e-8, 0.0, 80, Z.copy(), Z.copy()),   # lo = hi = Z: every step has length 0
    ]


def rows_dot(A, d):
    """y_i = the dot of row i with d in the stated order: what the program's `apply` computes"""
    rows, n = A.shape
    nb = -(-n // 256)
    a = np.zeros((rows, nb * 256))
    a[:, :n] = A * d[None, :]
    a = a.reshape(rows, nb, 4, 64)
    lane = np.zeros((rows, nb, 64))
    for t in range(4):
        lane = lane + a[:, :, t]
    P = np.zeros((rows, 64))
    P[:, :nb] = tree64(lane)
    return tree64(P)


def test_the_row_products_follow_the_dots_order():
    A, Z, g, _ = loop_problem()
    y = rows_dot(A[:3], g)
    for i in range(3):
        assert y[i] == B.dot(A[i], g)
    assert nb_of(N_LOOP) == 2 and N_LOOP % 256 != 0


def nb_of(n):
    return -(-n // 256)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("newton_box_plan")
    src, exe, data = str(tmp / "plan.cpp"), str(tmp / "plan"), str(tmp / "data.bin")
    with open(src, "w") as f:
        f.write(PROGRAM)
    A, Z, g, fixed = loop_problem()
    with open(data, "wb") as f:
        for rows in (decide_grid(), breakpoint_grid(), classify_grid(), update_grid(), min_grid(), direction_grid()):
            f.write(struct.pack("q", len(rows)) + np.array(rows, dtype=np.float64).tobytes())
        f.write(struct.pack("q", N_LOOP) + A.tobytes() + Z.tobytes() + g.tobytes() + fixed.tobytes())
        runs = loop_runs()
        f.write(struct.pack("q", len(runs)))
        for run in runs:
            f.write(np.array(run[:7], dtype=np.float64).tobytes() + run[7].tobytes() + run[8].tobytes())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe], check=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    out = {}
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] in ("sizes", "codes"):
            out[w[0]] = tuple(int(v) for v in w[1:])
        elif w[0].startswith("loop_") and w[0] != "loop_again":
            out.setdefault(w[0], []).append(np.array([int(v, 16) for v in w[1:]], dtype=np.uint64).view(np.float64))
        else:
            out.setdefault(w[0], []).append(w[1:])
    return out


def _bits(x):
    return struct.unpack("Q", struct.pack("d", x))[0]


def same(got_hex, want):
    got = struct.unpack("d", struct.pack("Q", int(got_hex, 16)))[0]
    return (math.isnan(got) and math.isnan(want)) or int(got_hex, 16) == _bits(float(want))


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_newton_box_decide_agrees_with_the_rule_on_the_grid(printed):
    g = decide_grid()
    assert len(printed["decide"]) == len(g)
    seen = set()
    for row, (status, sbits) in zip(g, printed["decide"]):
        want_status, want_s = B.box_decide_restated(*row[:7], int(row[7]))
        assert int(status) == want_status and same(sbits, want_s), (row, status, want_status, want_s)
        st0, s0 = decide_restated(*row[:6], int(row[7]))
        seen.add((st0, row[5] > 0, "cut" if (want_status, want_s) != (st0, s0) and not (math.isnan(s0) and math.isnan(want_s)) else "kept",
                  "zero" if row[6] == 0 else "finite" if math.isfinite(row[6]) else "inf"))
    # every branch: NOT_FINITE passes through; non-positive curvature without a radius goes to a finite face and stays as it is without
    # one; a longer step is cut at the face whatever its status; a shorter one is kept
    assert (NOT_FINITE, False, "kept", "zero") in seen and (NOT_FINITE, True, "kept", "finite") in seen
    assert (NEG_CURVATURE, False, "cut", "finite") in seen and (NEG_CURVATURE, False, "cut", "zero") in seen
    assert (NEG_CURVATURE, False, "kept", "inf") in seen
    assert (NEG_CURVATURE, True, "cut", "finite") in seen and (NEG_CURVATURE, True, "kept", "inf") in seen
    assert (BOUNDARY, True, "cut", "finite") in seen and (BOUNDARY, True, "kept", "finite") in seen
    assert (CONTINUE, False, "cut", "zero") in seen and (CONTINUE, False, "kept", "finite") in seen and (CONTINUE, True, "kept", "inf") in seen


def test_decisions_spelled_out(printed):
    ans = dict(zip(decide_grid(), printed["decide"]))
    hexs = lambda x: f"{_bits(x):016x}"
    # kappa = 3.7, rr = 1.3: alpha = 1.3 / 3.7.  tau_box == alpha keeps the CG step (not >), one ulp less cuts it
    alpha = 1.3 / 3.7
    row = (3.7, 1.0, 0.0, 0.0, 1.3, 0.0)
    assert ans[row + (alpha, 1.0)] == [str(CONTINUE), hexs(alpha)]
    below = float(np.nextafter(alpha, 0.0))
    assert ans[row + (below, 1.0)] == [str(CONTINUE), hexs(below)]
    assert ans[row + (0.0, 1.0)] == [str(CONTINUE), hexs(0.0)], "a step of length 0 is legal"
    # kappa = -2.5 without a radius: to the face at 0.25 and on; without a face the unbounded rule (d in iteration 1, nothing later)
    neg = (-2.5, 1.0, 0.0, 0.0, 1.3, 0.0)
    assert ans[neg + (0.25, 5.0)] == [str(CONTINUE), hexs(0.25)]
    assert ans[neg + (INF, 1.0)] == [str(NEG_CURVATURE), hexs(1.0)] and ans[neg + (INF, 5.0)] == [str(NEG_CURVATURE), hexs(0.0)]
    # with a radius of 2: tau = 2; the face at 0.25 is nearer (goes on), the face at 1e3 is further (NEG_CURVATURE at the radius)
    negr = (-2.5, 1.0, 0.0, 0.0, 1.3, 2.0)
    assert ans[negr + (0.25, 5.0)] == [str(CONTINUE), hexs(0.25)] and ans[negr + (1e3, 5.0)] == [str(NEG_CURVATURE), hexs(2.0)]
    assert ans[(math.nan, 1.0, 0.0, 0.0, 1.3, 0.0, 0.25, 1.0)][0] == str(NOT_FINITE)
    assert ans[(1.0, 1.0, 0.0, 0.0, 4.0, 0.0, NAN, 2.0)] == [str(CONTINUE), hexs(4.0)], "a NaN tau_box cuts nothing"
    assert ans[(-1.0, 1.0, 0.0, 0.0, 4.0, 0.0, NAN, 1.0)] == [str(NEG_CURVATURE), hexs(1.0)]


def test_the_breakpoint_expression(printed):
    g = breakpoint_grid()
    assert len(printed["breakpoint"]) == len(g)
    for row, (tbits,) in zip(g, printed["breakpoint"]):
        z, p, d, lo, hi = (np.array([v]) for v in row)
        want = B.breakpoints_restated(z, p, d, lo, hi, np.array([True]))[0]
        assert same(tbits, want), (row, tbits, want)
    ans = dict(zip(g, (b[0] for b in printed["breakpoint"])))
    assert ans[(0.5, 0.0, -1.0, 0.5, INF)] == f"{_bits(0.0):016x}" and ans[(0.5, 0.0, 1.0, -INF, 0.5)] == f"{_bits(0.0):016x}"
    assert ans[(0.3, 0.2, 0.7, 0.3, 0.5)] == f"{_bits(0.0):016x}", "already on the bound: max(0, .)"
    assert ans[(0.3, 0.0, 0.7, -1.0, 1.0)] == f"{_bits((1.0 - (0.3 + 0.0)) / 0.7):016x}"
    assert math.isnan(struct.unpack("d", struct.pack("Q", int(ans[(INF, 0.0, 1.0, -INF, INF)], 16)))[0])
    assert ans[(0.3, 0.0, 0.0, -1.0, 1.0)] == f"{_bits(INF):016x}" and ans[(0.3, 0.0, 0.7, -INF, INF)] == f"{_bits(INF):016x}"


def test_the_start_rule(printed):
    g = classify_grid()
    assert len(printed["classify"]) == len(g)
    for row, (state,) in zip(g, printed["classify"]):
        z, lo, hi, gi = (np.array([v]) for v in row)
        assert int(state) == B.classify_restated(z, lo, hi, gi, np.array([True]))[0], row
    ans = dict(zip(g, (int(s[0]) for s in printed["classify"])))
    assert ans[(0.5, 0.5, 1.0, 3.0)] == B.HELD_LO and ans[(0.5, 0.5, 1.0, -2.0)] == B.FREE and ans[(1.0, 0.5, 1.0, -2.0)] == B.HELD_HI
    assert ans[(1.0, 1.0, 1.0, 3.0)] == B.HELD_LO and ans[(1.0, 1.0, 1.0, -2.0)] == B.HELD_HI and ans[(1.0, 1.0, 1.0, 0.0)] == B.FREE
    assert ans[(1.0, 1.5, 0.0, 3.0)] == B.HELD_LO, "lo > hi: the lower bound is tested first"
    assert ans[(NAN, 0.5, 1.0, 3.0)] == B.FREE and ans[(0.5, 0.5, 1.0, NAN)] == B.FREE


def test_the_clamp_rule(printed):
    g = update_grid()
    assert len(printed["update"]) == len(g)
    seen = set()
    for row, (state, pbits, rbits, zbits) in zip(g, printed["update"]):
        s0, z, lo, hi, d, w, s, t, p, r = row
        a = lambda v: np.array([v])
        with np.errstate(all="ignore"):
            x = a(p) + s * a(d)
            want_r = a(r) + s * a(w)
        x, st, n_hit = B.clamp_restated(a(z), x, a(d), a(lo), a(hi), a(t), s, a(int(s0)))
        assert int(state) == st[0] and same(pbits, x[0]) and same(rbits, want_r[0]), (row, state, st)
        want_z = lo if st[0] == B.HIT_LO else hi if st[0] == B.HIT_HI else z + x[0]
        assert same(zbits, want_z), row
        assert n_hit == (1 if st[0] != int(s0) else 0)
        seen.add((int(s0), int(st[0])))
    assert seen == {(0, 0), (1, 1), (1, 4), (1, 5), (2, 2), (3, 3), (4, 4), (5, 5)}, "only a free entry changes its state"
    ans = dict(zip(g, printed["update"]))
    by_rounding = ans[(1.0, 0.1, -INF, 0.3, 0.2, 0.0, 1.0, float(np.nextafter(1.0, 2.0)), 0.0, 0.0)]
    assert 0.1 + (0.0 + 1.0 * 0.2) >= 0.3 and int(by_rounding[0]) == B.HIT_HI and by_rounding[3] == f"{_bits(0.3):016x}"
    assert by_rounding[1] == f"{_bits(0.3 - 0.1):016x}", "p = hi - Z, so that Zp is the bound itself"


def test_the_tree_of_minima(printed):
    g = min_grid()
    assert len(printed["mintree"]) == len(g)
    for row, (tree, line) in zip(g, printed["mintree"]):
        want = B.min_restated(row)
        assert same(tree, want) and same(line, want), "a minimum is exact: the tree and a left-to-right pass agree; NaNs are skipped"
    assert B.min_restated(g[3]) == 2.5 and B.min_restated(g[4]) == INF and B.min_restated(g[5]) == 0.0


def test_the_direction_rule(printed):
    g = direction_grid()
    assert len(printed["direction"]) == len(g)
    for (s, restart, beta, d, r), (dbits,) in zip(g, printed["direction"]):
        if restart:
            want = -r if s == B.FREE else 0.0
        else:
            want = 0.0 if s >= B.HIT_LO else beta * d - r
        assert same(dbits, want), (s, restart, beta, d, r)


@pytest.mark.parametrize("k", range(8))
def test_the_whole_loop_on_a_dense_matrix(printed, k):
    A, Z, g, fixed = loop_problem()
    has_lo, has_hi, radius, shift, rtol, atol, max_iter, lo, hi = loop_runs()[k]
    want = B.box_loop(lambda d: rows_dot(A, d), g, fixed == 0.0, Z, lo if has_lo else None, hi if has_hi else None, radius=radius, shift=shift,
                      rtol=rtol, atol=atol, max_iter=max_iter)
    p, info, trace, states, zp = (printed[f"loop_{w}"][k] for w in ("p", "info", "trace", "states", "zp"))
    it = int(want["info"][1])
    print("run", k, "status", int(info[0]), "iterations", int(info[1]), "held", info[8], "hit", info[9], "restarts", info[10], "|F|", info[11])
    assert np.array_equal(info, want["info"]), (info, want["info"])
    assert np.array_equal(p, want["p"]) and np.array_equal(states, want["states"]) and np.array_equal(zp, want["Zp"])
    trace = trace.reshape(max_iter, 6)
    assert np.array_equal(trace[:it], want["trace"]), (trace[:it], want["trace"])
    assert np.all(trace[it:] == -7.0), "rows past the last iteration are left as they were"
    assert printed["loop_again"][k] == ["1"]
    # what the run was chosen for
    status, restarts, hit, held = int(info[0]), int(info[10]), int(info[9]), int(info[8])
    if k == 0:
        assert status == CONVERGED and hit == held == restarts == 0 and np.all(states[fixed == 0.0] == B.FREE) and np.all(trace[:it, 4] == INF)
    if k == 1:
        assert status == CONVERGED and hit >= 3 and restarts >= 2
    if k == 2:
        assert status == MAX_ITER and it == 3
    if k == 3:
        assert np.any((trace[:it, 0] <= 0) & (trace[:it, 5] > 0)) and it > 1, "a negative-curvature step to a face, and on"
    if k == 4:
        assert status in (BOUNDARY, NEG_CURVATURE) and abs(info[4] - 1.0) <= 1e-12
    if k in (5, 6):
        assert held > 0 and np.all(p[(states == B.HELD_LO) | (states == B.HELD_HI)] == 0.0)
    if k == 7:
        assert np.all(p == 0.0) and np.all(trace[:it, 2] == 0.0) and int(info[11]) == 0
    free0 = fixed == 0.0
    assert np.all(p[~free0] == 0.0) and np.all(states[~free0] == B.FIXED)
    lo_, hi_ = (lo if has_lo else np.full(N_LOOP, -INF)), (hi if has_hi else np.full(N_LOOP, INF))
    moved = (states == B.FREE) | (states >= B.HIT_LO)
    assert np.all(zp[moved] >= lo_[moved]) and np.all(zp[moved] <= hi_[moved]), "inside the box, exactly"
    assert np.array_equal(zp[states == B.HIT_LO], lo_[states == B.HIT_LO]) and np.array_equal(zp[states == B.HIT_HI], hi_[states == B.HIT_HI])
    assert (info[8], info[9], info[11]) == (np.sum((states == 2) | (states == 3)), np.sum(states >= 4), np.sum(states == 1))


def test_without_bounds_the_loop_is_the_unbounded_loop(printed):
    """run 0 against the restatement of the unbounded step's loop (test_gpu_newton_step.cg_in_numpy's text, around the same product)"""
    A, Z, g, fixed = loop_problem()
    M = fixed == 0.0
    gm = np.where(M, g, 0.0)
    r, x, d = gm.copy(), np.zeros(N_LOOP), -gm
    rr0 = rr = B.dot(r, r)
    trace = []
    for j in range(1, 41):
        w = np.where(M, rows_dot(A, d) + 3.0 * d, 0.0)
        kappa, dd = B.dot(d, w), B.dot(d, d)
        status, s = decide_restated(kappa, dd, B.dot(x, d), B.dot(x, x), rr, 0.0, j)
        assert status == CONTINUE
        x, r = x + s * d, r + s * w
        rr_new = B.dot(r, r)
        trace.append([kappa, dd, s, rr_new])
        if np.sqrt(rr_new) <= 1e-8 * np.sqrt(rr0):
            break
        d, rr = (rr_new / rr) * d - r, rr_new
    pg = B.dot(x, gm)
    info = [CONVERGED, j, np.sqrt(rr0), np.sqrt(rr_new), np.sqrt(B.dot(x, x)), pg, -0.5 * (pg + B.dot(x, r)), kappa / dd]
    assert np.array_equal(printed["loop_p"][0], x) and np.array_equal(printed["loop_info"][0][:8], np.array(info, dtype=np.float64))
    assert np.array_equal(printed["loop_trace"][0].reshape(40, 6)[:j, :4], np.array(trace))


def test_the_sizes_and_the_codes(printed):
    assert printed["sizes"] == (12, 16, 12, 6, 3 * 11610 + 12 * 46 + 16 + -(-11610 // 8))
    assert printed["codes"] == (B.FIXED, B.FREE, B.HELD_LO, B.HELD_HI, B.HIT_LO, B.HIT_HI) == (0, 1, 2, 3, 4, 5)
