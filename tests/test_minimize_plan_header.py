"""csrc/dto_minimize_plan.h from plain C++: a stand-alone program (its own main) is compiled with g++ (address and undefined-behaviour
sanitizers on, -ffp-contract=off) against the header alone and run without a GPU; nothing is loaded into Python.  It prints the bits of
minimize_trial_decide and minimize_outer_decide on a grid and of the whole loop, minimize_solve, on toy callables; they are compared
with the NumPy restatement of minimize_cases.py.

The toy: f(Z) = 0.5 (a .* Z) . Z + 0.5 c (u . Z)^2 + q sum Z_i^4 with every dot in the truncated-Newton step's stated order, so that NumPy
can state it again; the step is the header's own newton_box_solve on the model WITHOUT the quartic term (so that trials are rejected);
the feasible map is the identity; one linear equality row w . Z - b with a multiplier and a penalty."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import auglag_cases as A
import minimize_cases as M
import newton_box_cases as B
from newton_box_cases import CONVERGED, NOT_FINITE
from test_gpu_newton_step import dot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
INF, NAN = math.inf, math.nan

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dto_minimize_plan.h"
#include "dto_newton_box_plan.h"
using namespace dto;

static unsigned long long bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }
static void must_read(void* p, size_t n, FILE* f) { if (n && fread(p, 1, n, f) != n) { printf("FAILED short file\n"); exit(1); } }
static std::vector<double> vec(FILE* f, size_t n) { std::vector<double> v(n); must_read(v.data(), 8 * n, f); return v; }
static void print_vector(const char* what, const double* v, size_t n) {
    printf("%s", what);
    for (size_t i = 0; i < n; ++i) printf(" %016llx", bits(v[i]));
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long count = 0;
    must_read(&count, 8, f);
    for (long long c = 0; c < count; ++c) {
        double k[5 + MINIMIZE_OPTIONS];   // phi, phi_t, predicted, step status, delta, options
        must_read(k, sizeof k, f);
        const MinimizeTrial D = minimize_trial_decide(k[0], k[1], k[2], (int)k[3], k[4], k + 5);
        printf("trial %016llx %d %016llx %d\n", bits(D.ratio), D.accepted, bits(D.delta_next), D.stop);
    }
    must_read(&count, 8, f);
    for (long long c = 0; c < count; ++c) {
        double k[3 + MINIMIZE_OPTIONS];   // viol, new viol, rho_r, options
        must_read(k, sizeof k, f);
        const MinimizeOuter D = minimize_outer_decide(k[0], k[1], k + 3);
        printf("outer %d %d %016llx\n", D.grew, D.stop, bits(minimize_rho_next(k[2], D.grew, k + 3)));
    }
    must_read(&count, 8, f);
    for (long long c = 0; c < count; ++c) {
        double k[10];   // n, has_rho, outer, trials, nan_at, q, c, mu0, rho0, b
        must_read(k, sizeof k, f);
        const long long n = (long long)k[0];
        const bool has_rho = k[1] != 0.0;
        const int outer = (int)k[2], trials = (int)k[3];
        const long long nan_at = (long long)k[4];
        const double q = k[5], cc = k[6], b = k[9];
        const std::vector<double> opt = vec(f, MINIMIZE_OPTIONS), a = vec(f, n), u = vec(f, n), w = vec(f, n), Z0 = vec(f, n);
        std::vector<double> Z = Z0, mu{k[7]}, rho{k[8]}, P((size_t)newton_chunks(n)), t1((size_t)n), t2((size_t)n), g((size_t)n), p((size_t)n);
        std::vector<unsigned char> fixed((size_t)n, 0);
        const unsigned char is_eq = 1;
        long long merits = 0;
        auto row = [&](const double* z) { return newton_sub(newton_dot(w.data(), z, n, P.data()), b); };
        auto merit = [&](const double* Zin, double* Zout) {
            if (Zout != Zin) for (long long i = 0; i < n; ++i) Zout[i] = Zin[i];
            for (long long i = 0; i < n; ++i) { t1[(size_t)i] = newton_mul(a[(size_t)i], Zout[i]); t2[(size_t)i] = newton_mul(Zout[i], Zout[i]); }
            const double s = newton_dot(u.data(), Zout, n, P.data());
            double phi = newton_mul(0.5, newton_dot(t1.data(), Zout, n, P.data()));
            phi = newton_add(phi, newton_mul(newton_mul(0.5, cc), newton_mul(s, s)));
            phi = newton_add(phi, newton_mul(q, newton_dot(t2.data(), t2.data(), n, P.data())));
            if (has_rho) phi = newton_add(phi, al_row(true, row(Zout), mu[0], rho[0]).psi);
            return merits++ == nan_at ? al_nan() : phi;
        };
        auto step = [&](const double* z, double delta, double* Zp, double* sinfo) {
            const double cs = newton_mul(cc, newton_dot(u.data(), z, n, P.data()));
            const AlRow R = has_rho ? al_row(true, row(z), mu[0], rho[0]) : AlRow{0.0, 0.0, 0.0, 0.0};
            for (long long i = 0; i < n; ++i) {
                const double z2 = newton_mul(z[i], z[i]);
                g[(size_t)i] = newton_add(newton_add(newton_mul(a[(size_t)i], z[i]), newton_mul(cs, u[(size_t)i])), newton_mul(newton_mul(newton_mul(4.0, q), z2), z[i]));
                if (has_rho) g[(size_t)i] = newton_add(g[(size_t)i], newton_mul(R.mult, w[(size_t)i]));
            }
            auto apply = [&](const double* d, double* y) {
                const double cd = newton_mul(cc, newton_dot(u.data(), d, n, P.data()));
                const double wd = has_rho ? newton_mul(R.weight, newton_dot(w.data(), d, n, P.data())) : 0.0;
                for (long long i = 0; i < n; ++i) {
                    y[i] = newton_add(newton_mul(a[(size_t)i], d[i]), newton_mul(cd, u[(size_t)i]));
                    if (has_rho) y[i] = newton_add(y[i], newton_mul(wd, w[(size_t)i]));
                }
            };
            newton_box_solve(n, z, g.data(), fixed.data(), nullptr, nullptr, delta, opt[MIN_OPT_SHIFT], opt[MIN_OPT_RTOL], opt[MIN_OPT_ATOL],
                             (int)opt[MIN_OPT_MAX_ITER], apply, p.data(), sinfo, nullptr, nullptr, Zp);
        };
        auto rows = [&](const double* z, double* mu_eff, double* rinfo) {
            const double gr = row(z);
            al_rows_pass(1, &is_eq, &gr, mu.data(), rho.data(), mu_eff, nullptr, rinfo);
        };
        std::vector<double> info(MINIMIZE_INFO, -7.0), hist((size_t)(MINIMIZE_HISTORY * outer * trials), -7.0), ohist((size_t)(MINIMIZE_OUTER_HISTORY * outer), -7.0);
        minimize_solve(n, 1, 0, Z.data(), has_rho ? mu.data() : nullptr, has_rho ? rho.data() : nullptr, opt.data(), outer, trials, 12, step, merit, rows,
                       info.data(), hist.data(), ohist.data());
        print_vector("run_Z", Z.data(), Z.size());
        print_vector("run_mu", mu.data(), 1);
        print_vector("run_rho", rho.data(), 1);
        print_vector("run_info", info.data(), info.size());
        print_vector("run_history", hist.data(), hist.size());
        print_vector("run_outer", ohist.data(), ohist.size());
        printf("run_merits %lld\n", merits);
    }
    fclose(f);
    const MinimizeOptions D = minimize_default_options();
    print_vector("defaults", D.v, MINIMIZE_OPTIONS);
    printf("sizes %d %d %d %d %d %d\n", MINIMIZE_OPTIONS, MINIMIZE_STATE, MINIMIZE_INFO, MINIMIZE_HISTORY, MINIMIZE_OUTER_HISTORY, MINIMIZE_MAIL);
    return 0;
}
"""


# ------------------------------------------------------------------------------------------------------------- the grids
def trial_grid():
    """(phi, phi_t, predicted, step status, delta, options)"""
    out = []
    d = M.options()
    # ratios exactly at the three bars (predicted = 1, phi_t = 0: ratio = phi), just beside them, and far away
    for ratio in (0.1, 0.25, 0.75, np.nextafter(0.1, 1), np.nextafter(0.25, 0), np.nextafter(0.75, 1), -3.0, 0.5, 0.9, 1.0, 40.0):
        for status in (CONVERGED, 1, 2, 3):
            out.append((float(ratio), 0.0, 1.0, status, 1.0, d))
    out += [(2.0, 1.0, 0.0, 1, 1.0, d), (1.0, 1.0, 0.0, 1, 1.0, d), (1.0, 2.0, 0.0, 1, 0.5, d)]               # predicted = 0: +inf, NaN, -inf
    out += [(1.0, NAN, 0.3, 1, 1.0, d), (1.0, INF, 0.3, 1, 1.0, d), (1.0, -INF, 0.3, 1, 2.0, d), (NAN, 0.0, 1.0, 1, 1.0, d)]
    out += [(1.0, 0.1, 1.0, NOT_FINITE, 1.0, d), (1.0, 0.5, 1.0, NOT_FINITE, 3.0, d)]                            # a good ratio, a step that is not finite
    out += [(1.0, 0.1, 1.0, CONVERGED, 1.0, d), (1.0, 0.1, 1.0, 1, 1.0, d)]                                    # ratio 0.9: no growth behind CONVERGED
    capped = M.options(radius_max=1.5)
    out += [(1.0, 0.1, 1.0, 1, 1.0, capped), (1.0, 0.1, 1.0, 1, 0.75, capped), (1.0, 0.1, 1.0, 1, 0.5, capped), (1.0, 0.1, 1.0, 1, 1.5, capped)]
    floor = M.options(radius_min=0.3)
    out += [(0.0, 1.0, 1.0, 1, 1.0, floor), (0.0, 1.0, 1.0, 1, 1.2, floor), (0.0, 1.0, 1.0, 1, 1.25, floor), (1.0, 0.5, 1.0, 1, 0.2, floor)]
    other = M.options(eta_accept=0.0, eta_shrink=0.5, eta_grow=0.5000001, shrink_div=3.0, grow_mul=1.0)
    out += [(r, 0.0, 1.0, 1, 0.7, other) for r in (0.0, 1e-300, 0.5, 0.50000005, 0.6, -1e-300)]
    return out


def outer_grid():
    """(viol, new viol, rho_r, options)"""
    d, other = M.options(), M.options(viol_div=2.0, rho_mul=3.0, ctol=1e-3)
    out = []
    for opt in (d, other):
        for viol, new in ((1.0, 0.25), (1.0, np.nextafter(0.25, 1)), (1.0, 0.5), (1.0, 0.1), (0.0, 0.0), (NAN, 0.1), (1.0, NAN), (NAN, NAN), (INF, 1.0),
                          (1.0, 1e-3), (1.0, 1e-4), (0.004, 1e-3)):
            for rho in (10.0, 0.0, 1e308):
                out.append((viol, new, rho, opt))
    return out


# ------------------------------------------------------------------------------------------------------------ the toy runs
def toy(n, seed):
    rng = np.random.default_rng(seed)
    a = 10.0 ** rng.uniform(-0.5, 0.5, n)
    u = rng.standard_normal(n) / math.sqrt(n)
    w = rng.standard_normal(n) / math.sqrt(n)
    Z0 = 2.0 * rng.standard_normal(n) / math.sqrt(n) + 0.3
    return dict(n=n, a=a, u=u, w=w, Z0=Z0, q=0.5 * n, c=3.0, b=0.4)


def toy_callables(ty, nan_at):
    a, u, w, q, c, b = (ty[k] for k in ("a", "u", "w", "q", "c", "b"))
    n = ty["n"]
    calls = [0]
    row = lambda Z: np.array([F(dot(w, Z)) - F(b)])
    F = np.float64
    eq = np.array([True])

    def merit(Z, mu, rho):
        Z = np.array(Z)
        z2 = Z * Z
        s = F(dot(u, Z))
        phi = F(0.5) * F(dot(a * Z, Z))
        phi = phi + (F(0.5) * F(c)) * (s * s)
        phi = phi + F(q) * F(dot(z2, z2))
        if rho is not None:
            phi = phi + A.rows_restated(eq, row(Z), mu, rho)[0][0]
        calls[0] += 1
        return (NAN if calls[0] - 1 == nan_at else float(phi)), Z

    def step(Z, delta, mu, rho):
        cs = F(c) * F(dot(u, Z))
        g = (a * Z + cs * u) + ((F(4.0) * F(q)) * (Z * Z)) * Z
        weight = 0.0
        if rho is not None:
            _, mult, wt, _ = A.rows_restated(eq, row(Z), mu, rho)
            g = g + mult[0] * w
            weight = wt[0]

        def product(d):
            y = a * d + (F(c) * F(dot(u, d))) * u
            if rho is not None:
                y = y + (F(weight) * F(dot(w, d))) * w
            return y

        out = B.box_loop(product, g, np.ones(n, dtype=bool), Z, radius=delta, **ty["kw"])
        return out["info"], out["Zp"]

    def rows(Z, mu, rho):
        g = row(Z)
        return A.rows_restated(eq, g, mu, rho)[1], A.info_restated(eq, g, mu, rho)

    return step, merit, rows, calls


def runs():
    out = []

    def add(what, ty, rho=None, outer=1, trials=8, nan_at=-1, **opt):
        out.append(dict(what=what, ty=ty, rho=rho, outer=outer, trials=trials, nan_at=nan_at, opt=M.options(**dict(dict(max_iter=20, rtol=1e-6, radius0=8.0), **opt))))

    for n, seed in ((5, 1), (257, 2), (4200, 3)):
        ty = toy(n, seed)
        g0 = float(np.linalg.norm((ty["a"] * ty["Z0"] + ty["c"] * (ty["u"] @ ty["Z0"]) * ty["u"]) + 4.0 * ty["q"] * ty["Z0"] ** 3))
        add(f"n{n}_plain", ty)                                               # the stops disabled
        add(f"n{n}_rho", ty, rho=5.0, outer=3, trials=4)
        add(f"n{n}_gtol", ty, trials=30, gtol=0.05 * g0)
        add(f"n{n}_radius_min", ty, radius_min=2.5)
        add(f"n{n}_nan", ty, nan_at=3)
        add(f"n{n}_rho_nan", ty, rho=5.0, outer=3, trials=4, nan_at=7)
    ty = toy(257, 2)
    add("rho_converged", ty, rho=5.0, outer=6, trials=30, gtol=1.0, ctol=0.05)
    add("rho_grows", ty, rho=0.01, outer=4, trials=3, viol_div=1e6)
    add("other_rules", ty, trials=12, eta_accept=0.2, eta_shrink=0.3, eta_grow=0.6, shrink_div=2.0, grow_mul=3.0, radius_max=2.5, radius0=0.4, shift=0.5)
    return out


RUNS = runs()
TRIALS, OUTERS = trial_grid(), outer_grid()


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("minimize_plan")
    src, exe, data = str(tmp / "plan.cpp"), str(tmp / "plan"), str(tmp / "data.bin")
    with open(src, "w") as f:
        f.write(PROGRAM)
    with open(data, "wb") as f:
        f.write(struct.pack("q", len(TRIALS)))
        for *head, opt in TRIALS:
            f.write(np.array(list(head) + list(opt), dtype=np.float64).tobytes())
        f.write(struct.pack("q", len(OUTERS)))
        for *head, opt in OUTERS:
            f.write(np.array(list(head) + list(opt), dtype=np.float64).tobytes())
        f.write(struct.pack("q", len(RUNS)))
        for r in RUNS:
            ty = r["ty"]
            head = [ty["n"], r["rho"] is not None, r["outer"], r["trials"], r["nan_at"], ty["q"], ty["c"], 0.25, r["rho"] or 0.0, ty["b"]]
            f.write(np.array(head, dtype=np.float64).tobytes())
            for a in (r["opt"], ty["a"], ty["u"], ty["w"], ty["Z0"]):
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe], check=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    out = {}
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] in ("sizes", "trial", "outer", "run_merits"):
            out.setdefault(w[0], []).append(w[1:])
        else:
            out.setdefault(w[0], []).append(np.array([int(v, 16) for v in w[1:]], dtype=np.uint64).view(np.float64))
    return out


def f64(word):
    return np.array([int(word, 16)], dtype=np.uint64).view(np.float64)[0]


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)) or (a.shape == b.shape and np.array_equal(a, b, equal_nan=True))


def test_the_sizes_and_the_defaults(printed):
    assert tuple(int(v) for v in printed["sizes"][0]) == (16, 16, 16, 8, 4, 4)
    assert same(printed["defaults"][0], np.array(M.DEFAULTS))
    plan = open(os.path.join(CSRC, "dto_minimize_plan.h")).read()
    import re
    assert "hip" not in re.sub(r"//.*", "", plan).lower().replace("__hipcc__", ""), "plain C++: no HIP in the header"


def test_the_trial_decision_on_the_grid(printed):
    assert len(printed["trial"]) == len(TRIALS)
    seen = set()
    for (phi, phi_t, predicted, status, delta, opt), got in zip(TRIALS, printed["trial"]):
        ratio, accepted, delta_next, stop = M.trial_decide(phi, phi_t, predicted, status, delta, opt)
        g_ratio, g_delta = f64(got[0]), f64(got[2])
        assert same(g_ratio, ratio) and int(got[1]) == int(accepted) and same(g_delta, delta_next) and int(got[3]) == stop, (phi, phi_t, predicted, status, delta)
        seen.add((stop, accepted, delta_next < delta, delta_next > delta))
    # the defaults at the bars, as the README's comparisons decide them
    d = M.options()
    assert M.trial_decide(0.1, 0.0, 1.0, 1, 1.0, d) == (0.1, False, 0.25, 0), "ratio == 0.1 is not accepted, and shrinks"
    assert M.trial_decide(0.25, 0.0, 1.0, 1, 1.0, d) == (0.25, True, 1.0, 0), "ratio == 0.25 does not shrink"
    assert M.trial_decide(0.75, 0.0, 1.0, 1, 1.0, d) == (0.75, True, 1.0, 0), "ratio == 0.75 does not grow"
    assert M.trial_decide(1.0, 0.1, 1.0, CONVERGED, 1.0, d)[2] == 1.0 and M.trial_decide(1.0, 0.1, 1.0, 1, 1.0, d)[2] == 2.0
    assert M.trial_decide(1.0, 0.1, 1.0, 1, 1.0, M.options(radius_max=1.5))[2] == 1.5, "radius_max reached"
    assert M.trial_decide(0.0, 1.0, 1.0, 1, 1.0, M.options(radius_min=0.3))[2:] == (0.25, M.STOP_RADIUS), "radius_min crossed"
    assert M.trial_decide(2.0, 1.0, 0.0, 1, 1.0, d)[1:] == (False, 1.0, M.STOP_NOT_FINITE), "predicted = 0"
    assert M.trial_decide(1.0, 0.1, 1.0, NOT_FINITE, 3.0, d)[1:] == (False, 3.0, M.STOP_NOT_FINITE)
    assert {s[0] for s in seen} == {M.STOP_NONE, M.STOP_RADIUS, M.STOP_NOT_FINITE}


def test_the_outer_decision_on_the_grid(printed):
    assert len(printed["outer"]) == len(OUTERS)
    for (viol, new, rho, opt), got in zip(OUTERS, printed["outer"]):
        grew, feasible = M.outer_decide(viol, new, opt)
        want = M.rho_next(np.array([rho]), grew, opt)[0]
        assert int(got[0]) == int(grew) and int(got[1]) == int(feasible) and same(f64(got[2]), want), (viol, new, rho)
    d = M.options()
    assert M.outer_decide(NAN, 0.1, d)[0] and M.outer_decide(1.0, NAN, d)[0], "a NaN grows the penalty"
    assert not M.outer_decide(1.0, 0.25, d)[0] and M.outer_decide(1.0, np.nextafter(0.25, 1), d)[0]
    assert M.rho_next(np.array([0.0, 10.0]), True, d).tolist() == [0.0, 100.0], "a row with rho_r = 0 stays unpenalised"


@pytest.fixture(scope="module")
def restated():
    out = []
    for r in RUNS:
        ty = dict(r["ty"], kw=M.step_kw(r["opt"]))
        step, merit, rows, calls = toy_callables(ty, r["nan_at"])
        has_rho = r["rho"] is not None
        with np.errstate(all="ignore"):
            run = M.minimize_loop(step, merit, rows, ty["Z0"], np.array([0.25]) if has_rho else None, np.array([r["rho"]]) if has_rho else None, 0,
                                  r["opt"], r["outer"], r["trials"])
        out.append(dict(run, calls=calls[0]))
    return out


@pytest.mark.parametrize("i", range(len(RUNS)), ids=[r["what"] for r in RUNS])
def test_the_whole_loop_equals_the_restatement_bit_for_bit(printed, restated, i):
    r, want = RUNS[i], restated[i]
    info = printed["run_info"][i]
    nt, no = len(want["history"]), len(want["outer_history"])
    print(r["what"], "status", info[0], "outer", info[1], "trials", info[2], "accepted", info[3], "phi", info[4], info[5], "delta", info[6], "viol", info[8],
          info[9], "grew", info[10])
    assert same(info, want["info"]), (info, want["info"])
    assert same(printed["run_Z"][i], want["Z"])
    if r["rho"] is not None:
        assert same(printed["run_mu"][i], want["mu"]) and same(printed["run_rho"][i], want["rho"])
    hist = printed["run_history"][i].reshape(-1, 8)
    assert same(hist[:nt], want["history"]) and np.all(hist[nt:] == -7.0), "rows past the last trial are left as they are"
    oh = printed["run_outer"][i].reshape(-1, 4)
    assert same(oh[:no], want["outer_history"]) and np.all(oh[no:] == -7.0)
    assert int(printed["run_merits"][i][0]) == want["calls"] == want["merits"]


def test_what_the_runs_are_there_for(restated):
    by = {r["what"]: w for r, w in zip(RUNS, restated)}
    for n in (5, 257, 4200):
        plain = by[f"n{n}_plain"]
        assert plain["info"][0] == M.M_MAX_TRIALS and plain["info"][2] == 8, "the stops disabled: every trial runs"
        assert 0 < plain["info"][3] < 8, "accepted and rejected trials"
        assert np.all(np.diff([plain["info"][4]] + [row[3] for row in plain["history"] if row[1]]) < 0.0), "phi falls over the accepted trials"
        rho = by[f"n{n}_rho"]
        assert rho["info"][0] == M.M_MAX_OUTER and rho["info"][1] == 3 and rho["info"][2] == 12 and len(rho["outer_history"]) == 3
        g = by[f"n{n}_gtol"]
        assert g["info"][0] == M.M_CONVERGED and g["info"][2] < 30 and g["history"][-1][1] == 0.0 and g["history"][-1][0] == 0.0
        assert g["merits"] == g["info"][2], "no merit behind the last step: one in front, one per trial but the last"
        rm = by[f"n{n}_radius_min"]
        assert rm["info"][0] == M.M_RADIUS and rm["info"][6] == 2.0 and rm["history"][-1][0] < 0.25, "RADIUS behind the first shrink"
        assert np.all(rm["history"][:, 2] >= 8.0)
        nan = by[f"n{n}_nan"]
        assert nan["info"][0] == M.M_NOT_FINITE and nan["info"][2] == 3 and np.isnan(nan["history"][-1][3]) and nan["history"][-1][1] == 0.0
        rn = by[f"n{n}_rho_nan"]
        assert rn["info"][0] == M.M_NOT_FINITE and rn["info"][1] == 2 and len(rn["outer_history"]) == 1, "no row pass behind NOT_FINITE"
    assert by["rho_converged"]["info"][0] == M.M_CONVERGED and by["rho_converged"]["info"][9] <= 0.05
    assert by["rho_grows"]["info"][10] == 4 and by["rho_grows"]["rho"][0] == 0.01 * 10.0 * 10.0 * 10.0 * 10.0
    assert np.max(by["other_rules"]["history"][:, 2]) <= 2.5
