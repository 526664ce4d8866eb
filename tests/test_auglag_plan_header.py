"""csrc/dto_auglag_plan.h from plain C++: a stand-alone program (its own main) is compiled with g++ (address and undefined-behaviour
sanitizers on) against the header alone and run without a GPU.  It runs the header's row rule (al_row) on a grid and its whole row pass
(al_rows_pass) on 1, 63, 64, 65 and 300 rows and prints the bits, which are compared with the restatements in NumPy of auglag_cases.py --
what include/dto_engine.h, "Augmented-Lagrangian terms", states."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import auglag_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
INF, NAN = math.inf, math.nan
PASS_ROWS = (1, 63, 64, 65, 300)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dto_auglag_plan.h"
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
    for (long long c = count_of(f); c > 0; --c) {   // is_eq, g, mu, rho
        double v[4];
        must_read(v, sizeof v, f);
        const AlRow R = al_row(v[0] != 0.0, v[1], v[2], v[3]);
        printf("row %016llx %016llx %016llx %016llx\n", bits(R.psi), bits(R.mult), bits(R.weight), bits(R.viol));
    }
    for (long long c = count_of(f); c > 0; --c) {   // n, has_mu, then is_eq, g, mu, rho as doubles
        const long long n = count_of(f), has_mu = count_of(f);
        std::vector<double> e((size_t)n), g((size_t)n), mu((size_t)n), rho((size_t)n), mult((size_t)n, -7.0), weight((size_t)n, -7.0), info(AL_INFO, -7.0);
        must_read(e.data(), 8 * e.size(), f);
        must_read(g.data(), 8 * g.size(), f);
        must_read(mu.data(), 8 * mu.size(), f);
        must_read(rho.data(), 8 * rho.size(), f);
        std::vector<unsigned char> eq((size_t)n);
        for (long long i = 0; i < n; ++i) eq[(size_t)i] = e[(size_t)i] != 0.0;
        al_rows_pass(n, eq.data(), g.data(), has_mu ? mu.data() : nullptr, rho.data(), mult.data(), weight.data(), info.data());
        print_vector("pass_mult", mult);
        print_vector("pass_weight", weight);
        print_vector("pass_info", info);
        double i2[AL_INFO];   // the optional outputs left out: the same scalars
        al_rows_pass(n, eq.data(), g.data(), has_mu ? mu.data() : nullptr, rho.data(), nullptr, nullptr, i2);
        printf("pass_again %d\n", memcmp(i2, info.data(), sizeof i2) == 0 ? 1 : 0);
    }
    fclose(f);
    printf("slots %d %d %d %d %d %d %d\n", AL_P, AL_ACTIVE, AL_MAX_VIOL, AL_SUM_VIOL2, AL_MAX_DMULT, AL_PENALISED, AL_INFO);
    return 0;
}
"""


# ---------------------------------------------------------------------------------------------------------------- the grids
def row_grid():
    """s = mu + rho g equal to 0 and one ulp to either side (by moving mu), rho = 0, both kinds of row, NaN, infinite and negative inputs"""
    rows = []
    for rho in (10.0, 0.3, 1e-300, 1e300):
        for g in (0.25, -0.25, 1e-9, -3.0, 0.0, -0.0):
            mu0 = -(rho * g)                         # exactly representable: s = 0 up to the rounding of the sum
            for mu in (mu0, np.nextafter(mu0, INF), np.nextafter(mu0, -INF), 1.0, -1.0, 0.0):
                rows += [(e, g, float(mu), rho) for e in (0.0, 1.0)]
    specials = (0.0, -0.0, 1.0, -1.0, INF, -INF, NAN, 5e-324, 1.7e308)
    for g in specials:
        for mu in specials:
            for rho in (0.0, 10.0, -0.0, -1.0, INF, -INF, NAN):
                rows += [(e, g, mu, rho) for e in (0.0, 1.0)]
    return rows


def pass_cases():
    out = []
    for k, n in enumerate(PASS_ROWS):
        rng = np.random.default_rng(40 + n)
        is_eq = (rng.random(n) < 0.3).astype(np.float64)
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)
        mu = rng.standard_normal(n)
        rho = np.where(rng.random(n) < 0.2, 0.0, 10.0 ** rng.integers(-2, 4, n))
        out.append((n, 1, is_eq, g, mu, rho))
    n = 300
    rng = np.random.default_rng(7)
    out.append((n, 0, np.zeros(n), rng.standard_normal(n), np.zeros(n), np.full(n, 10.0)))                     # mu = NULL: zeros
    out.append((n, 1, np.zeros(n), rng.standard_normal(n), rng.standard_normal(n), np.zeros(n)))                # every rho = 0: the merit's sum
    g = rng.standard_normal(n)
    g[137] = NAN
    out.append((n, 1, np.zeros(n), g, rng.standard_normal(n), np.full(n, 10.0)))                                # one NaN row
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("auglag_plan")
    src, exe, data = str(tmp / "plan.cpp"), str(tmp / "plan"), str(tmp / "data.bin")
    with open(src, "w") as f:
        f.write(PROGRAM)
    with open(data, "wb") as f:
        rows = row_grid()
        f.write(struct.pack("<q", len(rows)))
        f.write(np.asarray(rows, dtype="<f8").tobytes())
        cases = pass_cases()
        f.write(struct.pack("<q", len(cases)))
        for n, has_mu, is_eq, g, mu, rho in cases:
            f.write(struct.pack("<qq", n, has_mu))
            for a in (is_eq, g, mu, rho):
                f.write(np.asarray(a, dtype="<f8").tobytes())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe], check=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    out = {"row": [], "pass_mult": [], "pass_weight": [], "pass_info": [], "pass_again": []}
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "slots":
            out["slots"] = tuple(int(v) for v in w[1:])
        elif w[0] == "pass_again":
            out["pass_again"].append(int(w[1]))
        else:
            out[w[0]].append(np.array([int(v, 16) for v in w[1:]], dtype=np.uint64).view(np.float64))
    return out


def same(a, b):
    """equal bits, except that every NaN is one value"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------------------------ tests
def test_the_row_rule_on_the_grid(printed):
    rows = np.asarray(row_grid())
    got = np.array(printed["row"])
    assert got.shape == (rows.shape[0], 4)
    psi, mult, weight, viol = A.rows_restated(rows[:, 0] != 0.0, rows[:, 1], rows[:, 2], rows[:, 3])
    for k, want in enumerate((psi, mult, weight, viol)):
        bad = [i for i in range(rows.shape[0]) if not same(got[i, k:k + 1], want[i:i + 1])]
        assert not bad, (("psi", "mult", "weight", "viol")[k], rows[bad[0]], got[bad[0]], want[bad[0]])


def test_what_the_rule_promises(printed):
    rows = np.asarray(row_grid())
    got = np.array(printed["row"])
    is_eq, g, mu, rho = rows[:, 0] != 0.0, rows[:, 1], rows[:, 2], rows[:, 3]
    psi, mult, weight, viol = got.T
    refused = np.isnan(g) | np.isnan(mu) | np.isnan(rho) | (rho < 0.0)
    assert np.isnan(psi[refused]).all() and np.isnan(mult[refused]).all(), "a NaN input or a negative rho gives NaN in psi and mult"
    plain = ~refused & (rho == 0.0)
    assert plain.any() and same(mult[plain], mu[plain]) and np.all(weight[plain] == 0.0), "rho == 0: the row is not penalised"
    with np.errstate(all="ignore"):
        assert same(psi[plain], mu[plain] * g[plain])
        s = mu + rho * g
    pen = ~refused & (rho > 0.0)
    active = pen & (is_eq | (s > 0.0))
    inactive = pen & ~is_eq & ~(s > 0.0)
    assert active.any() and inactive.any()
    assert same(mult[active], s[active]) and same(weight[active], rho[active])
    assert np.all(mult[inactive] == 0.0) and np.all(weight[inactive] == 0.0)
    edge = pen & ~is_eq & (s == 0.0)
    assert edge.any() and np.all(weight[edge] == 0.0), "s == 0 is inactive"
    ok = ~np.isnan(g)
    assert np.all(viol[ok & is_eq] == np.abs(g[ok & is_eq])) and np.all(viol[ok & ~is_eq] == np.maximum(0.0, g[ok & ~is_eq]))


def test_the_row_pass_and_the_order_of_its_sums(printed):
    assert printed["slots"] == (0, 1, 2, 3, 4, 5, 8)
    cases = pass_cases()
    assert len(printed["pass_info"]) == len(cases) and all(v == 1 for v in printed["pass_again"])
    for k, (n, has_mu, is_eq, g, mu, rho) in enumerate(cases):
        m = mu if has_mu else np.zeros(n)
        psi, mult, weight, _ = A.rows_restated(is_eq != 0.0, g, m, rho)
        assert same(printed["pass_mult"][k], mult) and same(printed["pass_weight"][k], weight), (k, n)
        want = A.info_restated(is_eq != 0.0, g, m, rho)
        assert same(printed["pass_info"][k], want), (k, n, printed["pass_info"][k], want)
    # every rho = 0: P is the merit's sum of mu_r g_r in the same order
    n, _, _, g, mu, _ = cases[-2]
    assert printed["pass_info"][-2][0] == A.lane_sum(mu * g) and printed["pass_info"][-2][1] == 0.0 and printed["pass_info"][-2][5] == 0.0
    assert np.isnan(printed["pass_info"][-1][[0, 2, 3, 4]]).all() and printed["pass_info"][-1][5] == 300.0, "a NaN row shows in P and both maxima"


def test_the_lane_order_is_not_the_plain_order():
    """the restated sum differs from a left-to-right sum on 300 rows: the test above can tell the orders apart"""
    differs = 0
    for seed in range(8):
        x = np.random.default_rng(seed).standard_normal(300)
        plain = 0.0
        for v in x:
            plain += v
        differs += A.lane_sum(x) != plain
        assert abs(A.lane_sum(x) - plain) <= 1e-12
    assert differs >= 4
    assert A.lane_sum(x[:1]) == x[0]
