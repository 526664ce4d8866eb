"""csrc/dto_newton_plan.h from plain C++: a stand-alone program (its own main) is compiled with g++ (address and undefined-behaviour
sanitizers on) against the header alone (no HIP, no engine header) and run without a GPU.  It reads vectors and a grid of scalars from
a file written here, runs the header's dot (newton_dot: the functions the kernels call per lane, and the halving tree) and the header's
decision (newton_decide, the text the kernel calls), and prints the bits, which are compared with restatements in NumPy of what
include/dto_engine.h, "Truncated-Newton step", states."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")

# 1 chunk (ragged, full, one entry past), 46 chunks with a ragged last one, 64 chunks, 65 chunks (a lane of the final stage holds two
# partial sums), 87 chunks whose last holds 64 entries
LENGTHS = [1, 63, 64, 65, 255, 256, 257, 11610, 16384, 16385, 22080]
CONTINUE, CONVERGED, BOUNDARY, NEG_CURVATURE, MAX_ITER, NOT_FINITE = -1, 0, 1, 2, 3, 4

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dto_newton_plan.h"
using namespace dto;

static unsigned long long bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }
static void must_read(void* p, size_t n, FILE* f) { if (fread(p, 1, n, f) != n) { printf("FAILED short file\n"); exit(1); } }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long n_len = 0;
    must_read(&n_len, 8, f);
    for (long long c = 0; c < n_len; ++c) {
        long long n = 0;
        must_read(&n, 8, f);
        std::vector<double> x((size_t)n), y((size_t)n), P((size_t)newton_chunks(n));
        must_read(x.data(), 8 * (size_t)n, f);
        must_read(y.data(), 8 * (size_t)n, f);
        printf("dot %lld %lld %016llx\n", n, (long long)newton_chunks(n), bits(newton_dot(x.data(), y.data(), n, P.data())));
    }
    long long n_grid = 0;
    must_read(&n_grid, 8, f);
    for (long long c = 0; c < n_grid; ++c) {
        double v[7];
        must_read(v, sizeof v, f);
        const NewtonDecision D = newton_decide(v[0], v[1], v[2], v[3], v[4], v[5], (int)v[6]);
        printf("decide %d %016llx\n", D.status, bits(D.s));
    }
    double cv[4];
    long long n_conv = 0;
    must_read(&n_conv, 8, f);
    for (long long c = 0; c < n_conv; ++c) {
        must_read(cv, sizeof cv, f);
        printf("converged %d\n", newton_converged(cv[0], cv[1], cv[2], cv[3]) ? 1 : 0);
    }
    fclose(f);
    printf("sizes %d %d %d %lld\n", NEWTON_CHUNK, NEWTON_SLOTS, NEWTON_STATE, (long long)newton_workspace_doubles(11610));
    printf("codes %d %d %d %d %d %d\n", NEWTON_CONTINUE, NEWTON_CONVERGED, NEWTON_BOUNDARY, NEWTON_NEG_CURVATURE, NEWTON_MAX_ITER, NEWTON_NOT_FINITE);
    return 0;
}
"""


def vectors(n):
    """entries over twelve orders of magnitude with both signs, so that no two summation orders agree by accident"""
    rng = np.random.default_rng(1000 + n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    y = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    return x, y


def tree64(a):
    """the halving tree along the last axis of (.., 64): a_l += a_{l+off}, off = 32 .. 1; returns a_0"""
    a = a.copy()
    for off in (32, 16, 8, 4, 2, 1):
        a[..., :off] = a[..., :off] + a[..., off:2 * off]
    return a[..., 0]


def lanes(v):
    """v cut into rows of 64: lane l starts from 0 and adds row 0, row 1, .. of its column (absent entries add an exact 0)"""
    rows = -(-v.size // 64)
    pad = np.zeros(rows * 64)
    pad[:v.size] = v
    acc = np.zeros(64)
    for row in pad.reshape(rows, 64):
        acc = acc + row
    return acc


def dot_restated(x, y):
    prod = x * y
    nb = -(-x.size // 256)
    P = np.array([tree64(lanes(prod[256 * b:256 * (b + 1)])) for b in range(nb)])
    return tree64(lanes(P))


def tau(dd, pd, pp, radius):
    f = np.float64   # (scalar operations of NumPy round once each and return NaN or inf where Python raises)
    with np.errstate(all="ignore"):
        disc = f(pd) * f(pd) + f(dd) * (f(radius) * f(radius) - f(pp))
        return float((-f(pd) + np.sqrt(disc)) / f(dd))


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def decide_restated(kappa, dd, pd, pp, rr, radius, j):
    if not (math.isfinite(kappa) and math.isfinite(rr)):
        return NOT_FINITE, 0.0
    if kappa <= 0:
        return NEG_CURVATURE, (tau(dd, pd, pp, radius) if radius > 0 else (1.0 if j == 1 else 0.0))
    alpha = _div(rr, kappa)
    if radius > 0 and (pp + (2.0 * alpha) * pd) + (alpha * alpha) * dd >= radius * radius:
        return BOUNDARY, tau(dd, pd, pp, radius)
    return CONTINUE, alpha


def grid():
    rows = []
    for kappa in (0.0, -0.0, -2.5, 1e-300, 0.37, 3.7, math.nan, math.inf, -math.inf):
        for rr in (1.3, 4.0, math.nan, math.inf):
            for radius in (0.0, 0.9, 2.0, 1e3):
                for j in (1, 2, 5):
                    for dd, pd, pp in ((1.0, 0.0, 0.0), (2.3, 0.4, 0.5), (7.1, -0.9, 0.8), (0.6, 0.3, 3.9)):
                        rows.append((kappa, dd, pd, pp, rr, radius, float(j)))
    # the boundary exactly at equality: alpha = 4, p = 0, |d| = 1, so the trial point lies ON radius = 4; one ulp further out it is inside
    rows.append((1.0, 1.0, 0.0, 0.0, 4.0, 4.0, 3.0))
    rows.append((1.0, 1.0, 0.0, 0.0, 4.0, float(np.nextafter(4.0, 5.0)), 3.0))
    rows.append((1.0, 1.0, 0.0, 0.0, 4.0, float(np.nextafter(4.0, 3.0)), 3.0))
    # equality with p != 0: pp + 2 alpha pd + alpha^2 dd = 1 + 2 * 0.5 * 1 + 0.25 * 4 = 3 = radius^2 has no exact radius; 0.25 + 1 + 1 = 2.25 has
    rows.append((2.0, 4.0, 1.0, 0.25, 1.0, 1.5, 2.0))
    return rows


CONV = [(1e-12, 1.0, 1e-6, 0.0), (1.0000000001e-12, 1.0, 1e-6, 0.0), (4.0, 16.0, 0.5, 0.0), (4.0, 16.0, 0.49, 0.0), (4.0, 16.0, 0.1, 2.0),
        (4.0, 16.0, 0.1, 1.9), (0.0, 0.0, 0.0, 0.0), (math.nan, 1.0, 1e-6, 0.0)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("newton_plan")
    src, exe, data = str(tmp / "plan.cpp"), str(tmp / "plan"), str(tmp / "data.bin")
    with open(src, "w") as f:
        f.write(PROGRAM)
    with open(data, "wb") as f:
        f.write(struct.pack("q", len(LENGTHS)))
        for n in LENGTHS:
            x, y = vectors(n)
            f.write(struct.pack("q", n) + x.tobytes() + y.tobytes())
        g = grid()
        f.write(struct.pack("q", len(g)) + np.array(g, dtype=np.float64).tobytes())
        f.write(struct.pack("q", len(CONV)) + np.array(CONV, dtype=np.float64).tobytes())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe], check=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    out = dict(dot={}, decide=[], converged=[])
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "dot":
            out["dot"][int(w[1])] = (int(w[2]), int(w[3], 16))
        elif w[0] == "decide":
            out["decide"].append((int(w[1]), int(w[2], 16)))
        elif w[0] == "converged":
            out["converged"].append(int(w[1]))
        else:
            out[w[0]] = tuple(int(v) for v in w[1:])
    return out


def _bits(x):
    return struct.unpack("Q", struct.pack("d", x))[0]


@pytest.mark.parametrize("n", LENGTHS)
def test_the_headers_dot_order_is_the_stated_one(printed, n):
    x, y = vectors(n)
    chunks, got = printed["dot"][n]
    assert chunks == -(-n // 256)
    want = dot_restated(x, y)
    assert got == _bits(float(want)), (n, struct.unpack("d", struct.pack("Q", got))[0], want)
    if n >= 255:   # the order matters on these vectors: NumPy's pairwise dot gives other bits
        assert _bits(float(np.dot(x, y))) != got or _bits(float(np.sum(x * y))) != got


def test_the_chunk_counts_of_the_named_lengths():
    assert [-(-n // 256) for n in (11610, 16384, 16385, 22080)] == [46, 64, 65, 87]
    assert 11610 % 256 != 0 and 22080 - 86 * 256 == 64


def test_newton_decide_agrees_with_the_formulas_on_the_grid(printed):
    g = grid()
    assert len(printed["decide"]) == len(g)
    seen = set()
    for row, (status, sbits) in zip(g, printed["decide"]):
        want_status, want_s = decide_restated(*row[:6], int(row[6]))
        assert status == want_status, row
        if math.isnan(want_s):
            assert math.isnan(struct.unpack("d", struct.pack("Q", sbits))[0]), row
        else:
            assert sbits == _bits(want_s), (row, want_s)
        seen.add((status, row[5] > 0))
    # every branch was taken, with and without a radius where both exist
    assert seen >= {(NOT_FINITE, False), (NOT_FINITE, True), (NEG_CURVATURE, False), (NEG_CURVATURE, True), (BOUNDARY, True),
                    (CONTINUE, False), (CONTINUE, True)}


def test_answers_spelled_out(printed):
    g = grid()
    ans = dict(zip(g, printed["decide"]))
    one, zero = _bits(1.0), _bits(0.0)
    assert ans[(0.0, 1.0, 0.0, 0.0, 1.3, 0.0, 1.0)] == (NEG_CURVATURE, one), "kappa = 0 is non-positive curvature: the first iteration takes d"
    assert ans[(0.0, 1.0, 0.0, 0.0, 1.3, 0.0, 2.0)] == (NEG_CURVATURE, zero), "later iterations stay"
    assert ans[(-2.5, 1.0, 0.0, 0.0, 1.3, 2.0, 5.0)] == (NEG_CURVATURE, _bits(2.0)), "with a radius: to the boundary, tau = radius / |d|"
    assert ans[(math.nan, 1.0, 0.0, 0.0, 1.3, 0.0, 1.0)][0] == NOT_FINITE and ans[(3.7, 1.0, 0.0, 0.0, math.inf, 0.9, 1.0)][0] == NOT_FINITE
    assert ans[(1.0, 1.0, 0.0, 0.0, 4.0, 4.0, 3.0)] == (BOUNDARY, _bits(4.0)), "the trial point ON the boundary counts as reached (>=)"
    assert ans[(1.0, 1.0, 0.0, 0.0, 4.0, float(np.nextafter(4.0, 5.0)), 3.0)] == (CONTINUE, _bits(4.0))
    assert ans[(1.0, 1.0, 0.0, 0.0, 4.0, float(np.nextafter(4.0, 3.0)), 3.0)][0] == BOUNDARY
    assert ans[(2.0, 4.0, 1.0, 0.25, 1.0, 1.5, 2.0)] == (BOUNDARY, _bits(0.5)), "0.25 + 2 * 0.5 * 1 + 0.25 * 4 = 1.5^2 exactly; tau = alpha"
    assert ans[(3.7, 1.0, 0.0, 0.0, 1.3, 0.0, 1.0)] == (CONTINUE, _bits(1.3 / 3.7))


def test_the_convergence_test_and_the_sizes(printed):
    want = [1 if math.sqrt(a) <= max(d, c * math.sqrt(b)) else 0 for a, b, c, d in CONV[:-1]] + [0]
    assert printed["converged"] == want
    assert want[:7] == [1, 0, 1, 0, 1, 0, 1]
    assert printed["sizes"] == (256, 8, 16, 3 * 11610 + 8 * 46 + 16)
    assert printed["codes"] == (CONTINUE, CONVERGED, BOUNDARY, NEG_CURVATURE, MAX_ITER, NOT_FINITE)
