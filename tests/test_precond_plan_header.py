"""csrc/dto_precond_plan.h from plain C++: a stand-alone program (its own main) is compiled with g++ (address and undefined-behaviour
sanitizers on, -ffp-contract=off) against the header alone and run without a GPU; nothing is loaded into Python.  It runs the header's
preparation and application (PrecondHost) and its whole loop (precond_solve) on symmetric systems of 5, 257 and 16500 entries -- one
chunk, several chunks, and more than 64 chunks, so that stage 2's second trip runs -- and prints the bits, which are compared with the
NumPy restatement of precond_cases.py.

The operator is A d = dg .* d + sum_k (coef_k (u_k . d)) u_k with the dot in the stated order, so that NumPy can state it again."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import newton_box_cases as B
import precond_cases as PC
from newton_box_cases import CONVERGED, MAX_ITER
from test_gpu_newton_step import dot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
INF = math.inf
RANK = 3

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dto_precond_plan.h"
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
    long long runs = 0;
    must_read(&runs, 8, f);
    for (long long c = 0; c < runs; ++c) {
        double k[11];   // n, has_lo, has_hi, radius, shift, rtol, atol, max_iter, cnt, m, harvest
        must_read(k, sizeof k, f);
        const long long n = (long long)k[0];
        const int max_iter = (int)k[7], cnt = (int)k[8], m = (int)k[9], harvest = (int)k[10];
        const std::vector<double> dg = vec(f, n), U = vec(f, RANK * n), coef = vec(f, RANK), Z = vec(f, n), g = vec(f, n), fx = vec(f, n), lo = vec(f, n),
                                  hi = vec(f, n), S = vec(f, (size_t)cnt * n), Y = vec(f, (size_t)cnt * n);
        std::vector<unsigned char> fixed((size_t)n), nonfixed((size_t)n);
        for (long long i = 0; i < n; ++i) { fixed[(size_t)i] = fx[(size_t)i] != 0.0; nonfixed[(size_t)i] = !fixed[(size_t)i]; }
        std::vector<double> P((size_t)newton_chunks(n));
        auto apply = [&](const double* d, double* y) {
            for (long long i = 0; i < n; ++i) y[i] = newton_mul(dg[(size_t)i], d[i]);
            for (int r = 0; r < RANK; ++r) {
                const double t = newton_mul(coef[(size_t)r], newton_dot(U.data() + (size_t)r * n, d, n, P.data()));
                for (long long i = 0; i < n; ++i) y[i] = newton_add(y[i], newton_mul(t, U[(size_t)r * n + i]));
            }
        };
        // the application alone: F0 = F = the entries that are not fixed, r = g
        PrecondHost H;
        H.prepare(n, cnt, S.data(), Y.data(), nonfixed.data());
        std::vector<double> z((size_t)n);
        const double rz = H.apply(g.data(), nonfixed.data(), true, z.data());
        printf("admitted %d %016llx %016llx\n", H.admitted(), bits(H.pc[PPC_GAMMA]), bits(rz));
        print_vector("apply_z", z.data(), (size_t)n);
        // the loop
        const int hm = m > 0 ? m : 1;
        std::vector<double> p((size_t)n), info(PRECOND_INFO), trace((size_t)(PRECOND_TRACE * max_iter), -7.0), es((size_t)n), zp((size_t)n),
            HS((size_t)hm * n, -3.0), HY((size_t)hm * n, -3.0);
        precond_solve(n, Z.data(), g.data(), fixed.data(), k[1] != 0.0 ? lo.data() : nullptr, k[2] != 0.0 ? hi.data() : nullptr, k[3], k[4], k[5], k[6],
                      max_iter, apply, cnt, S.data(), Y.data(), m, harvest, HS.data(), HY.data(), p.data(), info.data(), trace.data(), es.data(),
                      zp.data());
        print_vector("loop_p", p.data(), p.size());
        print_vector("loop_info", info.data(), info.size());
        print_vector("loop_trace", trace.data(), trace.size());
        print_vector("loop_states", es.data(), es.size());
        print_vector("loop_zp", zp.data(), zp.size());
        // the pairs the harvest left, oldest first
        const long long taken = (long long)info[13], kept = taken < m ? taken : m, first = taken > m ? taken % m : 0;
        printf("loop_pairs");
        for (long long q = 0; q < kept; ++q) {
            const size_t slot = (size_t)((first + q) % m);
            for (long long i = 0; i < n; ++i) printf(" %016llx", bits(HS[slot * n + i]));
            for (long long i = 0; i < n; ++i) printf(" %016llx", bits(HY[slot * n + i]));
        }
        printf("\n");
        // an empty store: newton_box_solve's bits
        std::vector<double> p2((size_t)n), i2(NEWTON_BOX_INFO), t2((size_t)(NEWTON_BOX_TRACE * max_iter), -7.0), es2((size_t)n), zp2((size_t)n);
        newton_box_solve(n, Z.data(), g.data(), fixed.data(), k[1] != 0.0 ? lo.data() : nullptr, k[2] != 0.0 ? hi.data() : nullptr, k[3], k[4], k[5], k[6],
                         max_iter, apply, p2.data(), i2.data(), t2.data(), es2.data(), zp2.data());
        print_vector("box_p", p2.data(), p2.size());
        print_vector("box_info", i2.data(), i2.size());
        print_vector("box_trace", t2.data(), t2.size());
        print_vector("box_states", es2.data(), es2.size());
        print_vector("box_zp", zp2.data(), zp2.size());
    }
    fclose(f);
    printf("sizes %d %d %d %d %d %d %lld %lld\n", PRECOND_SLOTS, PRECOND_STATE, PRECOND_INFO, PRECOND_TRACE, PRECOND_PC, PRECOND_MAX_PAIRS,
           (long long)precond_workspace_doubles(11610, 8), (long long)precond_store_doubles(530000, 16));
    printf("eps %016llx\n", bits(PRECOND_EPS));
    return 0;
}
""".replace("RANK", str(RANK))


# ------------------------------------------------------------------------------------------------------------ the systems
def system(n, seed):
    """a positive definite operator with a spread diagonal (condition about 20 with the shift) and three rank-one terms"""
    rng = np.random.default_rng(seed)
    dg = 10.0 ** rng.uniform(-0.5, 0.5, n)
    U = rng.standard_normal((RANK, n)) / math.sqrt(n)
    coef = np.array([5.0, 2.0, 0.5])
    Z, g = rng.standard_normal(n), rng.standard_normal(n)
    fixed = np.zeros(n)
    if n > 10:
        fixed[rng.choice(n, n // 8, replace=False)] = 1.0
    return dict(n=n, dg=dg, U=U, coef=coef, Z=Z, g=g, fixed=fixed)


def product_of(sy):
    def product(d):
        y = sy["dg"] * d
        for r in range(RANK):
            t = sy["coef"][r] * dot(sy["U"][r], d)
            y = y + t * sy["U"][r]
        return y
    return product


def pairs_of(sy, count, seed, shift):
    """pairs (s, A s + shift s) of random directions: positive curvature"""
    rng = np.random.default_rng(seed)
    prod = product_of(sy)
    S = [rng.standard_normal(sy["n"]) for _ in range(count)]
    return S, [prod(s) + shift * s for s in S]


def runs():
    """dicts: the system, the keywords of the loop, the pairs, m, harvest, and what the run is there for"""
    out = []

    def add(what, sy, S, Y, m, harvest=0, lo=None, hi=None, **kw):
        n = sy["n"]
        kw = dict(dict(radius=0.0, shift=0.5, rtol=1e-8, atol=0.0, max_iter=80), **kw)
        out.append(dict(what=what, sy=sy, S=S, Y=Y, m=m, harvest=harvest, lo=lo, hi=hi, kw=kw, n=n))

    for n, seed in ((5, 1), (257, 2), (16500, 3)):
        sy = system(n, seed)
        add(f"n{n}_empty", sy, [], [], 8, harvest=1)                                   # an empty store; harvests fewer than m pairs at n = 5
        for m in ((1, 3) if n == 5 else (1, 3, 8, 16) if n == 257 else (8, 16)):
            S, Y = pairs_of(sy, m, 10 * seed + m, 0.5)
            add(f"n{n}_m{m}", sy, S, Y, m)
    sy = system(257, 2)
    S, Y = pairs_of(sy, 8, 77, 0.5)
    add("harvest_wraps", sy, S[:3], Y[:3], 3, harvest=1)                               # more than m pairs taken: the ring wraps
    add("rejected_middle", sy, S[:2] + [S[2]] + S[3:5], Y[:2] + [-Y[2]] + Y[3:5], 8)   # s . y < 0 in the middle
    add("all_rejected", sy, S[:4], [-y for y in Y[:4]], 8)
    add("max_iter_3", sy, S, Y, 8, harvest=1, max_iter=3)
    rng = np.random.default_rng(5)
    wide = (sy["Z"] - 0.6 - 1.5 * rng.random(257), sy["Z"] + 0.6 + 1.5 * rng.random(257))
    add("box_hits", sy, S, Y, 8, harvest=1, lo=wide[0], hi=wide[1])                     # entries reach bounds: F shrinks, restarts with -z
    add("box_radius", sy, S, Y, 8, lo=wide[0], hi=wide[1], radius=0.5)
    add("indefinite", sy, S, Y, 8, harvest=1, lo=sy["Z"] - 1.0, hi=sy["Z"] + 1.0, shift=-3.0)   # negative curvature: pairs not taken
    # a forced fallback behind the start: gamma = s . y / y . y = 1e306 and |g| = 1e3, so gamma * r overflows and rz is no finite number
    e = np.zeros(257)
    free = np.flatnonzero(sy["fixed"] == 0.0)
    e[free[:2]] = 0.6
    big = dict(sy, g=1e3 * sy["g"])
    add("fallback_start", big, [1e153 * e], [1e-153 * e], 8, harvest=1)
    add("fallback_start_plain", big, [], [], 8)
    return out


RUNS = runs()


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("precond_plan")
    src, exe, data = str(tmp / "plan.cpp"), str(tmp / "plan"), str(tmp / "data.bin")
    with open(src, "w") as f:
        f.write(PROGRAM)
    with open(data, "wb") as f:
        f.write(struct.pack("q", len(RUNS)))
        for r in RUNS:
            sy, kw, n = r["sy"], r["kw"], r["n"]
            lo = np.full(n, -INF) if r["lo"] is None else r["lo"]
            hi = np.full(n, INF) if r["hi"] is None else r["hi"]
            head = [n, r["lo"] is not None, r["hi"] is not None, kw["radius"], kw["shift"], kw["rtol"], kw["atol"], kw["max_iter"], len(r["S"]), r["m"],
                    r["harvest"]]
            f.write(np.array(head, dtype=np.float64).tobytes())
            for a in (sy["dg"], sy["U"], sy["coef"], sy["Z"], sy["g"], sy["fixed"], lo, hi, *r["S"], *r["Y"]):
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe], check=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    out = {}
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "sizes":
            out["sizes"] = tuple(int(v) for v in w[1:])
        elif w[0] in ("admitted", "eps"):
            out.setdefault(w[0], []).append(w[1:])
        else:
            out.setdefault(w[0], []).append(np.array([int(v, 16) for v in w[1:]], dtype=np.uint64).view(np.float64))
    return out


@pytest.fixture(scope="module")
def restated():
    """the NumPy loop of every run, once"""
    out = []
    for r in RUNS:
        sy = r["sy"]
        nonfixed = sy["fixed"] == 0.0
        with np.errstate(over="ignore", invalid="ignore"):      # the forced fallback overflows on purpose
            out.append(restate(r, sy, nonfixed))
    return out


def restate(r, sy, nonfixed):
    loop = PC.precond_loop(product_of(sy), sy["g"], nonfixed, sy["Z"], r["S"], r["Y"], lo=r["lo"], hi=r["hi"], harvest=bool(r["harvest"]), **r["kw"])
    box = B.box_loop(product_of(sy), sy["g"], nonfixed, sy["Z"], lo=r["lo"], hi=r["hi"], **r["kw"])
    return dict(loop=loop, box=box, z=PC.precondition_restated(r["S"], r["Y"], sy["g"], nonfixed), prep=PC.prepare_restated(r["S"], r["Y"], nonfixed))


def same(a, b):
    return a.shape == np.shape(b) and np.array_equal(a, b, equal_nan=True)


def by_name(what):
    return next(i for i, r in enumerate(RUNS) if r["what"] == what)


# ---------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("i", range(len(RUNS)), ids=[r["what"] for r in RUNS])
def test_the_application_is_the_restatement_bit_for_bit(printed, restated, i):
    r, want = RUNS[i], restated[i]
    q, gamma, rz = printed["admitted"][i]
    assert int(q) == len(want["prep"]["idx"])
    assert struct.unpack("d", struct.pack("Q", int(gamma, 16)))[0] == want["prep"]["gamma"]
    assert same(printed["apply_z"][i], want["z"]), r["what"]
    nonfixed = r["sy"]["fixed"] == 0.0
    assert np.all(printed["apply_z"][i][~nonfixed] == 0.0)


@pytest.mark.parametrize("i", range(len(RUNS)), ids=[r["what"] for r in RUNS])
def test_precond_solve_is_the_restated_loop_bit_for_bit(printed, restated, i):
    r, want = RUNS[i], restated[i]["loop"]
    n, max_iter = r["n"], r["kw"]["max_iter"]
    info = printed["loop_info"][i]
    k = int(info[1])
    print(r["what"], "status", int(info[0]), "iterations", k, "box iterations", int(restated[i]["box"]["info"][1]), "admitted", int(info[12]),
          "taken", int(info[13]), "fallbacks", int(info[14]), "hits", int(info[9]), "restarts", int(info[10]))
    assert same(printed["loop_p"][i], want["p"]) and same(info, want["info"]), (r["what"], info, want["info"])
    trace = printed["loop_trace"][i].reshape(max_iter, 8)
    assert same(trace[:k], want["trace"]) and np.all(trace[k:] == -7.0), "rows past the last iteration are left as they are"
    assert same(printed["loop_states"][i], want["states"]) and same(printed["loop_zp"][i], want["Zp"])
    kept = want["pairs"][-r["m"]:]
    flat = np.concatenate([np.concatenate([d, w]) for d, w in kept]) if kept else np.zeros(0)
    assert same(printed["loop_pairs"][i], flat), "the harvest leaves the loop's (d, w), oldest first"
    assert info[13] == len(want["pairs"]) and (r["harvest"] or info[13] == 0)


@pytest.mark.parametrize("i", range(len(RUNS)), ids=[r["what"] for r in RUNS])
def test_the_programs_box_solve_is_the_box_loop(printed, restated, i):
    want, max_iter = restated[i]["box"], RUNS[i]["kw"]["max_iter"]
    k = int(want["info"][1])
    assert same(printed["box_p"][i], want["p"]) and same(printed["box_info"][i], want["info"])
    assert same(printed["box_trace"][i].reshape(max_iter, 6)[:k], want["trace"])


def test_an_empty_store_or_no_admitted_pair_is_newton_box_solve_bit_for_bit(printed):
    seen = 0
    for i, r in enumerate(RUNS):
        if r["S"] and r["what"] != "all_rejected":
            continue
        seen += 1
        max_iter = r["kw"]["max_iter"]
        assert same(printed["loop_p"][i], printed["box_p"][i]) and same(printed["loop_info"][i][:12], printed["box_info"][i]), r["what"]
        assert same(printed["loop_trace"][i].reshape(max_iter, 8)[:, :6], printed["box_trace"][i].reshape(max_iter, 6))
        assert same(printed["loop_states"][i], printed["box_states"][i]) and same(printed["loop_zp"][i], printed["box_zp"][i])
        k = int(printed["loop_info"][i][1])
        tr = printed["loop_trace"][i].reshape(max_iter, 8)[:k]
        assert np.array_equal(tr[:, 6], tr[:, 3]) and np.all(tr[:, 7] == 0.0), "rz = rr bit for bit, the preconditioner is off"
        assert printed["loop_info"][i][12] == 0.0 and printed["loop_info"][i][14] == 0.0
        assert printed["loop_info"][i][15] == printed["loop_info"][i][2], "sqrt(rz0) = sqrt(rr0)"
    assert seen == 5


def test_what_the_runs_are_there_for(printed, restated):
    info = lambda what: printed["loop_info"][by_name(what)]
    for n in (257, 16500):
        for m in (8, 16):
            pre, plain = info(f"n{n}_m{m}"), info(f"n{n}_empty")
            assert pre[0] == plain[0] == CONVERGED and pre[12] == m and pre[14] == 0, "every pair (s, A s) is admitted"
    assert info("n5_empty")[13] < 8 and info("n5_empty")[13] >= 1, "a harvest that takes fewer than m pairs"
    assert info("harvest_wraps")[13] > 3, "more pairs taken than the ring holds"
    assert info("rejected_middle")[12] == 4 and restated[by_name("rejected_middle")]["prep"]["idx"] == [0, 1, 3, 4]
    assert info("all_rejected")[12] == 0
    assert info("max_iter_3")[0] == MAX_ITER and info("max_iter_3")[13] == 3
    assert info("box_hits")[9] >= 3 and info("box_hits")[10] >= 1 and info("box_hits")[0] == CONVERGED
    assert info("indefinite")[13] < info("indefinite")[1], "an iteration with kappa <= 0 offers no pair"
    fb, plain = by_name("fallback_start"), by_name("fallback_start_plain")
    assert info("fallback_start")[12] == 1 and info("fallback_start")[14] == 1 and info("fallback_start")[0] == CONVERGED
    assert same(printed["loop_p"][fb], printed["loop_p"][plain]), "behind the fallback the solve is the plain one"
    assert np.all(printed["loop_trace"][fb].reshape(-1, 8)[:int(info("fallback_start")[1]), 7] == 0.0)


def test_sizes_and_the_admission_bar(printed):
    slots, state, n_info, n_trace, pc, cap, work, store = printed["sizes"]
    assert (slots, state, n_info, n_trace, pc, cap) == (13, 24, 16, 8, 2 + 16 + 512, 16)
    nb = -(-11610 // 256)
    assert work == 4 * 11610 + (13 + 16 + 8 * 9 + 8) * nb + 24 + 530 + (11610 + 7) // 8
    assert store == 2 * 2 * 16 * 530000 and store * 8 / 1e6 == pytest.approx(271.36)
    assert int(printed["eps"][0][0], 16) == struct.unpack("Q", struct.pack("d", PC.EPS))[0] and PC.EPS == 2.0 ** -26
    plan = open(os.path.join(CSRC, "dto_precond_plan.h")).read()
    import re
    assert '#include "dto_newton_box_plan.h"' in plan and "hip" not in re.sub(r"//.*", "", plan).lower().replace("__hipcc__", "")
