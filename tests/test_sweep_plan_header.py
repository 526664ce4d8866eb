"""csrc/dto_sweep_plan.h from plain C++: a stand-alone program is compiled with g++ (address and undefined-behaviour sanitizers on)
against the header alone (no HIP, no engine header), run without a GPU, and what it prints is checked.

a. Step budget.  The program restates, verbatim, the two texts the header replaced -- the host's chain (taylor_budget, plan_sweep,
   cheap_plan with its 199-index hump loop, run_sweep's tc rule: dto_engine.cpp) and the body of k_plan_dev (dto_sweep_fused.hip, its
   own budget lambda, the literal 9.0, the three-index hump) -- and compares both with the header's device_plan and with the host
   path resolved through the header (cheap_plan(loose), else plan_sweep, then sweep_tc) on every point of a grid.
b. Launch shapes.  A table of the three planners' outputs, every field.  The expected values were printed by the planners of the
   library built from the commit before the header existed (they touch no device), never by the header.
c. Form choice.  One row per rule of choose_sweep; the expected forms are those the GPU tests assert through the profile counters
   (cited per row).
d. Kernel instantiations.  A second program walks choose_sweep over every shape the callbacks can ask for and prints each
   (form, instantiation) it names, and the header's four lists (the X-macros prepare and launch read): the two sets must be equal in
   the product build, and under the pins of tests/test_gpu_sweep_forms.py (-DDTO_TUNING) nothing outside the lists may appear."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")

# (npad, drives, type set, intervals, CUs, shared_chip) -> fused plan, cluster plan, generator-stationary plan ("0": refused; None:
# not asked -- the cluster and generator-stationary planners do not read shared_chip).  Type sets: 0 the p column alone, 1 first
# order (p, d^j), 2 second order (p, d^j, h^{ij}), 3 first order plus one more p column (the J w product's exp(A) w_x).
#   fused:   ok MT NT ipw nslot nblocks WC WK S64 NX lds_bytes
#   cluster: ok MT NT R ipw n_groups n_clusters nblocks lds_bytes step_us workspace_doubles
#   gs:      ok KU MP NT ipw has_src n_groups n_clusters nblocks cap lds_bytes term_us norm_doubles
SHAPES = [
    ((256, 4, 1, 1999, 256, 0), "1 4 3 9 1 223 1 2 0 0 95272", "1 2 2 2 6 334 128 256 83968 47.074666666666666 2162688", "1 8 5 2 6 1 334 32 256 66 140560 152.17200000000003 513024"),
    ((256, 4, 1, 1999, 256, 1), "1 4 2 12 1 167 2 1 0 0 126856", None, None),
    ((256, 4, 0, 1999, 256, 0), "0", "1 1 2 4 32 63 64 256 83968 25.583466666666666 1081344", "1 8 5 2 32 0 63 32 256 64 140464 25.618181818181817 96768"),
    ((256, 4, 2, 1999, 256, 0), "1 4 3 3 5 667 1 2 0 0 95344", "1 2 2 2 2 1000 128 256 83968 47.074666666666666 2162688", "1 8 5 2 2 1 1000 32 256 64 140464 442.68218181818185 1536000"),
    ((256, 4, 3, 1999, 256, 0), "1 4 3 8 1 250 1 2 0 0 101544", "1 1 2 4 5 400 64 256 83968 25.583466666666666 1081344", "1 8 5 2 5 1 400 32 256 65 140512 179.83963636363634 614400"),
    ((256, 4, 1, 249, 256, 0), "0", "1 1 2 4 6 42 48 192 83968 25.583466666666666 811008", "1 8 5 1 3 1 83 32 256 9 83968 24.463636363636361 63744"),
    ((256, 4, 1, 249, 256, 1), "0", None, None),
    ((256, 2, 1, 999, 256, 0), "1 4 1 5 1 200 1 2 0 0 32048", "1 2 2 2 10 100 104 208 83968 29.881706666666666 1757184", "1 8 3 2 10 1 100 32 256 40 137904 36.341818181818184 153600"),
    ((256, 1, 1, 39, 256, 0), "0", "1 1 1 4 8 5 8 32 83968 9.5262933333333351 67584", "1 8 3 1 8 1 5 8 64 8 83968 10.861818181818181 3840"),
    ((256, 5, 1, 999, 256, 0), "1 4 2 5 1 200 1 2 0 0 63712", "1 2 2 2 5 200 128 256 83968 55.671146666666665 2162688", "0"),
    ((256, 4, 1, 1999, 32, 0), "1 4 3 9 1 223 1 2 0 0 95272", "1 2 2 2 6 334 16 32 83968 47.074666666666666 270336", "0"),
    ((256, 2, 0, 1, 256, 0), "0", "1 1 1 4 16 1 8 32 83968 12.516373333333336 67584", "1 8 3 1 16 0 1 8 64 16 83968 11.792727272727273 768"),
    ((256, 2, 2, 249, 256, 0), "0", "1 1 2 4 5 50 56 224 83968 16.986986666666667 946176", "1 8 3 2 5 1 50 32 256 10 136944 18.170909090909092 76800"),
    ((256, 1, 1, 1999, 256, 1), "1 4 1 8 1 250 1 2 0 0 34136", None, None),
    ((256, 4, 1, 39, 32, 0), "0", "1 1 2 4 6 7 8 32 83968 25.583466666666666 135168", "0"),
    ((256, 5, 0, 249, 256, 0), "0", "1 1 1 4 16 16 16 64 83968 21.486613333333338 135168", "0"),
    ((128, 2, 1, 999, 256, 0), "1 2 1 5 1 200 1 1 0 0 16688", "1 1 2 2 10 100 104 208 83968 9.9934933333333333 905216", "1 4 3 2 10 1 100 64 256 20 83968 12.585454545454546 76800"),
    ((128, 2, 1, 999, 256, 1), "1 2 1 5 1 200 1 1 0 0 16688", None, None),
    ((128, 4, 1, 249, 256, 0), "0", "1 1 1 2 3 83 88 176 83968 10.748266666666666 382976", "1 4 5 1 3 1 83 64 256 6 83968 11.654545454545454 31872"),
    ((128, 1, 0, 1999, 256, 0), "0", "1 1 1 2 16 125 128 256 83968 6.2631466666666675 557056", "1 4 3 1 16 0 125 64 256 32 83968 8.8618181818181814 48000"),
    ((128, 5, 2, 999, 256, 0), "1 2 3 2 6 500 1 1 0 0 46232", "1 1 2 2 1 999 128 256 83968 16.440853333333333 1114112", "0"),
    ((128, 2, 3, 39, 256, 0), "0", "1 1 1 2 4 10 16 32 83968 7.7581866666666679 69632", "1 4 3 1 4 1 10 16 64 4 83968 10.396363636363636 3840"),
    ((128, 2, 1, 1, 32, 0), "0", "1 1 1 2 5 1 8 16 83968 7.7581866666666679 34816", "1 4 3 1 5 1 1 8 32 5 83968 10.396363636363636 384"),
    ((128, 4, 2, 1999, 256, 0), "1 2 3 3 5 667 1 1 0 0 49264", "1 1 2 2 2 1000 128 256 83968 14.291733333333333 1114112", "1 4 5 2 2 1 1000 64 256 32 83968 140.91054545454546 768000"),
    ((128, 4, 1, 1999, 32, 1), "1 2 3 9 1 223 1 1 0 0 49192", None, None),
    ((64, 2, 1, 999, 256, 0), "1 1 1 4 1 250 1 1 1 1 75248", "0", "0"),
    ((64, 2, 1, 999, 256, 1), "1 1 1 5 1 200 1 1 1 1 75280", None, None),
    ((64, 4, 1, 1999, 256, 0), "1 1 1 3 1 667 1 1 1 1 75336", "0", "0"),
    ((64, 5, 1, 999, 256, 0), "1 1 1 2 1 500 1 1 0 0 7384", "0", "0"),
    ((64, 2, 0, 39, 256, 1), "1 1 1 16 0 3 1 1 1 0 75560", None, None),
    ((64, 4, 2, 999, 256, 0), "1 1 1 1 5 999 1 1 1 2 75600", "0", "0"),
    ((64, 5, 2, 249, 256, 0), "1 1 2 1 6 249 1 1 0 0 12912", "0", "0"),
    ((64, 1, 3, 1, 32, 0), "1 1 1 1 1 1 1 1 1 1 75144", "0", "0"),
    ((64, 2, 1, 1999, 32, 0), "1 1 1 5 1 400 1 1 1 1 75280", "0", "0"),
    ((192, 2, 1, 999, 256, 0), "0", "0", "0"),
    ((192, 4, 0, 249, 256, 0), "0", "0", "0"),
    # (512 states: the cluster planner answers for 128 and 256 states alone)
    ((512, 2, 1, 999, 256, 0), "0", "0", "0"),
    ((512, 4, 1, 249, 256, 0), "0", "0", "0"),
    ((512, 1, 0, 1999, 256, 1), "0", None, None),
    ((512, 4, 2, 39, 32, 0), "0", "0", "0"),
]

# label -> form.  Situation fields not named by a row: 256 CUs, sweep_form 0, no reuse, not frozen, a term store of 80 terms, q = 1,
# d_ub = 40, no store, chip not shared, not step_only; Kpad as dto_create sizes it (intervals rounded up to 128, at 64 and 192
# states to 64).
FORMS = [
    # tests/test_gpu_sweep_forms.py::test_gs_coefficient_table_at_the_lds_limit, test_gs_rounds_and_ragged_groups (eval_constraint)
    ("single_column_256", "gs"),
    # DESIGN.md section 4 (the headline Jacobian sweep, alone and beside the chain); the shapes are rows 1 and 2 of SHAPES
    ("headline_alone", "fused"),
    ("headline_shared", "fused"),
    # tests/test_gpu_cluster_sweep.py::test_short_horizons_take_the_gs_form, test_gs_sweep_on_shards (alone);
    # beside another stream's kernels the generator-stationary form is out and the fused planner refuses: cluster
    ("shard_249_alone", "gs"),
    ("shard_249_shared", "cluster"),
    # tests/test_gpu_states64.py::test_forms_against_the_oracle_and_the_general_forms
    ("states_64", "s64"),
    ("states_64_single_column", "s64"),
    # tests/test_gpu_sweep_forms.py::test_gs_edge_shapes[n129-step]
    ("states_192", "step"),
    # tests/test_gpu_cluster_sweep.py::test_cluster_sweep_matches_the_oracle_and_the_step_form (Jacobian; eval_constraint: step)
    ("two_rounds_256x249", "cluster"),
    ("two_rounds_single_column", "step"),
    # tests/test_gpu_sweep_forms.py::run_case (the sweep_form = 1 handle of every case)
    ("option_step", "step"),
    # tests/test_gpu_edge_cases.py::test_reuse_forward_sweep_between_callbacks (the frozen sweep is step-per-launch)
    ("frozen", "step"),
    # tests/test_gpu_edge_cases.py::test_reuse_forward_sweep_runs_no_sweep_it_has_cached ('g Jw g': the product's sweep is 'step')
    ("step_only", "step"),
    # tests/test_gpu_edge_cases.py::test_reuse_takes_the_chains_step_budget_where_the_cheap_bound_is_not_enough
    ("store_too_shallow", "step"),
    ("store_deep_enough", "fused"),
    ("store_without_term_store", "step"),
    # tests/test_gpu_edge_cases.py::test_reuse_forward_sweep_runs_no_sweep_it_has_cached (option on: 'g g' -> 'step 0')
    ("stored_single_column_reuse", "step"),
    ("stored_single_column_no_reuse", "gs"),
    # 128 states (clusters of 4: the planner itself would still find 8 clusters on 63 CUs).  With 64 CUs:
    # tests/test_gpu_sweep_forms.py::test_gs_instances; below 64 the form is out: a single column falls to step (no other form takes
    # one), a 39-interval shard, which the fused planner refuses (8 workgroups), to cluster
    ("cus_64_single_column", "gs"),
    ("cus_63_single_column", "step"),
    ("cus_64_shard", "gs"),
    ("cus_63_shard", "cluster"),
    # launch_sweep_gs refuses a slab of 2^31 bytes or more (32-bit buffer offsets), so choose_sweep must not pick the form there: a
    # single column of 2^20 intervals at 256 states is exactly 2^31 bytes (and on enough CUs for one round, which the planner accepts)
    ("slab_below_2_31", "gs"),
    ("slab_of_2_31", "step"),
    # 512 states: tests/test_gpu_large_states.py runs them on the step form (the cluster form measured slower there)
    ("states_512", "step"),
]

PROGRAM = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include "dto_sweep_plan.h"
using namespace dto;

// ---------------------------------------------------------------- a. the two texts the header replaced, verbatim
namespace parent {
struct SweepPlan {
    int q, d_ub;
    int tc = -1;
};
int taylor_budget(double br) {
    int t = 8;
    double term = 1.0;
    for (int i = 1; i <= t; ++i) term *= br / i;
    while (term > 1e-19 && t < 200) { ++t; term *= br / t; }
    return t + 6;
}
SweepPlan plan_sweep(double beta) {
    SweepPlan p{1, 12};
    if (!(beta == beta) || beta > 1e6) {
        p.q = 1; p.d_ub = 30;
        return p;
    }
    static const double theta_v = 9.0;
    p.q = std::max(1, (int)std::ceil(beta / theta_v));
    p.d_ub = taylor_budget(beta / p.q);
    return p;
}
struct Bounds {
    double beta, b1;
};
bool cheap_plan(const Bounds& bd, bool loose, SweepPlan& out) {
    out = plan_sweep(bd.beta);
    if (out.q == 1) return true;
    if (loose && bd.beta == bd.beta && bd.beta < 40.0) {
        double lh = 0.0;
        for (int k = 1; k < 200; ++k) lh = std::max(lh, k * std::log(bd.beta) - std::lgamma(k + 1.0));
        if (lh <= 9.0) {
            SweepPlan p{1, taylor_budget(bd.beta)};
            p.tc = std::min(p.d_ub / 2 - 1, std::max(2, (int)std::ceil(bd.beta) + 4));
            out = p;
            return true;
        }
    }
    return false;
}
// the host's path to {q, d_ub, tc} from the cheap bound alone: cheap_plan(loose), else plan_sweep, then run_sweep's tc rule
void host_chain(double beta, int out[3]) {
    SweepPlan plan;
    if (!cheap_plan(Bounds{beta, beta}, true, plan)) plan = plan_sweep(beta);
    const int tc_env = -1;
    int tc = tc_env >= 0 ? tc_env : (plan.tc >= 0 ? plan.tc : plan.d_ub / 2 - 1);
    if (tc < 2) tc = 0;
    out[0] = plan.q; out[1] = plan.d_ub; out[2] = tc;
}
// k_plan_dev's body
void k_plan_dev(double beta, int out[3]) {
    auto budget = [](double br) {
        int t = 8;
        double term = 1.0;
        for (int i = 1; i <= t; ++i) term *= br / i;
        while (term > 1e-19 && t < 200) { ++t; term *= br / t; }
        return t + 6;
    };
    int q = 1, d_ub = 30, tc = -1;
    if (beta == beta && beta <= 1e6) {
        q = (int)ceil(beta / 9.0);
        if (q < 1) q = 1;
        d_ub = budget(beta / q);
        if (q > 1 && beta < 40.0) {
            double lh = 0.0;
            const int k0 = (int)floor(beta);
            for (int k = (k0 > 1 ? k0 - 1 : 1); k <= k0 + 1; ++k) lh = fmax(lh, k * log(beta) - lgamma(k + 1.0));
            if (lh <= 9.0) {
                q = 1;
                d_ub = budget(beta);
                const int a0 = d_ub / 2 - 1, a1 = (int)ceil(beta) + 4;
                tc = a0 < (a1 > 2 ? a1 : 2) ? a0 : (a1 > 2 ? a1 : 2);
            }
        }
    }
    if (tc < 0) tc = d_ub / 2 - 1;
    if (tc < 2) tc = 0;
    out[0] = q; out[1] = d_ub; out[2] = tc;
}
}  // namespace parent

static long n_points = 0, n_differ = 0;
static void budget_point(double beta) {
    int host[3], dev[3];
    parent::host_chain(beta, host);
    parent::k_plan_dev(beta, dev);
    const SweepPlan d = device_plan(beta, 9.0);
    SweepPlan r;
    if (!cheap_plan(beta, true, 9.0, r)) r = plan_sweep(beta, 9.0);
    r.tc = sweep_tc(r);
    ++n_points;
    const bool same = host[0] == dev[0] && host[1] == dev[1] && host[2] == dev[2] && d.q == host[0] && d.d_ub == host[1] && d.tc == host[2] &&
                      r.q == host[0] && r.d_ub == host[1] && r.tc == host[2];
    if (!same) {
        ++n_differ;
        printf("differ %.17g host %d %d %d k_plan_dev %d %d %d device_plan %d %d %d resolved %d %d %d\n", beta, host[0], host[1], host[2],
               dev[0], dev[1], dev[2], d.q, d.d_ub, d.tc, r.q, r.d_ub, r.tc);
    }
}
static void budget() {
    for (int i = 0; i <= 60 * 1024; ++i) budget_point(i / 1024.0);
    for (int k = 1; k <= 60; ++k) {
        budget_point(std::nextafter((double)k, 0.0));
        budget_point((double)k);
        budget_point(std::nextafter((double)k, 1e9));
    }
    const double inf = std::numeric_limits<double>::infinity();
    for (double b : {std::numeric_limits<double>::quiet_NaN(), inf, 1e6, std::nextafter(1e6, inf), 1e-300, 1e5}) budget_point(b);
    printf("budget points %ld differ %ld\n", n_points, n_differ);
    for (double b : {11.07, 11.125, 11.25, 0.0, 9.0, 1e5}) {
        const SweepPlan p = device_plan(b, 9.0);
        printf("plan %.17g %d %d %d\n", b, p.q, p.d_ub, p.tc);
    }
    // the pieces that have no second text: the tc override, plan_hump's arithmetic, the growth rate
    printf("tc %d %d %d %d\n", sweep_tc(SweepPlan{1, 66}), sweep_tc(SweepPlan{1, 66, 16}), sweep_tc(SweepPlan{1, 66, 16}, 5), sweep_tc(SweepPlan{1, 5}));
    const double logH[4] = {12.5, 9.5, 8.75, 3.0};
    const int kend[4] = {50, 41, 33, 198};
    const SweepPlan h1 = plan_hump(true, logH, kend, 9.0, 20.0), h2 = plan_hump(false, logH, kend, 9.0, 20.0), h3 = plan_hump(true, logH, kend, 2.0, 20.0),
                    h4 = plan_hump(true, logH, kend, 3.5, 20.0), ps = plan_sweep(20.0, 9.0), p2 = plan_sweep(20.0, 2.0);
    printf("hump %d %d %d  %d %d %d  %d %d %d  %d %d %d  sweep %d %d  %d %d\n", h1.q, h1.d_ub, h1.tc, h2.q, h2.d_ub, h2.tc, h3.q, h3.d_ub, h3.tc,
           h4.q, h4.d_ub, h4.tc, ps.q, ps.d_ub, p2.q, p2.d_ub);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    printf("growth %g %g %d %d\n", growth_rate(9.5, 7.25), growth_rate(7.25, 9.5), (int)std::isnan(growth_rate(9.5, nan)), (int)std::isnan(growth_rate(nan, 9.5)));
}

// ---------------------------------------------------------------- b. launch shapes
static SweepTypes type_set(int m, int set) {
    SweepTypes ty = make_types(set == 0 ? 0 : m, set == 2);
    if (set == 3) ty.t[ty.T++] = TypeDesc{0, {0, 0}, {0, 0}, {0, 0}};
    return ty;
}
static void shape(int npad, int m, int set, long n_int, int n_cu, int sh) {
    const SweepTypes ty = type_set(m, set);
    FusedSweepPlan f{};
    printf("F %d %d %d %ld %d %d :", npad, m, set, n_int, n_cu, sh);
    if (sweep_fused_plan(npad, m, ty, n_int, n_cu, f, sh != 0))
        printf(" 1 %d %d %d %d %d %d %d %d %d %zu\n", f.MT, f.NT, f.ipw, f.nslot, f.nblocks, f.WC, f.WK, f.S64, f.NX, f.lds_bytes);
    else printf(" 0\n");
    if (sh) return;
    ClusterSweepPlan c{};
    printf("C %d %d %d %ld %d %d :", npad, m, set, n_int, n_cu, sh);
    if (sweep_cluster_plan(npad, m, ty, n_int, n_cu, c))
        printf(" 1 %d %d %d %d %d %d %d %zu %.17g %zu\n", c.MT, c.NT, c.R, c.ipw, c.n_groups, c.n_clusters, c.nblocks, c.lds_bytes, c.step_us,
               sweep_cluster_workspace_doubles(npad, c));
    else printf(" 0\n");
    GsSweepPlan g{};
    printf("G %d %d %d %ld %d %d :", npad, m, set, n_int, n_cu, sh);
    if (sweep_gs_plan(npad, m, ty, n_int, n_cu, g))
        printf(" 1 %d %d %d %d %d %d %d %d %d %zu %.17g %zu\n", g.KU, g.MP, g.NT, g.ipw, g.has_src, g.n_groups, g.n_clusters, g.nblocks, g.cap,
               g.lds_bytes, g.term_us, sweep_gs_norm_doubles(g));
    else printf(" 0\n");
}

// ---------------------------------------------------------------- c. form choice
static SweepSituation situation(int npad, int m, int set, long n_int) {
    SweepSituation s{};
    const int TN = npad % 128 == 0 ? 128 : 64;
    s.npad = npad; s.Kpad = (int)((n_int + TN - 1) / TN * TN); s.m = m;
    s.types = type_set(m, set);
    s.n_int = n_int; s.n_cu = 256;
    s.has_term_store = true; s.dcap = 80;
    s.q = 1; s.d_ub = 40;
    return s;
}
static void form(const char* label, const SweepSituation& s) {
    static const char* names[5] = {"gs", "fused", "s64", "cluster", "step"};
    const SweepChoice c = choose_sweep(s);
    printf("form %s %s %d %d\n", label, names[c.form], (int)c.store, (int)c.shared_chip);
}
static void forms() {
    SweepSituation s = situation(256, 4, 0, 1999);               form("single_column_256", s);
    s = situation(256, 4, 1, 1999);                              form("headline_alone", s);
    s.shared_chip = true;                                        form("headline_shared", s);
    s = situation(256, 4, 1, 249);                               form("shard_249_alone", s);
    s.shared_chip = true;                                        form("shard_249_shared", s);
    s = situation(64, 2, 1, 999);                                form("states_64", s);
    s = situation(64, 2, 0, 999);                                form("states_64_single_column", s);
    s = situation(192, 2, 1, 999);                               form("states_192", s);
    s = situation(256, 4, 1, 249); s.q = 2;                      form("two_rounds_256x249", s);
    s = situation(256, 4, 0, 249); s.q = 2;                      form("two_rounds_single_column", s);
    s = situation(256, 4, 1, 1999); s.sweep_form = 1;            form("option_step", s);
    s = situation(256, 4, 1, 1999); s.frozen = true;             form("frozen", s);
    s = situation(256, 4, 1, 1999); s.step_only = true;          form("step_only", s);
    s = situation(256, 4, 1, 1999); s.store = true; s.d_ub = 80; form("store_too_shallow", s);
    s.d_ub = 79;                                                 form("store_deep_enough", s);
    s.has_term_store = false;                                    form("store_without_term_store", s);
    s = situation(256, 4, 0, 1999); s.store = true; s.reuse = true;   form("stored_single_column_reuse", s);
    s.reuse = false;                                             form("stored_single_column_no_reuse", s);
    s = situation(128, 2, 0, 999); s.n_cu = 64;                  form("cus_64_single_column", s);
    s.n_cu = 63;                                                 form("cus_63_single_column", s);
    s = situation(128, 2, 1, 39); s.n_cu = 64;                   form("cus_64_shard", s);
    s.n_cu = 63;                                                 form("cus_63_shard", s);
    s = situation(256, 4, 0, (1 << 20) - 128); s.n_cu = 300000;  form("slab_below_2_31", s);
    s = situation(256, 4, 0, 1 << 20); s.n_cu = 300000;          form("slab_of_2_31", s);
    s = situation(512, 4, 1, 499);                               form("states_512", s);
}

int main() {
    budget();
@SHAPES@
    forms();
    return 0;
}
"""


# ---------------------------------------------------------------- d. kernel instantiations
# The shapes: npad 64 .. 1024, 1 .. 7 drives, the four column-type sets of the callbacks (type_set above), store and shared_chip
# both ways, q = 1 and 2, EVERY interval count from 1 to 4000 (the planners' answers change at interval counts that depend on the
# type count and the CUs, so no coarser grid is argued for; a walk takes under two seconds) -- on 256 CUs, and once more on 48.
# The second CU count is there for k_sweep_cluster<2, 1, 2>: on 256 CUs four members with two tiles (124) or two members with two
# tiles (222) always cost less in sweep_cluster_plan's model, so that instance is reached only where four-member clusters are too
# few (fewer than 32 CUs) or too coarse (48 CUs: 8 clusters of 4 against 24 of 2) -- a partitioned chip -- and under the pins.
# Situation fields not walked: as in `situation` above.  The step form names its tile per launch: grid.y is the type count, or the
# generators of a split-K step / launch_apply_generators.
ENUM_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "dto_sweep_plan.h"
using namespace dto;

static SweepTypes type_set(int m, int set) {
    SweepTypes ty = make_types(set == 0 ? 0 : m, set == 2);
    if (set == 3) ty.t[ty.T++] = TypeDesc{0, {0, 0}, {0, 0}, {0, 0}};
    return ty;
}
int main(int argc, char** argv) {   // the CU counts to walk
    static const char* names[5] = {"gs", "fused", "s64", "cluster", "step"};
    static bool seen[2][5][1 << 16];   // [CU count][form][four numbers below 16]
    const int n_cus = argc - 1 < 2 ? argc - 1 : 2;
    int cus[2] = {0, 0};
    for (int ci = 0; ci < n_cus; ++ci) cus[ci] = atoi(argv[1 + ci]);
    for (int ci = 0; ci < n_cus; ++ci) {
        auto saw = [&](int form, int a, int b, int c, int d) { seen[ci][form][((a * 16 + b) * 16 + c) * 16 + d] = true; };
        for (int npad : {64, 128, 256, 512, 1024})
            for (int m = 1; m <= 7; ++m)
                for (int set = 0; set < 4; ++set) {
                    SweepSituation s{};
                    const int TN = npad % 128 == 0 ? 128 : 64;
                    s.npad = npad; s.m = m; s.types = type_set(m, set); s.n_cu = cus[ci];
                    s.has_term_store = true; s.dcap = 80; s.d_ub = 40;
                    for (int store = 0; store < 2; ++store)
                        for (int shared = 0; shared < 2; ++shared)
                            for (int q = 1; q <= 2; ++q)
                                for (long n_int = 1; n_int <= 4000; ++n_int) {
                                    s.Kpad = (int)((n_int + TN - 1) / TN * TN); s.n_int = n_int;
                                    s.store = store != 0; s.shared_chip = shared != 0; s.q = q;
                                    const SweepChoice c = choose_sweep(s);
                                    if (c.form == SWEEP_GS) saw(c.form, 0, 0, 0, 0);   // (k_sweep_gs keeps its list in dto_sweep_gs.hip)
                                    else if (c.form == SWEEP_FUSED) saw(c.form, c.fused.MT, c.fused.NT, c.fused.WC, c.fused.WK);
                                    else if (c.form == SWEEP_S64) saw(c.form, s64_generator_slots(m), c.fused.NX, 0, 0);
                                    else if (c.form == SWEEP_CLUSTER) saw(c.form, c.cluster.MT, c.cluster.NT, c.cluster.R, 0);
                                    else
                                        for (int ny : {s.types.T, m + 1}) saw(c.form, sweep_step_tile_rows(npad, s.Kpad, ny) / 16, 32 / 16, 0, 0);
                                }
                }
    }
    static const int count[5] = {0, 4, 2, 3, 2};   // numbers that name an instantiation of the form
    for (int ci = 0; ci < n_cus; ++ci)
        for (int form = 0; form < 5; ++form)
            for (int k = 0; k < (1 << 16); ++k) {
                if (!seen[ci][form][k]) continue;
                const int v[4] = {k >> 12, (k >> 8) & 15, (k >> 4) & 15, k & 15};
                printf("inst %d %s", cus[ci], names[form]);
                for (int i = 0; i < count[form]; ++i) printf(" %d", form == SWEEP_STEP ? 16 * v[i] : v[i]);
                printf("\n");
            }
#define F(MT, NT, WC, WK) printf("list fused %d %d %d %d\n", MT, NT, WC, WK);
    DTO_SWEEP_FUSED_INSTANCES(F)
#define S(MP, NX) printf("list s64 %d %d\n", MP, NX);
    DTO_SWEEP_S64_INSTANCES(S)
#define C(MT, NT, R) printf("list cluster %d %d %d\n", MT, NT, R);
    DTO_SWEEP_CLUSTER_INSTANCES(C)
#define K(TM, TN) printf("list step %d %d\n", TM, TN);
    DTO_SWEEP_STEP_TILES(K)
    return 0;
}
"""

# the pins of tests/test_gpu_sweep_forms.py (test_gs_instances_two_tiles, test_cluster_instances)
PINS = [{"DTO_GS_NT": "2"}] + [{"DTO_SWEEP_GS": "0", "DTO_CLUSTER_R": str(R), "DTO_CLUSTER_NT": str(NT)} for R in (2, 4) for NT in (1, 2)]


def _build(tmp, name, program, flags):
    src, exe = str(tmp / (name + ".cpp")), str(tmp / name)
    with open(src, "w") as f:
        f.write(program)
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe] + flags, check=True)
    return exe


def _instances(lines, prefix):
    return {l[len(prefix):] for l in lines if l.startswith(prefix)}


@pytest.fixture(scope="module")
def enumeration(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("sweep_instances")
    product = _build(tmp, "product", ENUM_PROGRAM, ["-O2"])
    tuning = _build(tmp, "tuning", ENUM_PROGRAM, ["-O2", "-DDTO_TUNING"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("DTO_")}
    start = lambda exe, cus, pins: subprocess.Popen([exe] + cus, stdout=subprocess.PIPE, text=True, env=dict(env, **pins))
    walks = [start(product, ["256"], {}), start(product, ["48"], {})] + [start(tuning, ["256"], pins) for pins in PINS]   # side by side
    lines = [w.communicate()[0].splitlines() for w in walks]
    assert all(w.returncode == 0 for w in walks)
    return lines[0] + lines[1], list(zip(PINS, lines[2:]))


def test_the_instantiation_lists_are_what_the_planner_names(enumeration):
    """Product build: every (form, instantiation) choose_sweep returns over the shapes above is in the header's list of its family,
    and every listed kernel is returned for some shape.  On 256 CUs alone the lists hold one kernel more than the planner names,
    k_sweep_cluster<2, 1, 2> (see the note above ENUM_PROGRAM); everything else is named there."""
    lines, _ = enumeration
    listed = _instances(lines, "list ")
    at_256, at_48 = _instances(lines, "inst 256 "), _instances(lines, "inst 48 ")
    print(sorted(at_256), sorted(at_48), sorted(listed), sep="\n")
    assert "gs" in at_256
    assert listed - (at_256 - {"gs"}) == {"cluster 2 1 2"}
    assert (at_256 | at_48) - {"gs"} == listed


def test_pinned_shapes_stay_inside_the_lists(enumeration):
    """TUNING build under each set of pins tests/test_gpu_sweep_forms.py runs its children with: nothing outside the lists."""
    _, pinned = enumeration
    for pins, lines in pinned:
        named = _instances(lines, "inst 256 ")
        print(pins, sorted(named))
        assert named - {"gs"} <= _instances(lines, "list "), pins
    # (the pins do reach what they are for: both tile counts of both cluster sizes at 256 states)
    reached = set().union(*[_instances(lines, "inst 256 ") for _, lines in pinned])
    assert {"cluster 2 1 2", "cluster 2 2 2", "cluster 1 1 4", "cluster 1 2 4", "cluster 1 1 2", "cluster 1 2 2"} <= reached


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("sweep_plan")
    src, exe = str(tmp / "plan.cpp"), str(tmp / "plan")
    calls = "".join("    shape(%d, %d, %d, %d, %d, %d);\n" % key for key, _f, _c, _g in SHAPES)
    with open(src, "w") as f:
        f.write(PROGRAM.replace("@SHAPES@", calls))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def _lines(output, prefix):
    return [l[len(prefix):] for l in output if l.startswith(prefix)]


def test_device_plan_and_host_path_equal_both_parent_texts_on_the_whole_grid(output):
    """beta = 0 .. 60 in steps of 1/1024 (61441), every integer 1 .. 60 with its two neighbouring doubles (180), NaN, +Inf, 1e6 and the
    next double above it, 1e-300, 1e5 (6): four answers per point -- the parent's host chain, the parent's k_plan_dev body,
    device_plan, the host path through the header -- and no point at which any two differ."""
    differ = _lines(output, "differ ")
    print("\n".join(differ[:20]))
    assert _lines(output, "budget points ") == ["%d differ 0" % (61441 + 180 + 6)] and differ == []


@pytest.mark.parametrize("beta,plan", [("11.07", (1, 66, 16)),    # the benchmark point (DESIGN section 8 quotes its 66 terms)
                                       ("11.125", (1, 66, 16)),   # the last of the grid that is one round ...
                                       ("11.25", (2, 48, 23)),    # ... and two rounds
                                       ("0", (1, 14, 6)), ("9", (1, 59, 28)), ("100000", (11112, 59, 28))],   # (grid points: the parent's)
                         ids=["benchmark", "one-round", "two-rounds", "zero", "theta", "1e5"])
def test_pinned_plans(output, beta, plan):
    got = {l.split()[0]: tuple(int(v) for v in l.split()[1:]) for l in _lines(output, "plan ")}
    key = [k for k in got if float(k) == float(beta)]
    print(beta, got[key[0]])
    assert got[key[0]] == plan


def test_tc_rule_hump_plan_and_growth_rate(output):
    # d_ub / 2 - 1; the plan's own value first; an override replaces both; below 2: from the first step on
    assert _lines(output, "tc ") == ["32 16 5 0"]
    # logH = {12.5, 9.5, 8.75, 3.0}, kend = {50, 41, 33, 198}: theta_v 9 -> three rounds of 33 + 6; not valid or no q qualifies ->
    # plan_sweep(20) (three rounds at theta_v 9, ten at 2); theta_v 3.5 -> four rounds, 198 + 6 capped at 200
    hump = _lines(output, "hump ")[0].split()
    assert hump[:3] == ["3", "39", "-1"] and hump[3:6] == hump[13:15] + ["-1"] and hump[6:9] == hump[15:17] + ["-1"], hump
    assert hump[9:12] == ["4", "200", "-1"] and hump[12] == "sweep" and hump[13] == "3" and hump[15] == "10", hump
    # `d2 == d2 ? std::min(beta, d2) : d2` as the driver wrote it twice: the smaller bound; a NaN norm stays NaN; so does a NaN beta
    # (std::min returns its first argument unless the second is smaller)
    assert _lines(output, "growth ") == ["7.25 7.25 1 1"]


def _numbers(text):
    return tuple(float(v) if "." in v or "e" in v else int(v) for v in text.split())


@pytest.mark.parametrize("key,fused,cluster,gs", SHAPES, ids=["-".join(str(v) for v in s[0]) for s in SHAPES])
def test_planner_outputs(output, key, fused, cluster, gs):
    tag = "%d %d %d %d %d %d :" % key
    for letter, want in (("F", fused), ("C", cluster), ("G", gs)):
        got = _lines(output, letter + " " + tag)
        print(letter, tag, got)
        if want is None:
            assert got == []
        else:
            assert len(got) == 1 and _numbers(got[0]) == _numbers(want)


def test_the_two_documented_shapes(output):
    """DESIGN.md section 4, 256 states x 4 drives x 1999 intervals on 256 CUs.  Alone: MT 4, NT 3, 9 intervals per workgroup, 223
    workgroups, the K loop split over two waves per SIMD.  Beside the chain: two column groups of two tiles, 12 intervals, 167."""
    alone = _numbers(_lines(output, "F 256 4 1 1999 256 0 :")[0])
    shared = _numbers(_lines(output, "F 256 4 1 1999 256 1 :")[0])
    #        ok MT NT ipw nslot nblocks WC WK S64 NX
    assert alone[:10] == (1, 4, 3, 9, 1, 223, 1, 2, 0, 0)
    assert shared[:10] == (1, 4, 2, 12, 1, 167, 2, 1, 0, 0)


def test_every_form_row_is_shown(output):
    assert sorted(l.split()[0] for l in _lines(output, "form ")) == sorted(label for label, _ in FORMS)


@pytest.mark.parametrize("label,want", FORMS, ids=[f[0] for f in FORMS])
def test_form_choice(output, label, want):
    got = {l.split()[0]: l.split()[1:] for l in _lines(output, "form ")}[label]
    print(label, got)
    assert got[0] == want
    # the choice carries what was asked (SweepArgs::as_chosen takes store and shared_chip from it)
    assert got[1] == ("1" if label.startswith("store") else "0")
    assert got[2] == ("1" if label.endswith("_shared") else "0")


def test_header_includes_only_the_standard_library():
    with open(os.path.join(CSRC, "dto_sweep_plan.h")) as f:
        includes = sorted(l.split()[1] for l in f if l.lstrip().startswith("#include"))
    assert includes == ["<cmath>", "<cstddef>", "<cstdint>", "<cstdlib>"], includes
