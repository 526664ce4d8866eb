// dto_sweep_plan.h -- everything that decides how a generator sweep runs: how many Taylor steps it may take, which of the five forms
// it takes, what launch shape that form gets and which kernel instantiations exist for it.  All of it is host arithmetic on a few
// integers and one norm bound.  Plain C++ (no HIP header, no engine header): the same functions serve the host driver
// (dto_engine.cpp), the launchers and kernels (dto_sweep_fused.hip, dto_sweep_gs.hip: the LDS carve-ups, and k_plan_dev, which runs
// device_plan on one lane) and a g++-built test (tests/test_sweep_plan_header.py).  Four groups: 1. step budget (host and device),
// 2. launch shapes, 3. form choice, 4. kernel instantiations.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#ifdef __HIPCC__
#define SWP_HD __host__ __device__
#else
#define SWP_HD
#endif

namespace dto {

// Tuning switches for A/B measurements exist only in builds with -DDTO_TUNING (`make TUNING=1`); the product
// library reads no environment variable.
inline int tune_int(const char* name, int dflt) {
#ifdef DTO_TUNING
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}
inline double tune_double(const char* name, double dflt) {
#ifdef DTO_TUNING
    const char* e = getenv(name);
    return e ? atof(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

// ------------------------------------------------------------------------------------------ 1. step budget (host and device)

struct SweepPlan {
    int q, d_ub;
    int tc = -1;   // first step at which the termination test runs (-1: d_ub / 2 - 1)
};

constexpr double TAYLOR_TERM_FLOOR = 1e-19;   // a round's budget counts the Taylor terms of exp(br) down to this ...
constexpr int TAYLOR_MIN_TERMS = 8;           // ... at least eight of them ...
constexpr int TAYLOR_MAX_TERMS = 200;         // ... at most 200 (also the cap of a budget taken from k_hump's term count) ...
constexpr int TAYLOR_EXTRA_TERMS = 6;         // ... and six more
constexpr double BETA_FINITE_MAX = 1e6;       // a bound past this (or NaN) is a non-finite iterate ...
constexpr int NONFINITE_BUDGET = 30;          // ... which gets bounded work: one round of 30 steps, NaN/Inf propagates to the output
constexpr double CHEAP_BETA_MAX = 40.0;       // the hump criterion is applied to the cheap bound itself only below this
// the hump limit of the cheap bound: the literal e^9, where plan_sweep and plan_hump read theta_v (DTO_THETA_V): they differ in
// TUNING builds that set it
constexpr double CHEAP_HUMP_LIMIT = 9.0;

// worst-case cancellation budget e^9 ~ 1e4 on the Taylor sums (tolerance 1e-10): what the host passes as `theta_v` below
inline double sweep_theta_v() {
    static const double theta_v = tune_double("DTO_THETA_V", 9.0);
    return theta_v;
}

// Step budget of one round of radius br: the Taylor terms of exp(br) down to 1e-19 (8 to 200 of them), and six more
SWP_HD inline int taylor_budget(double br) {
    int t = TAYLOR_MIN_TERMS;
    double term = 1.0;
    for (int i = 1; i <= t; ++i) term *= br / i;
    while (term > TAYLOR_TERM_FLOOR && t < TAYLOR_MAX_TERMS) { ++t; term *= br / t; }
    return t + TAYLOR_EXTRA_TERMS;
}

// The growth-rate rule: rounds of radius at most theta_v, each with the budget of its radius
SWP_HD inline SweepPlan plan_sweep(double beta, double theta_v) {
    SweepPlan p{1, 12};
    if (!(beta == beta) || beta > BETA_FINITE_MAX) {  // non-finite iterate: bounded work, NaN/Inf propagates to the output
        p.q = 1; p.d_ub = NONFINITE_BUDGET;
        return p;
    }
    const int q = (int)std::ceil(beta / theta_v);
    p.q = q < 1 ? 1 : q;
    p.d_ub = taylor_budget(beta / p.q);
    return p;
}

// log of the hump of the bound, max_k beta^k / k!: the maximum sits at k = floor(beta) or next to it
SWP_HD inline double hump_peak_log(double beta) {
    double lh = 0.0;
    const int k0 = (int)std::floor(beta);
    for (int k = (k0 > 1 ? k0 - 1 : 1); k <= k0 + 1; ++k) lh = std::fmax(lh, k * std::log(beta) - std::lgamma(k + 1.0));
    return lh;
}

// `loose`: the caller keeps no Taylor terms (eval_constraint without reuse_forward_sweep), so a generous step budget costs nothing --
// the one-launch sweeps end by their own termination test.  Then the hump criterion is applied to the cheap bound itself
// (max_k beta^k / k! <= e^9, the same four digits plan_hump allows): at the benchmark shape the triangle-inequality bound on
// ||A^2||^(1/2) is 9.5, just past the beta <= 9 rule, and the exact norm (a store-less basis GEMM, a kernel for the hump and two
// host round trips: 0.2 of the callback's 1.1 ms) was bought only to learn what this already shows.
// The step budget the cheap generator-norm bound alone gives, where that is a single round (q = 1): no exact norm needed.  Where it
// is not (false), `out` holds plan_sweep's plan.
SWP_HD inline bool cheap_plan(double beta, bool loose, double theta_v, SweepPlan& out) {
    out = plan_sweep(beta, theta_v);
    if (out.q == 1) return true;  // the cheap bound already gives one round
    if (loose && beta == beta && beta < CHEAP_BETA_MAX && hump_peak_log(beta) <= CHEAP_HUMP_LIMIT) {
        SweepPlan p{1, taylor_budget(beta)};
        // the terms of the series grow up to index ~beta and fall from there: the test (two successive terms below 1.1e-16 of the
        // sum, Al-Mohy & Higham's own criterion, which they apply from the first term on) starts a few terms past the peak
        // of the BOUND -- a function of Z alone, like d_ub / 2 - 1, but not inflated by the bound's slack in the tail
        const int half = p.d_ub / 2 - 1, past_peak = (int)std::ceil(beta) + 4;
        p.tc = half < (past_peak > 2 ? past_peak : 2) ? half : (past_peak > 2 ? past_peak : 2);
        out = p;
        return true;
    }
    return false;
}

// The termination test cannot fire early in the series: it is first run at step tc = d_ub/2 - 1 (d_ub comes from an
// upper bound on the terms needed at this very Z, so tc is a function of Z alone and results stay reproducible; a
// column block that would pass earlier merely adds a few terms below 1e-16 of its sum).  The plan's own tc goes first; a value
// below 2 means "from the first step on".  `forced` >= 0 replaces both.
SWP_HD inline int sweep_tc(const SweepPlan& plan, int forced = -1) {
    const int tc = forced >= 0 ? forced : (plan.tc >= 0 ? plan.tc : plan.d_ub / 2 - 1);
    return tc < 2 ? 0 : tc;
}

// Plan from the a-priori hump bound of k_hump (logH[q - 1], kend[q - 1]: log of the hump and the term count with q rounds; `valid`:
// all four are numbers): the fewest rounds whose Taylor sums cannot lose more than theta_v e-folds to cancellation; falls back to
// the growth-rate rule when no q <= 4 qualifies or the bound is not finite.
inline SweepPlan plan_hump(bool valid, const double logH[4], const int kend[4], double theta_v, double beta_fallback) {
    if (valid)
        for (int q = 1; q <= 4; ++q)
            if (logH[q - 1] <= theta_v) {
                const int d = kend[q - 1] + TAYLOR_EXTRA_TERMS;
                return SweepPlan{q, d < TAYLOR_MAX_TERMS ? d : TAYLOR_MAX_TERMS};
            }
    return plan_sweep(beta_fallback, theta_v);
}

// ||A^t|| <= ||A^2||^floor(t/2) ||A||^(t mod 2): an exact d2 = max_k ||A_k^2||^(1/2) is the sharper (and still rigorous) growth rate
// for the sweep's step budget; a NaN stays one
inline double growth_rate(double beta, double d2) { return d2 == d2 ? (d2 < beta ? d2 : beta) : d2; }

// The step budget of a sweep from the cheap norm bound alone, resolved to {q, d_ub, tc}: cheap_plan(loose) where it gives a single
// round, else plan_sweep -- what a host that waited for the bound would have used.  k_plan_dev runs this on one lane.
SWP_HD inline SweepPlan device_plan(double beta, double theta_v) {
    SweepPlan p;
    (void)cheap_plan(beta, /*loose=*/true, theta_v, p);
    p.tc = sweep_tc(p);
    return p;
}

// ------------------------------------------------------------------------------------------ 2. launch shapes

constexpr int MAX_TYPES = 36;                // column types of a generator sweep (p, d^i, h^{ij})

struct TypeDesc {     // one column type of a generator sweep
    int32_t n_extra;  // extra segments G_gen * Z_src * scaleE * mult
    int32_t gen[2];
    int32_t src[2];
    double mult[2];
};

struct SweepTypes {
    int32_t T;
    TypeDesc t[MAX_TYPES];
};

inline SweepTypes make_types(int m, bool second_order) {
    SweepTypes ty{};
    int T = 0;
    ty.t[T++] = TypeDesc{0, {0, 0}, {0, 0}, {0, 0}};  // p
    for (int j = 0; j < m; ++j) {                    // d^j: + E_j p
        TypeDesc d{};
        d.n_extra = 1; d.gen[0] = 1 + j; d.src[0] = 0; d.mult[0] = 1.0;
        ty.t[T++] = d;
    }
    if (second_order) {
        for (int i = 0; i < m; ++i)
            for (int j = i; j < m; ++j) {  // h^{ij}: + E_i d^j + E_j d^i
                TypeDesc d{};
                if (i == j) {
                    d.n_extra = 1; d.gen[0] = 1 + i; d.src[0] = 1 + i; d.mult[0] = 2.0;
                } else {
                    d.n_extra = 2;
                    d.gen[0] = 1 + i; d.src[0] = 1 + j; d.mult[0] = 1.0;
                    d.gen[1] = 1 + j; d.src[1] = 1 + i; d.mult[1] = 1.0;
                }
                ty.t[T++] = d;
            }
    }
    ty.T = T;
    return ty;
}

// LDS of a CU as the one-launch forms use it
constexpr size_t SWEEP_LDS_OPT_IN = 160 * 1024;   // dynamic LDS every sweep kernel opts into (*_prepare): the whole CU
constexpr size_t SWEEP_LDS_LIMIT = 156 * 1024;    // what a FusedLds carve-up may take of it
constexpr size_t SWEEP_LDS_ONE_PER_CU = 82 * 1024;
// more than half a CU's LDS: one workgroup per CU (the hand-off's condition)
inline size_t lds_one_per_cu(size_t bytes) { return bytes < SWEEP_LDS_ONE_PER_CU ? SWEEP_LDS_ONE_PER_CU : bytes; }

// a narrow column tile streams the generators from L2 at 512 / (16 NT) bytes per cycle and CU, which at NT = 1 is more than a CU
// sustains: the cost of a tile count NT is NT * L2_FACTOR[NT]
constexpr double L2_FACTOR[4] = {0.0, 1.6, 1.15, 1.0};

// Clusters of R workgroups: as many as the chip holds with ONE workgroup per CU (a multiple of 8, one per XCD and slot), capped by
// the interval groups they walk; fewer than 8: the cluster forms do not apply
inline long cluster_grid(int n_cu, int R, long n_groups) {
    long n_clusters = ((long)(n_cu / R) / 8) * 8;
    if (n_clusters > ((n_groups + 7) / 8) * 8) n_clusters = ((n_groups + 7) / 8) * 8;
    return n_clusters;
}

// LDS carve-up of k_sweep_fused and k_sweep_cluster, shared by host and device
struct FusedLds {
    int zs, scr, cg, se, tn, sn, xn, xg, xs, xm, flag, total;  // offsets in doubles
    SWP_HD FusedLds(int npad, int T, int m, int ipw, int nslot, int MT) {
        const int NC = T * ipw, ZS = npad + 2;
        (void)nslot; (void)MT;
        int o = 0;
        zs = o; o += NC * ZS + 40; // the B-fragment prefetch runs up to two groups of four k-steps past the last column (K split)
        scr = o;
        cg = o; o += (m + 1) * ipw;
        se = o; o += ipw;
        tn = o; o += 3 * NC;
        sn = o; o += NC;
        xm = o; o += 2 * T;
        xn = o; o += (T + 1) / 2;          // ints, two per double
        xg = o; o += T;                    // 2 ints per type
        xs = o; o += T;
        flag = o; o += 2;
        total = o;
    }
};

// LDS carve-up of k_sweep_s64
struct S64Lds {
    static constexpr int ZS = 66;   // column pitch: the B-fragment reads of a half-wave fall on 32 distinct 8-byte banks
    int zs, pb, cg, se, tn, sn, xm, xn, xg, xs, total;  // offsets in doubles
    SWP_HD S64Lds(int T, int m, int ipw) {
        int o = 0;
        zs = o; o += 16 * ZS;
        pb = o; o += 2 * 4 * 4 * 2 * 64 * 2;   // [term parity][row tile][source wavefront][half][lane] 16 bytes
        cg = o; o += (m + 1) * ipw;
        se = o; o += ipw;
        tn = o; o += 4 * 16;
        sn = o; o += 4 * 16;
        xm = o; o += 2 * T;
        xn = o; o += (T + 1) / 2;   // ints, two per double
        xg = o; o += T;
        xs = o; o += T;
        total = o;
    }
};

// LDS carve-up of k_sweep_gs, shared by host and device (doubles)
struct GsLds {
    int slot, nmax, tyt, colt, gct, flag, cgt, total;   // total: without the coefficient table [(MP + 1)][cap] that follows at cgt
    SWP_HD constexpr GsLds(int KU, int MP, int NT) : slot(0), nmax(0), tyt(0), colt(0), gct(0), flag(0), cgt(0), total(0) {
        const int NPAD = 32 * KU, ZS = NPAD + 2, NCP = 16 * NT;
        (void)MP;
        slot = NCP * ZS + 8;            // one column slot (also the scratch of the partial tiles [4][NCP][32]); two of them
        int o = 2 * slot;
        nmax = o; o += 2 * 3 * NCP;     // [2][3][NCP] cluster-wide column norms: term t-1, term t, sum (bit patterns)
        tyt = o; o += 5 * MAX_TYPES;    // per column type: multipliers [2] (doubles), then n_extra, generators [2], sources [2] (ints)
        colt = o; o += NCP;             // per column: {offset of the column inside a term slab for interval group 0, interval within the group} (ints)
        gct = o; o += MP * NCP + (MP * NCP + 1) / 2;   // per (generator, column): multiplier of the inhomogeneous term (0: none), its source column (ints)
        flag = o; o += 2;               // ints: [0] a rendezvous timed out
        cgt = o;                        // [(MP + 1)][cap]: dt ubar_g of every interval of the cluster (row MP: dt), built once
        total = o;
    }
};
inline size_t gs_lds_bytes(int KU, int MP, int NT, int cap) {
    return lds_one_per_cu(((size_t)GsLds(KU, MP, NT).total + (size_t)(MP + 1) * cap) * sizeof(double));
}

// ---- the whole sweep in one persistent launch (dto_sweep_fused.hip): a workgroup owns `ipw` intervals, all rows, all types
struct FusedSweepPlan {
    int MT, NT, ipw, nslot, nblocks;
    int WC = 1;  // column groups of wavefronts (4 WC wavefronts per workgroup), NT column tiles per group
    int WK = 1;  // 2: two wavefronts per SIMD split the K loop of a wave tile (256 states)
    int S64 = 0; // 1: the generator-stationary 64-state form (k_sweep_s64), NX = most inhomogeneous sources of a column type
    int NX = 0;
    size_t lds_bytes;
};

// Shape of the launch for a sweep over T column types of an integrator padded to npad states, n_int intervals:
// intervals per workgroup (ipw) and tile counts.  Returns false when the fused form does not apply.
inline bool sweep_fused_plan(int npad, int m, const SweepTypes& ty, int64_t n_int, int n_cu, FusedSweepPlan& out, bool shared_chip = false) {
    const int T = ty.T;
    if (T < 1 || n_int <= 0) return false;
    // One row pass must cover the matrix (npad = 64, 128 or 256: 4 wavefronts x 16 MT rows).  Larger matrices offer their
    // parallelism in the ROW dimension, which a workgroup-per-interval-group form cannot use without exchanging the term
    // columns between workgroups every step: there the step-per-launch sweep is faster (measured: 512 states 19.0 against
    // 22.6 ms, 1024 states 109 against 128 ms per Jacobian), as it is when the intervals are too few to give half the CUs a
    // workgroup (256 states x 200 knots: 2.25 against 2.50 ms).
    if (npad != 64 && npad != 128 && npad != 256) return false;
    const int MT = npad / 64;
    int nslot = 0;
    for (int g = 0; g <= m; ++g) {
        int mask = 0;
        for (int t = 0; t < T; ++t)
            for (int x = 0; x < ty.t[t].n_extra; ++x)
                if (ty.t[t].gen[x] == g) mask |= 1 << ty.t[t].src[x];
        nslot = nslot > __builtin_popcount(mask) ? nslot : __builtin_popcount(mask);
    }
    // cost model, 256 states: one workgroup per CU and round; a round takes NT units of MFMA time, and a narrow column tile
    // streams the generators from L2 at 512 / (16 NT) bytes per cycle and CU, which at NT = 1 is more than a CU sustains.
    // 64 and 128 states: the steps are latency-bound (two barriers and an epilogue per handful of MFMAs), several workgroups
    // share a CU, and one column tile per workgroup is fastest -- measured per sweep at 1000 knots, NT = 1 / 2 / 3:
    // 0.24 / 0.30 / 0.44 ms (64 states), 0.61 / 0.73 / 0.86 ms (128 states); three workgroups per CU count as one round.
    // 64 states, at most 16 columns per interval: the generator-stationary form, as many intervals as a 16-column tile holds
    // (measured per 1000-knot Jacobian sweep: see DESIGN.md section 4)
    static const int s64_env = tune_int("DTO_SWEEP_S64", 1);
    if (npad == 64 && s64_env && m + 1 <= 5 && T <= 16) {
        int nx = 0;
        for (int t = 0; t < T; ++t) nx = nx > ty.t[t].n_extra ? nx : ty.t[t].n_extra;
        // a workgroup's Taylor step costs the same for 1 or 16 live columns, so few intervals are spread over the CUs first
        // (one round of workgroups) and only then packed into the tile
        // (beside another kernel -- the Hessian's forward column next to its adjoint sweep -- the CU time is what counts: full tiles)
        int ipw = shared_chip ? 16 / T : (int)((n_int + n_cu - 1) / n_cu);
        ipw = ipw < 1 ? 1 : (ipw > 16 / T ? 16 / T : ipw);
        const long nblocks = (long)((n_int + ipw - 1) / ipw);
        if (nx <= 2) {
            out.MT = 1; out.NT = 1; out.WC = 1; out.WK = 1; out.ipw = ipw; out.nslot = nslot; out.nblocks = (int)nblocks;
            out.S64 = 1; out.NX = nx;
            out.lds_bytes = (size_t)S64Lds(T, m, ipw).total * sizeof(double);
            return true;
        }
    }
    out.S64 = 0;
    static const double t_small[2][4] = {{0.0, 0.24, 0.30, 0.44}, {0.0, 0.61, 0.73, 0.86}};
    auto search = [&](int WC) {
        bool found = false;
        double best = 0.0;
        for (int ipw = 1; ipw <= 48; ++ipw) {
            const int NC = T * ipw;
            int NT = (NC + 15) / 16;
            if (WC == 2) {
                if (NT > 4) break;
                if (NT != 4) continue;  // two column groups of two tiles each
                NT = 2;
            } else if (NT > 3) break;
            const FusedLds L(npad, T, m, ipw, nslot, MT);
            const size_t bytes = (size_t)L.total * sizeof(double);
            if (bytes > SWEEP_LDS_LIMIT) break;
            const long nblocks = (long)((n_int + ipw - 1) / ipw);
            const long slots = MT <= 2 ? 3L * n_cu : n_cu;
            const long rounds = (nblocks + slots - 1) / slots;
            // ties go to the fewer workgroups (less MFMA work issued in total)
            const double cost = (MT <= 2 ? (double)rounds * t_small[MT - 1][NT] : (double)rounds * NT * L2_FACTOR[NT]) + 1e-6 * (double)nblocks * NT;
            if (!found || cost < best) {
                found = true; best = cost;
                out.MT = MT; out.NT = NT; out.WC = WC; out.ipw = ipw; out.nslot = nslot; out.lds_bytes = bytes; out.nblocks = (int)nblocks;
            }
        }
        return found && 2 * out.nblocks >= n_cu;
    };
    // Eight wavefronts in two column groups (256 states, 49..64 columns: 12 intervals of a Jacobian sweep per workgroup): two
    // wavefronts per SIMD hide each other's operand traffic, +10 % MFMA rate per CU -- but a third fewer workgroups, each a
    // fifth longer (256 x 2000: 167 workgroups, 4.0 ms against 223, 3.3 ms).  It pays when the CUs the sweep leaves free are
    // used by another stream (`shared_chip`: the Jacobian's sweep next to the propagator chain), not when the sweep runs alone.
    out.WK = 1;
    if (shared_chip && npad == 256 && search(2)) return true;
    if (!search(1)) return false;
    if (npad == 256) out.WK = 2;   // (WC == 1) two waves per SIMD splitting the K loop
    return true;
}

// ---- the same sweep with the rows of the matrix split over a cluster of R workgroups that exchange their slices of every new
// term through global memory (dto_sweep_fused.hip): short shards of 128- and 256-state problems
struct ClusterSweepPlan {
    int MT, NT, R, ipw, n_groups, n_clusters, nblocks;
    size_t lds_bytes;
    double step_us;  // the cost model's time per Taylor step and round of clusters
};

// Shape of the cluster launch: R members per interval group, NT column tiles (ipw = 16 NT / T intervals per group), as many
// clusters as the chip holds with ONE workgroup per CU (cluster_grid); each cluster walks the groups
// cluster, cluster + n_clusters, ...  Cost model per Taylor step, in MFMA units of one 16-column tile over 64 MT rows: the
// tile count times the same L2 factor as the single-workgroup form (a narrow tile streams the generators faster than a CU
// takes them in) plus the exchange (rendezvous + slice traffic), which does not shrink with the tile.
inline bool sweep_cluster_plan(int npad, int m, const SweepTypes& ty, int64_t n_int, int n_cu, ClusterSweepPlan& out) {
    const int T = ty.T;
    if (T < 1 || n_int <= 0 || n_cu < 16) return false;
    if (npad != 128 && npad != 256) return false;   // (512 and 1024 states measured slower than the step launches: choose_sweep)
    static const int force_r = tune_int("DTO_CLUSTER_R", 0), force_nt = tune_int("DTO_CLUSTER_NT", 0);
    bool found = false;
    double best = 0.0;
    for (int R = 2; R <= 4; R += 2) {
        if (npad % (64 * R) != 0) continue;
        const int MT = npad / (64 * R);
        if (force_r && R != force_r) continue;
        for (int NT = 1; NT <= 2; ++NT) {   // (three-tile shapes spill beside the exchange registers)
            if (force_nt && NT != force_nt) continue;
            const int ipw = (16 * NT) / T;
            if (ipw < 1) continue;
            if (NT > 1 && (16 * (NT - 1)) / T == ipw) continue;  // the narrower shape holds as many intervals
            const FusedLds L(npad, T, m, ipw, 0, MT);
            const size_t bytes = (size_t)L.total * sizeof(double);
            if (bytes > SWEEP_LDS_LIMIT) continue;
            const long n_groups = (long)((n_int + ipw - 1) / ipw);
            const long n_clusters = cluster_grid(n_cu, R, n_groups);
            if (n_clusters < 8) continue;
            const long rounds = (n_groups + n_clusters - 1) / n_clusters;
            const double step_us = MT * NT * L2_FACTOR[NT] * (m + 1) * npad * 7.3e-3;   // 64 cycles per MFMA at 2.2 GHz
            const double exch_us = 3.0 + 16.0 * NT * npad * 8.0 * 1e-3 / 60.0;           // rendezvous + slices at ~60 GB/s per CU
            const double cost = rounds * (step_us + exch_us);
            if (!found || cost < best) {
                found = true; best = cost;
                out.MT = MT; out.NT = NT; out.R = R; out.ipw = ipw; out.n_groups = (int)n_groups; out.n_clusters = (int)n_clusters;
                out.nblocks = (int)(n_clusters * R); out.lds_bytes = lds_one_per_cu(bytes); out.step_us = step_us + exch_us;
            }
        }
    }
    return found;
}

inline size_t sweep_cluster_workspace_doubles(int npad, const ClusterSweepPlan& pl) {
    const size_t NCP = 16 * (size_t)pl.NT;
    return (size_t)pl.n_clusters * 2 * (NCP * npad + 8 * NCP);
}

// ---- the sweep with the generators STATIONARY in registers (dto_sweep_gs.hip, round 4): a cluster of npad / 32 workgroups shares an
// interval group, each member holding 32 rows of every generator for the whole launch; only the term slices move (through the
// sweep's own term slabs, sc1 on both sides).  128 and 256 states, at most 4 drives, no sub-stepping (q = 1).
struct GsSweepPlan {
    int KU, MP, NT, ipw, has_src, n_groups, n_clusters, nblocks, cap;
    size_t lds_bytes;
    double term_us;  // the cost model's time per Taylor term
};

// Shape of the launch: KU = npad / 32 members per cluster, as many clusters as the chip holds with one workgroup per CU
// (cluster_grid), NT column tiles per group (ipw = 16 NT / T intervals), each cluster walking the groups cluster,
// cluster + n_clusters, ... round-robin.  Cost per Taylor term: rounds x (product + collect / reduce / publish), in us.
inline bool sweep_gs_plan(int npad, int m, const SweepTypes& ty, int64_t n_int, int n_cu, GsSweepPlan& out) {
    const int T = ty.T;
    if (T < 1 || n_int <= 0) return false;
    if (npad != 256 && npad != 128) return false;   // clusters of 8 / 4 members of 32 rows each
    if (m + 1 > 5) return false;
    const int KU = npad / 32, R = KU;
    bool has_src = false;
    for (int t = 0; t < T; ++t) {
        if (ty.t[t].n_extra > 2) return false;
        if (ty.t[t].n_extra > 0) has_src = true;
    }
    static const int force_nt = tune_int("DTO_GS_NT", 0);
    bool found = false;
    double best = 0.0;
    for (int NT = 1; NT <= 2; ++NT) {
        if (force_nt && NT != force_nt) continue;
        const int ipw = (16 * NT) / T;
        if (ipw < 1) continue;
        const long n_groups = (long)((n_int + ipw - 1) / ipw);
        const long n_clusters = cluster_grid(n_cu, R, n_groups);
        if (n_clusters < 8) continue;
        const long rounds = (n_groups + n_clusters - 1) / n_clusters;
        if (rounds > 64) continue;
        const int MPs = m + 1 <= 3 ? 3 : 5;
        const int cap = (int)(rounds * ipw);
        if (gs_lds_bytes(KU, MPs, NT, cap) > SWEEP_LDS_OPT_IN) continue;
        const double prod_us = 2.0 * NT * (m + 1) * 2 * KU * 64.0 / 2200.0;   // MFMAs per wave x 64 cycles at 2.2 GHz
        const double fix_us = rounds > 1 ? 3.5 : 9.0;   // reduce + publish; a lone group per cluster also exposes its rendezvous and collect
        // (the two-tile instance with source terms at 4 drives is the one the register file cannot quite hold: 35 spilled registers,
        // measured 7 % slower per column than the one-tile instance)
        const double cost = rounds * (prod_us + fix_us) * (has_src && NT == 2 && MPs == 5 ? 1.08 : 1.0);
        if (!found || cost < best) {
            found = true; best = cost;
            out.KU = KU; out.MP = MPs; out.NT = NT; out.ipw = ipw; out.has_src = has_src ? 1 : 0;
            out.n_groups = (int)n_groups; out.n_clusters = (int)n_clusters; out.nblocks = (int)(n_clusters * R);
            out.cap = cap; out.lds_bytes = gs_lds_bytes(KU, MPs, NT, cap); out.term_us = cost;
        }
    }
    return found;
}

inline size_t sweep_gs_norm_doubles(const GsSweepPlan& pl) { return (size_t)pl.n_groups * 3 * pl.KU * 2 * 16 * pl.NT; }   // exchange slab of the partial column norms

// ------------------------------------------------------------------------------------------ 3. form choice

// the form a generator sweep took (dto_profile_get "sweep_gs" .. "sweep_step"): one count per run_sweep call, not per launch
enum { SWEEP_GS = 0, SWEEP_FUSED = 1, SWEEP_S64 = 2, SWEEP_CLUSTER = 3, SWEEP_STEP = 4 };

// The form a generator sweep takes and that form's launch plan.  choose_sweep is the one place that decides it: run_sweep executes
// a choice, and a caller whose streams or bookkeeping depend on the form asks first and hands the same choice on.
struct SweepChoice {
    int form = SWEEP_STEP;
    GsSweepPlan gs;            // form == SWEEP_GS
    FusedSweepPlan fused;      // form == SWEEP_FUSED, SWEEP_S64
    ClusterSweepPlan cluster;  // form == SWEEP_CLUSTER
    bool store = false, shared_chip = false;  // as asked (SweepArgs::as_chosen takes them from here)
    bool one_workgroup() const { return form == SWEEP_FUSED || form == SWEEP_S64; }  // the single-workgroup forms (these read plan_dev)
    SweepChoice& is(int f) { form = f; return *this; }
};

// What the rule reads.  store: every Taylor term is kept in the term store; shared_chip: another stream's kernels run beside the
// sweep (the propagator chain, the Hessian's adjoint sweep); step_only: the caller has initialised the sweep itself (the products'
// extra start vector).
struct SweepSituation {
    int npad, Kpad, m;         // padded states, padded intervals of the sweep's buffers, drives
    SweepTypes types;
    int64_t n_int;             // owned intervals
    int n_cu;
    int sweep_form;            // option "sweep_form": 1 = one launch per Taylor step
    bool reuse;                // option "reuse_forward_sweep"
    bool frozen;               // the sweep reads stored p terms and computes the tangent columns alone
    bool has_term_store;       // a term store exists ...
    int dcap;                  // ... and holds this many Taylor terms
    int q, d_ub;               // the plan's rounds and step budget
    bool store, shared_chip, step_only;
};

// In order: generator-stationary, fused (64 states: its generator-stationary instance), row-split cluster, one launch per Taylor step.
inline SweepChoice choose_sweep(const SweepSituation& s) {
    SweepChoice c{};
    c.store = s.store;
    c.shared_chip = s.shared_chip;
    const SweepTypes& ty = s.types;
    // no one-launch form: by option, with frozen p terms, where the term store cannot hold the step budget, and for a stored
    // single column under reuse_forward_sweep (a frozen sweep reads nterms_p in blocks of TN intervals)
    if (s.step_only || s.sweep_form == 1 || s.frozen) return c;
    if (s.store && (!(s.has_term_store && s.d_ub + 1 <= s.dcap) || (ty.T == 1 && s.reuse))) return c;
    // the fused planner's answer for a sweep that has the chip to itself: asked by the generator-stationary and the fused form
    const bool fused_alone = sweep_fused_plan(s.npad, s.m, ty, s.n_int, s.n_cu, c.fused);
    // Generator-stationary form (dto_sweep_gs.hip): clusters of npad / 32 workgroups with the generators resident in their registers.
    // It needs the whole chip to itself (one 512-register workgroup per CU, all cluster members resident): not beside the chain
    // (`shared_chip`), not with sub-stepping.  It is taken where the single-workgroup form cannot fill the chip: single-column sweeps
    // (eval_constraint, the Hessian's forward column) and sweeps the fused planner refuses (short shards); measured
    // (tools/sweep_gs_probe, 256 states): p column of 2000 knots 0.77 ms against 1.38 ms for the split-K step launches, Jacobian
    // sweep of 250 knots 0.80 against 1.15 ms for the row-split cluster form.
    static const int gs_on = tune_int("DTO_SWEEP_GS", 1);  // A/B runs (TUNING builds): 0 = never, 2 = wherever it can run
    if (gs_on && s.q == 1 && s.n_cu >= 64 && !(s.shared_chip && gs_on != 2) &&
        (size_t)ty.T * s.Kpad * s.npad * 8 < (1ull << 31) &&   // 32-bit buffer offsets into a term slab
        sweep_gs_plan(s.npad, s.m, ty, s.n_int, s.n_cu, c.gs) && (gs_on == 2 || ty.T == 1 || !fused_alone))
        return c.is(SWEEP_GS);
    // Fused form (dto_sweep_fused.hip): the whole series in one persistent launch, a workgroup per few intervals; single-column
    // sweeps only in the 64-state generator-stationary instance.  Beside another stream's kernels the planner is asked again for
    // the shape it takes there (a refusal would fall through to the cluster form; see sweep_with in do_jacobian).
    if (fused_alone && (ty.T != 1 || c.fused.S64) &&
        (!s.shared_chip || sweep_fused_plan(s.npad, s.m, ty, s.n_int, s.n_cu, c.fused, s.shared_chip)))
        return c.is(c.fused.S64 ? SWEEP_S64 : SWEEP_FUSED);
    // Row-split cluster form: where the single-workgroup form has too few interval groups for the chip -- short shards of 128-
    // and 256-state problems (the 250-knot share of the 2000-knot metric on 8 GPUs).  Measured per Jacobian / Hessian,
    // cluster against step per launch (tools/cluster_time.py): 256 x 250 2.12 / 2.02 against 2.22 / 2.04 ms, 128 x 250 0.74 /
    // 1.02 against 0.93 / 1.18 ms.  NOT used where it measured slower: single-column sweeps (eval_constraint 0.94 against
    // 0.62 ms at 250 knots, 1.52 against 1.45 at 2000: the rendezvous + slice exchange costs ~10 us per Taylor step, as much
    // as the step's MFMA work there) and 512 / 1024 states (23.6 against 18.7 ms, 57 against 47 ms per Jacobian: the step
    // launches tile the 2500 columns 32 wide, a cluster member is held to 16 by its LDS).
    if (ty.T != 1 && sweep_cluster_plan(s.npad, s.m, ty, s.n_int, s.n_cu, c.cluster)) return c.is(SWEEP_CLUSTER);
    return c;   // one launch per Taylor step: what remains, and the form for frozen p terms and the products' extra start vector
}

// ------------------------------------------------------------------------------------------ 4. kernel instantiations

// One list per kernel family: what its *_prepare opts into the whole CU's LDS, what its launch dispatches over, and what
// tests/test_sweep_plan_header.py holds against everything choose_sweep returns.  A plan outside its list is an error of the launch.
// k_sweep_fused<MT, NT, WC, WK>: 64 MT states; WC = 2 column groups of wavefronts or WK = 2 waves per SIMD only at 256 states
#define DTO_SWEEP_FUSED_INSTANCES(X) \
    X(1, 1, 1, 1) X(1, 2, 1, 1) X(1, 3, 1, 1) X(2, 1, 1, 1) X(2, 2, 1, 1) X(2, 3, 1, 1) X(4, 1, 1, 2) X(4, 2, 1, 2) X(4, 3, 1, 2) X(4, 2, 2, 1)
// k_sweep_s64<MP, NX>: generator slots (s64_generator_slots) and the most inhomogeneous sources of a column type
#define DTO_SWEEP_S64_INSTANCES(X) X(3, 0) X(3, 1) X(3, 2) X(5, 0) X(5, 1) X(5, 2)
// k_sweep_cluster<MT, NT, R>: 128 states over 2 members, 256 states over 2 and over 4
#define DTO_SWEEP_CLUSTER_INSTANCES(X) X(1, 1, 2) X(1, 2, 2) X(2, 1, 2) X(2, 2, 2) X(1, 1, 4) X(1, 2, 4)
// k_sweep<TM, TN> and its FROZEN form: the tiles of the step-per-launch sweep (sweep_step_tile_rows)
#define DTO_SWEEP_STEP_TILES(X) X(64, 32) X(32, 32)

inline int s64_generator_slots(int m) { return m + 1 <= 3 ? 3 : 5; }

// Rows of a step launch's tile (32 columns either way) for `ny` column types or generators in grid.y: 64 x 32 measured fastest at
// 256 x 2000 (1280 workgroups = 5 per CU: balanced); smaller problems get 32 x 32 tiles so that the launch still covers the chip
// (-5..10 % per step at 64 and 128 states)
inline int sweep_step_tile_rows(int npad, int Kpad, int ny) { return (long)(npad / 64) * (Kpad / 32) * ny >= 1024 ? 64 : 32; }

}  // namespace dto
