// dto_newton_box_plan.h -- the bound-constrained truncated-Newton step (dto_projected_newton_step_box and its _dev form,
// dto_newton_box.hip; include/dto_engine.h, "Bound-constrained truncated-Newton step") in plain C++ (no HIP header, no engine header):
// the entry rules, the scalar decision and the whole loop.  The dot order, newton_decide, newton_tau, newton_converged and the rounded
// operators are those of dto_newton_plan.h; every new expression is rounded on its own, in the operand order written.  The same text
// serves the kernels, the host routine (sizes) and a g++-built test (tests/test_newton_box_plan_header.py).
//
// Entry states (one byte per entry on the device):
//   0 fixed (dependent, or free_mask == 0.0)   1 free   2 / 3 held at the lower / upper bound from the start
//   4 / 5 hit the lower / upper bound during the call.
// F0 = the entries that are 1 behind the start (later 1, 4 or 5), F = the entries that are 1 now.  F only shrinks.
//
// The loop (newton_box_solve below is this text as a program; `apply` is y = T'HT d):
//   start      state by newton_box_classify;  r = g on F0, 0 elsewhere;  p = 0;  d = -r;  rr0 = rr = r . r;  rr == 0: CONVERGED, 0 iterations
//   iteration j = 1 .. max_iter
//     y = apply(d);  w = y + shift * d on F0, 0 elsewhere
//     kappa = d . w, dd = d . d, pd = p . d, pp = p . p                       (dto_newton_plan.h's order)
//     t_i = newton_box_breakpoint(..) on F;  tau_box = the minimum of the t_i that are no NaN, +inf without one
//     (status, s) = newton_box_decide(kappa, dd, pd, pp, rr, radius, tau_box, j)
//     unless NOT_FINITE:  p = p + s * d,  r = r + s * w  on every entry;  then on F, with t_i from the p BEFORE the update:
//         d_i > 0 and (t_i <= s or Z_i + p_i >= hi_i):  p_i = hi_i - Z_i, state 5
//         d_i < 0 and (t_i <= s or Z_i + p_i <= lo_i):  p_i = lo_i - Z_i, state 4           n_hit = the entries so fixed
//     rr' = r . r over the new F;  p . g (g on F0), p . r, p . p over all entries
//     BOUNDARY, NEG_CURVATURE, NOT_FINITE: stop
//     CONTINUE: sqrt(rr') <= max(atol, rtol * sqrt(rr0)): CONVERGED, stop
//               n_hit > 0:  restart, d = -r on F and 0 elsewhere;   else beta = rr' / rr, d = beta * d - r, and 0 on states 4 / 5
//               rr = rr';  j == max_iter: MAX_ITER
// r is kept on all of F0 and is not corrected for the rounding of a clamp, so r = g + A0 p holds on F0 up to that rounding and the
// predicted decrease -0.5 (p . g + p . r) stays the model's after a restart.  A minimum is exact, so the tree that forms tau_box does not
// matter; n_hit, the held count and |F| are integer counts, exact in doubles in any order.  With lo = -inf and hi = +inf everywhere no
// entry is held or hit, tau_box = +inf, and the loop is dto_projected_newton_step's bit for bit.
#pragma once

#include <cstdint>
#include <vector>

#include "dto_newton_plan.h"

namespace dto {

enum { NBOX_FIXED = 0, NBOX_FREE = 1, NBOX_HELD_LO = 2, NBOX_HELD_HI = 3, NBOX_HIT_LO = 4, NBOX_HIT_HI = 5 };

// partial results kept per chunk, [NEWTON_BOX_SLOTS][nb]: the curvature pass writes 0 .. 4 (NBX_TMIN is a minimum, the others sums), the
// update pass 5 .. 10, the start 5 .. 11 (6 .. 9 as zeros)
enum { NBX_KAPPA = 0, NBX_DD = 1, NBX_PD = 2, NBX_PP = 3, NBX_TMIN = 4, NBX_RR = 5, NBX_NHIT = 6, NBX_PG = 7, NBX_PR = 8, NBX_PP_NEW = 9,
       NBX_NFREE = 10, NBX_HELD = 11, NEWTON_BOX_SLOTS = 12 };
// the scalars on the device, NEWTON_BOX_STATE doubles.  Iteration j reads the slots [.. + (j - 1) % 2] of rr, hits and restarts and
// writes [.. + j % 2], so no launch reads a scalar it writes.
enum { NBS_STATUS = 0, NBS_ITER = 1, NBS_RR0 = 2, NBS_RR = 3 /* two */, NBS_DECISION = 5, NBS_S = 6, NBS_KAPPA = 7, NBS_DD = 8, NBS_HELD = 9,
       NBS_HITS = 10 /* two */, NBS_RESTARTS = 12 /* two */, NEWTON_BOX_STATE = 16 };
constexpr int NEWTON_BOX_INFO = 12, NEWTON_BOX_TRACE = 6;

// doubles of the routine's workspace: r, d and y / w, the partial results, the scalars, and the state bytes (eight to a double)
NWT_HD inline int64_t newton_box_workspace_doubles(int64_t n) {
    return 3 * n + NEWTON_BOX_SLOTS * newton_chunks(n) + NEWTON_BOX_STATE + (n + 7) / 8;
}

NWT_HD inline double newton_box_inf() { return __builtin_huge_val(); }
NWT_HD inline bool newton_box_in_f0(int state) { return state == NBOX_FREE || state >= NBOX_HIT_LO; }

// the state of an entry that is not fixed, from Z_i, its bounds and the reduced gradient g_i; the lower bound is tested first
NWT_HD inline int newton_box_classify(double z, double lo, double hi, double g) {
    if (z <= lo && g > 0.0) return NBOX_HELD_LO;
    if (z >= hi && g < 0.0) return NBOX_HELD_HI;
    return NBOX_FREE;
}

// the step along d at which a free entry reaches its bound: max(0, (hi - (Z + p)) / d) for d > 0, the same with lo for d < 0;
// +inf for d == 0.  A NaN is returned as it is (it takes no part in the minimum and `t <= s` is false); -0 becomes +0.
NWT_HD inline double newton_box_breakpoint(double z, double p, double d, double lo, double hi) {
    if (d > 0.0) {
        const double q = newton_div(newton_sub(hi, newton_add(z, p)), d);
        return q != q ? q : (q > 0.0 ? q : 0.0);
    }
    if (d < 0.0) {
        const double q = newton_div(newton_sub(lo, newton_add(z, p)), d);
        return q != q ? q : (q > 0.0 ? q : 0.0);
    }
    return newton_box_inf();
}
// min that skips a NaN t
NWT_HD inline double newton_box_min(double m, double t) { return t < m ? t : m; }

// the halving tree of minima on 64 lane values (the device form is six shuffles); returns a_0
inline double newton_box_mintree64(double* a) {
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) a[l] = newton_box_min(a[l], a[l + off]);
    return a[0];
}

// newton_decide, then the box: a step longer than tau_box stops at the face and the solve goes on; non-positive curvature without a
// radius follows d to the face when there is one.
NWT_HD inline NewtonDecision newton_box_decide(double kappa, double dd, double pd, double pp, double rr, double radius, double tau_box, int j) {
    const NewtonDecision D = newton_decide(kappa, dd, pd, pp, rr, radius, j);
    if (D.status == NEWTON_NOT_FINITE) return D;
    if (D.status == NEWTON_NEG_CURVATURE && radius == 0.0 && newton_finite(tau_box)) return NewtonDecision{NEWTON_CONTINUE, tau_box};
    if (D.s > tau_box) return NewtonDecision{NEWTON_CONTINUE, tau_box};
    return D;
}

// the update of one entry behind the decision (not called after NOT_FINITE): p and r move, a free entry that reaches its bound is
// clamped onto it.  t: its breakpoint from the p before the update.  Returns the new state.
NWT_HD inline int newton_box_update(int state, double z, double lo, double hi, double d, double w, double s, double t, double* p, double* r) {
    *p = newton_add(*p, newton_mul(s, d));
    *r = newton_add(*r, newton_mul(s, w));
    if (state != NBOX_FREE) return state;
    if (d > 0.0 && (t <= s || newton_add(z, *p) >= hi)) {
        *p = newton_sub(hi, z);
        return NBOX_HIT_HI;
    }
    if (d < 0.0 && (t <= s || newton_add(z, *p) <= lo)) {
        *p = newton_sub(lo, z);
        return NBOX_HIT_LO;
    }
    return state;
}

// Z + p as the next point: the bound itself, exactly, where the entry was hit
NWT_HD inline double newton_box_point(int state, double z, double p, double lo, double hi) {
    return state == NBOX_HIT_LO ? lo : state == NBOX_HIT_HI ? hi : newton_add(z, p);
}

// the direction behind a CG step without a hit (restart = false) or behind a hit (restart = true)
NWT_HD inline double newton_box_direction(int state, bool restart, double beta, double d, double r) {
    if (restart) return state == NBOX_FREE ? -r : 0.0;
    return state >= NBOX_HIT_LO ? 0.0 : newton_sub(newton_mul(beta, d), r);
}

// ---- the whole loop on host arrays (the statement of the algorithm; the device routine is these steps as launches) --------------------
// fixed[i] != 0: entry i is dependent or masked.  lo / hi may be null.  apply(d, y): y = T'HT d.  p [n], info [12]; trace [max_iter][6],
// entry_state [n] and zp [n] may be null.  Rows of the trace past the last iteration are left as they are.
template <class Apply>
inline void newton_box_solve(int64_t n, const double* Z, const double* g, const unsigned char* fixed, const double* lo, const double* hi,
                             double radius, double shift, double rtol, double atol, int max_iter, Apply&& apply, double* p, double* info,
                             double* trace, double* entry_state, double* zp) {
    const int64_t nb = newton_chunks(n);
    const double inf = newton_box_inf();
    std::vector<double> r((size_t)n), d((size_t)n), w((size_t)n), gm((size_t)n), t((size_t)n), P((size_t)nb), one((size_t)n, 1.0), ind((size_t)n);
    std::vector<int> st((size_t)n);
    auto LO = [&](int64_t i) { return lo ? lo[i] : -inf; };
    auto HI = [&](int64_t i) { return hi ? hi[i] : inf; };
    auto count = [&](auto&& pred) {   // an integer count through the dot's order (exact in any order)
        for (int64_t i = 0; i < n; ++i) ind[(size_t)i] = pred(st[(size_t)i]) ? 1.0 : 0.0;
        return newton_dot(ind.data(), one.data(), n, P.data());
    };
    auto rr_free = [&] {
        for (int64_t i = 0; i < n; ++i) ind[(size_t)i] = st[(size_t)i] == NBOX_FREE ? r[(size_t)i] : 0.0;
        return newton_dot(ind.data(), ind.data(), n, P.data());
    };
    for (int64_t i = 0; i < n; ++i) {
        st[(size_t)i] = fixed[i] ? NBOX_FIXED : newton_box_classify(Z[i], LO(i), HI(i), g[i]);
        gm[(size_t)i] = r[(size_t)i] = st[(size_t)i] == NBOX_FREE ? g[i] : 0.0;
        p[i] = 0.0;
        d[(size_t)i] = -r[(size_t)i];
    }
    const double held = count([](int s) { return s == NBOX_HELD_LO || s == NBOX_HELD_HI; });
    const double rr0 = rr_free();
    double rr = rr0, rr_new = rr0, hits = 0.0, restarts = 0.0, kappa = 0.0, dd = 0.0;
    int status = rr0 == 0.0 ? NEWTON_CONVERGED : NEWTON_CONTINUE, j = 0;
    while (status == NEWTON_CONTINUE && j < max_iter) {
        ++j;
        apply(d.data(), w.data());
        double tau_box = inf;
        for (int64_t i = 0; i < n; ++i) {
            const int s = st[(size_t)i];
            w[(size_t)i] = newton_box_in_f0(s) ? newton_add(w[(size_t)i], newton_mul(shift, d[(size_t)i])) : 0.0;
            t[(size_t)i] = s == NBOX_FREE ? newton_box_breakpoint(Z[i], p[i], d[(size_t)i], LO(i), HI(i)) : inf;
            tau_box = newton_box_min(tau_box, t[(size_t)i]);
        }
        kappa = newton_dot(d.data(), w.data(), n, P.data());
        dd = newton_dot(d.data(), d.data(), n, P.data());
        const double pd = newton_dot(p, d.data(), n, P.data()), pp = newton_dot(p, p, n, P.data());
        const NewtonDecision D = newton_box_decide(kappa, dd, pd, pp, rr, radius, tau_box, j);
        double n_hit = 0.0;
        if (D.status != NEWTON_NOT_FINITE)
            for (int64_t i = 0; i < n; ++i) {
                const int s = newton_box_update(st[(size_t)i], Z[i], LO(i), HI(i), d[(size_t)i], w[(size_t)i], D.s, t[(size_t)i], &p[i], &r[(size_t)i]);
                if (s != st[(size_t)i]) n_hit += 1.0;
                st[(size_t)i] = s;
            }
        rr_new = rr_free();
        hits += n_hit;
        if (trace) {
            double* row = trace + NEWTON_BOX_TRACE * (size_t)(j - 1);
            row[0] = kappa; row[1] = dd; row[2] = D.s; row[3] = rr_new; row[4] = tau_box; row[5] = n_hit;
        }
        status = D.status;
        if (status == NEWTON_CONTINUE && newton_converged(rr_new, rr0, rtol, atol)) status = NEWTON_CONVERGED;
        if (status != NEWTON_CONTINUE) break;
        const bool restart = n_hit > 0.0;
        const double beta = restart ? 0.0 : newton_div(rr_new, rr);
        for (int64_t i = 0; i < n; ++i) d[(size_t)i] = newton_box_direction(st[(size_t)i], restart, beta, d[(size_t)i], r[(size_t)i]);
        if (restart) restarts += 1.0;
        rr = rr_new;
        if (j == max_iter) status = NEWTON_MAX_ITER;
    }
    const double pg = newton_dot(p, gm.data(), n, P.data()), pr = newton_dot(p, r.data(), n, P.data()), pp = newton_dot(p, p, n, P.data());
    info[0] = (double)status;
    info[1] = (double)j;
    info[2] = sqrt(rr0);
    info[3] = sqrt(rr_new);
    info[4] = sqrt(pp);
    info[5] = pg;
    info[6] = newton_mul(-0.5, newton_add(pg, pr));
    info[7] = j >= 1 ? newton_div(kappa, dd) : 0.0;
    info[8] = held;
    info[9] = hits;
    info[10] = restarts;
    info[11] = count([](int s) { return s == NBOX_FREE; });
    for (int64_t i = 0; i < n; ++i) {
        if (entry_state) entry_state[i] = (double)st[(size_t)i];
        if (zp) zp[i] = newton_box_point(st[(size_t)i], Z[i], p[i], LO(i), HI(i));
    }
}

}  // namespace dto
