// dto_precond_plan.h -- the L-BFGS preconditioner of the bound-constrained truncated-Newton step (dto_preconditioned_newton_step,
// dto_newton_precondition, dto_newton_pairs_* and their _dev forms, dto_precond.hip; include/dto_engine.h, "Preconditioned truncated-Newton
// step") in plain C++ (no HIP header, no engine header): the pair store, the preparation, the application and the whole loop.  The dot
// order, the decision, the entry rules and the rounded operators are those of dto_newton_plan.h and dto_newton_box_plan.h; every new
// expression is rounded on its own, in the operand order written.  The same text serves the kernels, the host routine (sizes) and a
// g++-built test (tests/test_precond_plan_header.py).
//
// Pair store.  Up to m <= 16 pairs (s_k, y_k), raw vectors in the Z layout, k = 0 the oldest.  Two banks of 2 m vectors each; a bank
// is a ring: pair k lies in slot (head + k) % m.  A step reads the current bank and, with `harvest`, writes the other one; the banks
// swap when the call ends if it took a pair.  2 banks * 2 m * n doubles (precond_store_doubles).
//
// Preparation, once per call, behind the entry states (F0 = the entries that are free behind the start).  x~ is x on F0 and 0 elsewhere.
//   Gram entries in the dot order of dto_newton_plan.h:  SY_ij = s~_i . y~_j and YY_ij = y~_i . y~_j for i <= j, SS_ii = s~_i . s~_i
//   admission, oldest to newest:  pair k is admitted iff SY_kk, SS_kk, YY_kk are finite and SY_kk > PRECOND_EPS * sqrt(SS_kk * YY_kk)
//   gamma = SY_kk / YY_kk of the newest admitted pair; without one gamma = 1 and the operator is the identity
//   over the admitted pairs a, b = 0 .. q - 1 (ascending age order kept):  R_ab = SY_ab (a <= b),  M_ab = gamma * YY_ab, + SY_aa on the diagonal
// Application z = P_F H P_F r, F the entries free now (F is a subset of F0), the compact form of Byrd, Nocedal and Schnabel:
//   u_a = s~_a . r_F,  v_a = y~_a . r_F                      (the vectors masked to F; the dot order again)
//   a = R^-1 u            back substitution:  t = u_i;  t = t - R_ik a_k for k = i + 1 .. q - 1 ascending;  a_i = t / R_ii;  i = q - 1 .. 0
//   b_i = (sum over k ascending, from 0, of M_ik a_k) - gamma * v_i
//   c1 = R^-T b           forward substitution:  t = b_i;  t = t - R_ki c1_k for k = 0 .. i - 1 ascending;  c1_i = t / R_ii;  c2 = -a
//   z_i = (gamma * r_i + A1) + gamma * A2 on F, 0 elsewhere;  A1 = sum over a ascending, from 0, of c1_a * s_a,i;  A2 likewise of c2_a * y_a,i
//   without an admitted pair (or switched off): z_i = r_i on F, 0 elsewhere, so that r . z is r . r over F bit for bit
// The operator is a principal submatrix of a positive definite matrix whenever the admitted pairs have one, so no Gram matrix is
// rebuilt when an entry hits a bound.
//
// The loop (precond_solve below) is newton_box_solve with these changes and no others:
//   z is formed from r behind the start and behind every update (also behind the last one);  rz = r . z over F
//   rz takes rr's place in the decision (alpha = rz / kappa) and in beta = rz' / rz;  d = beta * d - z;  the start is d = -z, a restart
//   d = -z on F and 0 elsewhere;  convergence, reach, tau, tau_box, the clamps, the predicted decrease and info[0 .. 11] stay Euclidean
//   fallback: where the loop goes on (behind the start, or behind a CG step that did not converge) with the preconditioner on and rz'
//   not finite or <= 0, it is switched off for the rest of the call: rz' = rr', d = -r (the start's or the restart's form), one
//   fallback is counted
//   harvest: iteration j offers (d, w) as the loop holds them behind the curvature pass (w = y + shift d on F0); the pair is taken iff
//   kappa is finite and > 0; take t (0-based) goes to slot t % m of the other bank
//   info [16]: the box step's 12, the pairs admitted, the pairs taken, the fallbacks, sqrt(rz0) (rz0 behind a fallback of the start: rr0)
//   trace [max_iter][8]: the box step's six columns, rz' as formed, and 1 / 0: the preconditioner is on / off behind the iteration
#pragma once

#include <cstdint>
#include <vector>

#include "dto_newton_box_plan.h"

namespace dto {

constexpr int PRECOND_MAX_PAIRS = 16;
// the admission bar on the cosine between s~ and y~: 2^-26, the square root of the unit roundoff.  A pair (d, A d) of CG on a positive
// definite A has a cosine of at least 2 sqrt(cond) / (cond + 1), so every such pair with cond(A) < 1.8e16 is admitted; below the bar
// the rounding of the two dots leaves no digit of the curvature s . y.
constexpr double PRECOND_EPS = 1.4901161193847656e-08;

// partial results per chunk: the box step's twelve slots, then r . z
enum { NPX_RZ = NEWTON_BOX_SLOTS, PRECOND_SLOTS = NEWTON_BOX_SLOTS + 1 };
// the scalars on the device, PRECOND_STATE doubles.  [0 .. 2] are what the host reads back.  The pairs marked `two` alternate as in
// the box step: iteration j reads [.. + (j - 1) % 2] and writes [.. + j % 2].
enum { NPS_STATUS = 0, NPS_ITER = 1, NPS_TAKEN_OUT = 2, NPS_RR0 = 3, NPS_RZ = 4 /* two */, NPS_DECISION = 6, NPS_S = 7, NPS_KAPPA = 8, NPS_DD = 9,
       NPS_HELD = 10, NPS_HITS = 11 /* two */, NPS_RESTARTS = 13 /* two */, NPS_ACTIVE = 15 /* two */, NPS_TAKEN = 17 /* two */,
       NPS_FALLBACKS = 19 /* two */, NPS_RZ0 = 21, NPS_TOOK = 22, PRECOND_STATE = 24 };
constexpr int PRECOND_INFO = 16, PRECOND_TRACE = 8;
// the prepared system, PRECOND_PC doubles: q, gamma, the admitted pairs' indices, R [16][16] (upper triangle used), M [16][16]
enum { PPC_NADM = 0, PPC_GAMMA = 1, PPC_IDX = 2, PPC_R = PPC_IDX + PRECOND_MAX_PAIRS, PPC_M = PPC_R + PRECOND_MAX_PAIRS * PRECOND_MAX_PAIRS,
       PRECOND_PC = PPC_M + PRECOND_MAX_PAIRS * PRECOND_MAX_PAIRS };

// the Gram entries of cnt pairs: SY_ij at precond_tri(i, j), YY_ij at T + precond_tri(i, j), SS_ii at 2 T + i;  T = cnt (cnt + 1) / 2
NWT_HD inline int precond_tri(int i, int j) { return j * (j + 1) / 2 + i; }   // i <= j
NWT_HD inline int precond_gram_count(int cnt) { return cnt * (cnt + 1) + cnt; }
constexpr int PRECOND_GRAM_MAX = PRECOND_MAX_PAIRS * (PRECOND_MAX_PAIRS + 1) + PRECOND_MAX_PAIRS;

NWT_HD inline int precond_slot(int head, int k, int m) { return (head + k) % m; }
NWT_HD inline int64_t precond_store_doubles(int64_t n, int m) { return 4 * (int64_t)m * n; }
// doubles of the routine's workspace: r, d, y / w and z, the partial results, the partial sums of 2 cnt dots and of the Gram entries,
// the scalars, the prepared system and the state bytes
NWT_HD inline int64_t precond_workspace_doubles(int64_t n, int cnt) {
    return 4 * n + (PRECOND_SLOTS + 2 * cnt + precond_gram_count(cnt)) * newton_chunks(n) + PRECOND_STATE + PRECOND_PC + (n + 7) / 8;
}

NWT_HD inline bool precond_rz_bad(double rz) { return !(newton_finite(rz) && rz > 0.0); }
NWT_HD inline bool precond_takes(double kappa) { return newton_finite(kappa) && kappa > 0.0; }

// admission and the prepared system from the Gram entries G [precond_gram_count(cnt)]
NWT_HD inline void precond_prepare(int cnt, const double* G, double* pc) {
    const int T = cnt * (cnt + 1) / 2;
    int q = 0, idx[PRECOND_MAX_PAIRS];
    for (int k = 0; k < cnt; ++k) {
        const double sy = G[precond_tri(k, k)], yy = G[T + precond_tri(k, k)], ss = G[2 * T + k];
        if (newton_finite(sy) && newton_finite(ss) && newton_finite(yy) && sy > newton_mul(PRECOND_EPS, sqrt(newton_mul(ss, yy)))) idx[q++] = k;
    }
    double gamma = 1.0;
    if (q > 0) gamma = newton_div(G[precond_tri(idx[q - 1], idx[q - 1])], G[T + precond_tri(idx[q - 1], idx[q - 1])]);
    pc[PPC_NADM] = (double)q;
    pc[PPC_GAMMA] = gamma;
    for (int a = 0; a < PRECOND_MAX_PAIRS; ++a) pc[PPC_IDX + a] = a < q ? (double)idx[a] : 0.0;
    for (int a = 0; a < PRECOND_MAX_PAIRS; ++a)
        for (int b = 0; b < PRECOND_MAX_PAIRS; ++b) {
            double r = 0.0, m = 0.0;
            if (a < q && b < q) {
                const int lo = a <= b ? idx[a] : idx[b], hi = a <= b ? idx[b] : idx[a];
                if (a <= b) r = G[precond_tri(lo, hi)];
                m = newton_mul(gamma, G[T + precond_tri(lo, hi)]);
                if (a == b) m = newton_add(G[precond_tri(lo, hi)], m);
            }
            pc[PPC_R + a * PRECOND_MAX_PAIRS + b] = r;
            pc[PPC_M + a * PRECOND_MAX_PAIRS + b] = m;
        }
}

// the two triangular solves: c1, c2 [q] from u, v [cnt] (indexed by pair, the admitted ones are read)
NWT_HD inline void precond_coeffs(const double* pc, const double* u, const double* v, double* c1, double* c2) {
    const int q = (int)pc[PPC_NADM];
    const double gamma = pc[PPC_GAMMA];
    const double *R = pc + PPC_R, *M = pc + PPC_M;
    double a[PRECOND_MAX_PAIRS];
    for (int i = q - 1; i >= 0; --i) {
        double t = u[(int)pc[PPC_IDX + i]];
        for (int k = i + 1; k < q; ++k) t = newton_sub(t, newton_mul(R[i * PRECOND_MAX_PAIRS + k], a[k]));
        a[i] = newton_div(t, R[i * PRECOND_MAX_PAIRS + i]);
    }
    for (int i = 0; i < q; ++i) {
        double acc = 0.0;
        for (int k = 0; k < q; ++k) acc = newton_add(acc, newton_mul(M[i * PRECOND_MAX_PAIRS + k], a[k]));
        double t = newton_sub(acc, newton_mul(gamma, v[(int)pc[PPC_IDX + i]]));
        for (int k = 0; k < i; ++k) t = newton_sub(t, newton_mul(R[k * PRECOND_MAX_PAIRS + i], c1[k]));
        c1[i] = newton_div(t, R[i * PRECOND_MAX_PAIRS + i]);
        c2[i] = -a[i];
    }
}

// one term of A1 or A2, and the entry of z from them
NWT_HD inline double precond_acc(double acc, double c, double x) { return newton_add(acc, newton_mul(c, x)); }
NWT_HD inline double precond_entry(double gamma, double r, double a1, double a2) {
    return newton_add(newton_add(newton_mul(gamma, r), a1), newton_mul(gamma, a2));
}

// the direction: mode 0 the beta step (x = z), 1 a restart or a fallback behind an iteration (x = z or r), 2 the start (x = z or r)
enum { PRECOND_DIR_BETA = 0, PRECOND_DIR_RESTART = 1, PRECOND_DIR_START = 2 };
NWT_HD inline double precond_direction(int state, int mode, double beta, double d, double x) {
    if (mode == PRECOND_DIR_START) return -x;
    if (mode == PRECOND_DIR_RESTART) return state == NBOX_FREE ? -x : 0.0;
    return state >= NBOX_HIT_LO ? 0.0 : newton_sub(newton_mul(beta, d), x);
}

// ---- the application on host arrays: st the entry states (F0 for the Gram pass is `in_f0`), S / Y [cnt][n] with pair 0 the oldest ----
struct PrecondHost {
    int64_t n = 0;
    int cnt = 0;
    const double *S = nullptr, *Y = nullptr;
    double pc[PRECOND_PC];
    std::vector<double> a, b, P;

    // Gram entries over the entries with f0[i] != 0, then precond_prepare
    void prepare(int64_t n_, int cnt_, const double* S_, const double* Y_, const unsigned char* f0) {
        n = n_; cnt = cnt_; S = S_; Y = Y_;
        a.assign((size_t)n, 0.0); b.assign((size_t)n, 0.0); P.assign((size_t)newton_chunks(n), 0.0);
        pc[PPC_NADM] = 0.0; pc[PPC_GAMMA] = 1.0;
        if (cnt == 0) return;
        const int T = cnt * (cnt + 1) / 2;
        std::vector<double> G((size_t)precond_gram_count(cnt));
        auto masked = [&](const double* x, std::vector<double>& o) { for (int64_t i = 0; i < n; ++i) o[(size_t)i] = f0[i] ? x[i] : 0.0; };
        for (int j = 0; j < cnt; ++j) {
            masked(Y + (size_t)j * n, b);
            for (int i = 0; i <= j; ++i) {
                masked(S + (size_t)i * n, a);
                G[(size_t)precond_tri(i, j)] = newton_dot(a.data(), b.data(), n, P.data());
                if (i == j) G[(size_t)(2 * T + j)] = newton_dot(a.data(), a.data(), n, P.data());
                masked(Y + (size_t)i * n, a);
                G[(size_t)(T + precond_tri(i, j))] = newton_dot(a.data(), b.data(), n, P.data());
            }
        }
        precond_prepare(cnt, G.data(), pc);
    }
    int admitted() const { return (int)pc[PPC_NADM]; }
    // z from r over the entries with f[i] != 0 (on = false: the identity on F); returns r . z over F
    double apply(const double* r, const unsigned char* f, bool on, double* z) {
        const int q = admitted();
        std::vector<double> rf((size_t)n);
        for (int64_t i = 0; i < n; ++i) rf[(size_t)i] = f[i] ? r[i] : 0.0;
        if (on && q > 0) {
            double u[PRECOND_MAX_PAIRS], v[PRECOND_MAX_PAIRS], c1[PRECOND_MAX_PAIRS], c2[PRECOND_MAX_PAIRS];
            for (int k = 0; k < cnt; ++k) {
                for (int64_t i = 0; i < n; ++i) a[(size_t)i] = f[i] ? S[(size_t)k * n + i] : 0.0;
                u[k] = newton_dot(a.data(), rf.data(), n, P.data());
                for (int64_t i = 0; i < n; ++i) a[(size_t)i] = f[i] ? Y[(size_t)k * n + i] : 0.0;
                v[k] = newton_dot(a.data(), rf.data(), n, P.data());
            }
            precond_coeffs(pc, u, v, c1, c2);
            for (int64_t i = 0; i < n; ++i) {
                double a1 = 0.0, a2 = 0.0;
                for (int e = 0; e < q; ++e) {
                    const size_t k = (size_t)pc[PPC_IDX + e];
                    a1 = precond_acc(a1, c1[e], S[k * n + i]);
                    a2 = precond_acc(a2, c2[e], Y[k * n + i]);
                }
                z[i] = f[i] ? precond_entry(pc[PPC_GAMMA], r[i], a1, a2) : 0.0;
            }
        } else {
            for (int64_t i = 0; i < n; ++i) z[i] = rf[(size_t)i];
        }
        return newton_dot(rf.data(), z, n, P.data());
    }
};

// ---- the whole loop on host arrays: newton_box_solve's arguments, then the pairs (S / Y [cnt][n], pair 0 the oldest), the capacity m,
// `harvest` and the other bank HS / HY [m][n] as a ring (take t in slot t % m; may be null without harvest).  info [16], trace
// [max_iter][8].
template <class Apply>
inline void precond_solve(int64_t n, const double* Z, const double* g, const unsigned char* fixed, const double* lo, const double* hi,
                          double radius, double shift, double rtol, double atol, int max_iter, Apply&& apply, int cnt, const double* S,
                          const double* Y, int m, int harvest, double* HS, double* HY, double* p, double* info, double* trace,
                          double* entry_state, double* zp) {
    const int64_t nb = newton_chunks(n);
    const double inf = newton_box_inf();
    std::vector<double> r((size_t)n), d((size_t)n), w((size_t)n), z((size_t)n), gm((size_t)n), t((size_t)n), P((size_t)nb), one((size_t)n, 1.0), ind((size_t)n);
    std::vector<int> st((size_t)n);
    std::vector<unsigned char> f((size_t)n);
    auto LO = [&](int64_t i) { return lo ? lo[i] : -inf; };
    auto HI = [&](int64_t i) { return hi ? hi[i] : inf; };
    auto count = [&](auto&& pred) {
        for (int64_t i = 0; i < n; ++i) ind[(size_t)i] = pred(st[(size_t)i]) ? 1.0 : 0.0;
        return newton_dot(ind.data(), one.data(), n, P.data());
    };
    auto rr_free = [&] {
        for (int64_t i = 0; i < n; ++i) ind[(size_t)i] = st[(size_t)i] == NBOX_FREE ? r[(size_t)i] : 0.0;
        return newton_dot(ind.data(), ind.data(), n, P.data());
    };
    auto free_now = [&] {
        for (int64_t i = 0; i < n; ++i) f[(size_t)i] = st[(size_t)i] == NBOX_FREE;
        return f.data();
    };
    for (int64_t i = 0; i < n; ++i) {
        st[(size_t)i] = fixed[i] ? NBOX_FIXED : newton_box_classify(Z[i], LO(i), HI(i), g[i]);
        gm[(size_t)i] = r[(size_t)i] = st[(size_t)i] == NBOX_FREE ? g[i] : 0.0;
        p[i] = 0.0;
    }
    const double held = count([](int s) { return s == NBOX_HELD_LO || s == NBOX_HELD_HI; });
    const double rr0 = rr_free();
    PrecondHost H;
    H.prepare(n, cnt, S, Y, free_now());
    bool on = H.admitted() > 0;
    double rz = H.apply(r.data(), free_now(), on, z.data());
    int status = rr0 == 0.0 ? NEWTON_CONVERGED : NEWTON_CONTINUE, j = 0;
    double fallbacks = 0.0, taken = 0.0;
    if (status == NEWTON_CONTINUE && on && precond_rz_bad(rz)) {
        on = false;
        fallbacks = 1.0;
        rz = rr0;
    }
    const double rz0 = rz;
    for (int64_t i = 0; i < n; ++i) d[(size_t)i] = precond_direction(st[(size_t)i], PRECOND_DIR_START, 0.0, 0.0, fallbacks > 0.0 ? r[(size_t)i] : z[(size_t)i]);
    double rr_new = rr0, hits = 0.0, restarts = 0.0, kappa = 0.0, dd = 0.0;
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
        const NewtonDecision D = newton_box_decide(kappa, dd, pd, pp, rz, radius, tau_box, j);
        if (harvest && precond_takes(kappa)) {
            const size_t slot = (size_t)((int64_t)taken % m);
            for (int64_t i = 0; i < n; ++i) {
                HS[slot * n + i] = d[(size_t)i];
                HY[slot * n + i] = w[(size_t)i];
            }
            taken += 1.0;
        }
        double n_hit = 0.0;
        if (D.status != NEWTON_NOT_FINITE)
            for (int64_t i = 0; i < n; ++i) {
                const int s = newton_box_update(st[(size_t)i], Z[i], LO(i), HI(i), d[(size_t)i], w[(size_t)i], D.s, t[(size_t)i], &p[i], &r[(size_t)i]);
                if (s != st[(size_t)i]) n_hit += 1.0;
                st[(size_t)i] = s;
            }
        rr_new = rr_free();
        hits += n_hit;
        const double rz_new = H.apply(r.data(), free_now(), on, z.data());
        status = D.status;
        if (status == NEWTON_CONTINUE && newton_converged(rr_new, rr0, rtol, atol)) status = NEWTON_CONVERGED;
        const bool fallback = status == NEWTON_CONTINUE && on && precond_rz_bad(rz_new);
        if (fallback) {
            on = false;
            fallbacks += 1.0;
        }
        if (trace) {
            double* row = trace + PRECOND_TRACE * (size_t)(j - 1);
            row[0] = kappa; row[1] = dd; row[2] = D.s; row[3] = rr_new; row[4] = tau_box; row[5] = n_hit; row[6] = rz_new; row[7] = on ? 1.0 : 0.0;
        }
        if (status != NEWTON_CONTINUE) break;
        const bool restart = n_hit > 0.0;
        const double rz_use = fallback ? rr_new : rz_new;
        const int mode = restart || fallback ? PRECOND_DIR_RESTART : PRECOND_DIR_BETA;
        const double beta = mode == PRECOND_DIR_BETA ? newton_div(rz_use, rz) : 0.0;
        for (int64_t i = 0; i < n; ++i) d[(size_t)i] = precond_direction(st[(size_t)i], mode, beta, d[(size_t)i], fallback ? r[(size_t)i] : z[(size_t)i]);
        if (restart) restarts += 1.0;
        rz = rz_use;
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
    info[12] = (double)H.admitted();
    info[13] = taken;
    info[14] = fallbacks;
    info[15] = sqrt(rz0);
    for (int64_t i = 0; i < n; ++i) {
        if (entry_state) entry_state[i] = (double)st[(size_t)i];
        if (zp) zp[i] = newton_box_point(st[(size_t)i], Z[i], p[i], LO(i), HI(i));
    }
}

}  // namespace dto
