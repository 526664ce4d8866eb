// dto_newton_plan.h -- the fixed-order reductions and the scalar decision of the truncated-Newton step (dto_projected_newton_step and
// its _dev form, dto_newton.hip; include/dto_engine.h, "Truncated-Newton step").  Plain C++ (no HIP header, no engine header), like
// dto_feasible_plan.h and dto_reduced_plan.h: the same text serves the kernels (dto_newton.hip), the host routine (dto_engine.cpp) and a
// g++-built test (tests/test_newton_plan_header.py).
//
// A dot x . y over n entries.  The entries are cut into chunks of NEWTON_CHUNK = 256; nb = newton_chunks(n).
//   stage 1, chunk b:  lane l (0 .. 63) starts from a_l = 0 and adds x_i y_i over i = 256 b + l, + 64, .. < min(256 (b + 1), n) ascending,
//                      a_l = a_l + x_i * y_i  (product and sum rounded on their own: newton_lane_dot);  the 64 lane sums are combined by the
//                      halving tree of k_feas_merit / k_red_input_transposed, for off = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_{l+off}  (l < off),
//                      and P_b = a_0.
//   stage 2:           ONE wavefront combines the P_b the same way: lane l starts from a_l = 0 and adds P_b over b = l, l + 64, .. < nb
//                      ascending (newton_lane_sum), then the halving tree; the dot is a_0.
// No atomics; an entry outside the free set enters as an exact zero (the vectors hold 0 there).  On the device the tree is six wavefront
// shuffles; newton_tree64 is the same tree on an array and newton_dot the whole dot on host arrays.
//
// The decision of iteration j from the five scalars (newton_decide): see the function.  Every product, sum, quotient and square root
// below is rounded on its own -- contraction is switched off where the operators are written (clang: the pragma; a g++ build of a test
// passes -ffp-contract=off).
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define NWT_HD __host__ __device__
#else
#define NWT_HD
#endif

#if defined(__clang__)
#define NWT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NWT_NO_CONTRACT
#endif

namespace dto {

constexpr int NEWTON_CHUNK = 256;   // entries per chunk: one wavefront, four entries per lane
constexpr int NEWTON_LANES = 64;

// status of a step (DTO_NEWTON_* in include/dto_engine.h); NEWTON_CONTINUE is the decision "take the CG step alpha and go on"
enum { NEWTON_CONTINUE = -1, NEWTON_CONVERGED = 0, NEWTON_BOUNDARY = 1, NEWTON_NEG_CURVATURE = 2, NEWTON_MAX_ITER = 3, NEWTON_NOT_FINITE = 4 };

// partial sums kept per chunk, [NEWTON_SLOTS][nb]: the four dots of the curvature pass, then the four behind the update (r . r, and
// what an exit reports: p . g, p . r, p . p)
enum { NWT_KAPPA = 0, NWT_DD = 1, NWT_PD = 2, NWT_PP = 3, NWT_RR = 4, NWT_PG = 5, NWT_PR = 6, NWT_PP_NEW = 7, NEWTON_SLOTS = 8 };
// the scalars on the device, NEWTON_STATE doubles: what the host reads back (status, iterations), then what one launch hands the next
enum { NWS_STATUS = 0, NWS_ITER = 1, NWS_RR0 = 2, NWS_RR = 3 /* two: iteration j reads [3 + (j - 1) % 2], writes [3 + j % 2] */,
       NWS_DECISION = 5, NWS_S = 6, NWS_KAPPA = 7, NWS_DD = 8, NWS_DOTS = 9 /* four: the dots of a combine launch (A/B form) */,
       NEWTON_STATE = 16 };

NWT_HD inline int64_t newton_chunks(int64_t n) { return (n + NEWTON_CHUNK - 1) / NEWTON_CHUNK; }
// doubles of the routine's workspace: r, d and y / w, the partial sums and the scalars
NWT_HD inline int64_t newton_workspace_doubles(int64_t n) { return 3 * n + NEWTON_SLOTS * newton_chunks(n) + NEWTON_STATE; }

NWT_HD inline double newton_mul(double a, double b) {
    NWT_NO_CONTRACT
    return a * b;
}
NWT_HD inline double newton_add(double a, double b) {
    NWT_NO_CONTRACT
    return a + b;
}
NWT_HD inline double newton_sub(double a, double b) {
    NWT_NO_CONTRACT
    return a - b;
}
NWT_HD inline double newton_div(double a, double b) {
    NWT_NO_CONTRACT
    return a / b;
}
NWT_HD inline bool newton_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// stage 1, lane `lane` of chunk b
NWT_HD inline double newton_lane_dot(const double* x, const double* y, int64_t n, int64_t b, int lane) {
    const int64_t end = (b + 1) * NEWTON_CHUNK < n ? (b + 1) * NEWTON_CHUNK : n;
    double a = 0.0;
    for (int64_t i = b * NEWTON_CHUNK + lane; i < end; i += NEWTON_LANES) a = newton_add(a, newton_mul(x[i], y[i]));
    return a;
}
// stage 2, lane `lane`
NWT_HD inline double newton_lane_sum(const double* P, int64_t nb, int lane) {
    double a = 0.0;
    for (int64_t b = lane; b < nb; b += NEWTON_LANES) a = newton_add(a, P[b]);
    return a;
}
// the halving tree on an array of 64 lane values; returns a_0
inline double newton_tree64(double* a) {
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) a[l] = newton_add(a[l], a[l + off]);
    return a[0];
}
// the dot of two host arrays in the stated order; P: scratch of newton_chunks(n) doubles
inline double newton_dot(const double* x, const double* y, int64_t n, double* P) {
    const int64_t nb = newton_chunks(n);
    double a[NEWTON_LANES];
    for (int64_t b = 0; b < nb; ++b) {
        for (int l = 0; l < NEWTON_LANES; ++l) a[l] = newton_lane_dot(x, y, n, b, l);
        P[b] = newton_tree64(a);
    }
    for (int l = 0; l < NEWTON_LANES; ++l) a[l] = newton_lane_sum(P, nb, l);
    return newton_tree64(a);
}

// tau >= 0 with ||p + tau d|| = radius:  (-pd + sqrt(pd * pd + dd * (radius * radius - pp))) / dd
NWT_HD inline double newton_tau(double dd, double pd, double pp, double radius) {
    const double disc = newton_add(newton_mul(pd, pd), newton_mul(dd, newton_sub(newton_mul(radius, radius), pp)));
    return newton_div(newton_add(-pd, sqrt(disc)), dd);
}

struct NewtonDecision {
    int status;   // NEWTON_CONTINUE, NEWTON_BOUNDARY, NEWTON_NEG_CURVATURE or NEWTON_NOT_FINITE
    double s;     // the step along d: alpha, tau, 1 or 0
};

// Iteration j (1-based) of Steihaug-Toint CG from kappa = d.w, dd = d.d, pd = p.d, pp = p.p and rr = r.r (radius = 0: no trust region):
//   kappa or rr not finite                           NOT_FINITE, s = 0 (p and r stay)
//   kappa <= 0                                       NEG_CURVATURE, s = tau with a radius, else 1 in the first iteration and 0 later
//   alpha = rr / kappa
//   radius > 0 and (pp + (2 * alpha) * pd) + (alpha * alpha) * dd >= radius * radius      BOUNDARY, s = tau
//   otherwise                                        CONTINUE, s = alpha
NWT_HD inline NewtonDecision newton_decide(double kappa, double dd, double pd, double pp, double rr, double radius, int j) {
    if (!newton_finite(kappa) || !newton_finite(rr)) return NewtonDecision{NEWTON_NOT_FINITE, 0.0};
    if (kappa <= 0.0) return NewtonDecision{NEWTON_NEG_CURVATURE, radius > 0.0 ? newton_tau(dd, pd, pp, radius) : (j == 1 ? 1.0 : 0.0)};
    const double alpha = newton_div(rr, kappa);
    if (radius > 0.0) {
        const double reach = newton_add(newton_add(pp, newton_mul(newton_mul(2.0, alpha), pd)), newton_mul(newton_mul(alpha, alpha), dd));
        if (reach >= newton_mul(radius, radius)) return NewtonDecision{NEWTON_BOUNDARY, newton_tau(dd, pd, pp, radius)};
    }
    return NewtonDecision{NEWTON_CONTINUE, alpha};
}

// the convergence test behind an update:  sqrt(rr_new) <= max(atol, rtol * sqrt(rr0))
NWT_HD inline bool newton_converged(double rr_new, double rr0, double rtol, double atol) {
    const double bar = newton_mul(rtol, sqrt(rr0));
    return sqrt(rr_new) <= (atol > bar ? atol : bar);
}

}  // namespace dto
