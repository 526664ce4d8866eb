// dto_auglag_plan.h -- the row rules of the augmented-Lagrangian terms (dto_auglag_rows, dto_auglag_merit, dto_auglag_gradient,
// dto_auglag_hessian_products, dto_auglag_newton_step and their _dev forms, dto_auglag.hip; include/dto_engine.h, "Augmented-Lagrangian
// terms") in plain C++ (no HIP header, no engine header).  The rounded operators are those of dto_newton_plan.h; every product, sum and
// quotient below is rounded on its own, in the operand order written.  The same text serves the kernels, the host routines and a
// g++-built test (tests/test_auglag_plan_header.py).
//
// A non-dynamics row r is an equality row (g_r = 0) or an inequality row (g_r <= 0), with a multiplier mu_r and a penalty rho_r.
// al_row follows Powell, Hestenes and Rockafellar:
//   !(rho >= 0), g != g or mu != mu      psi = mult = weight = NaN  (the FIRST comparison, `!(rho >= 0.0)`, is the one a NaN rho and a
//                                        negative rho both fail; a NaN g or mu is caught by `x != x` beside it)
//   rho == 0                             not penalised: psi = mu * g, mult = mu, weight = 0
//   s = mu + rho * g
//   equality row, or s > 0               active:    mult = s, weight = rho, psi = (mu + (0.5 * rho) * g) * g
//   inequality row and not s > 0         inactive:  mult = 0, weight = 0,   psi = -((mu * mu) / (2 * rho))      (s = NaN from an infinite
//                                        rho at g = 0 lands here on an inequality row)
//   viol = |g| on an equality row, max(0, g) on an inequality row (a NaN g stays a NaN)
// mult = psi'(g) and weight = psi''(g) wherever psi is twice differentiable.
//
// The pass over the rows r = 0 .. n - 1 (the non-dynamics rows of a handle, r + n_dyn in its numbering) gives mult and weight per row and
// eight scalars, AL_INFO:
//   [0] P = sum psi_r   [1] active rows   [2] max viol   [3] sum viol^2   [4] max |mult - mu|   [5] penalised rows (rho != 0)   [6], [7] 0
// The sums have k_feas_merit's order: lane l (0 .. 63) starts from a_l = 0 and adds over r = l, l + 64, .. < n ascending, the 64 lane
// values are combined by the halving tree, for off = 32, 16, 8, 4, 2, 1:  a_l = a_l + a_{l+off}  (l < off), and the sum is a_0.  With
// every rho_r = 0, sigma * f + P therefore has the bits of dto_feasible_merit.  The counts are integers held in doubles and the maxima
// are exact (al_max keeps a NaN once it has met one), so their order does not matter; they run through the same lanes and tree.
#pragma once

#include <cmath>
#include <cstdint>

#include "dto_newton_plan.h"

namespace dto {

enum { AL_P = 0, AL_ACTIVE = 1, AL_MAX_VIOL = 2, AL_SUM_VIOL2 = 3, AL_MAX_DMULT = 4, AL_PENALISED = 5, AL_INFO = 8 };

struct AlRow { double psi, mult, weight, viol; };

NWT_HD inline double al_nan() { return __builtin_nan(""); }

NWT_HD inline AlRow al_row(bool is_eq, double g, double mu, double rho) {
    if (!(rho >= 0.0) || g != g || mu != mu) return AlRow{al_nan(), al_nan(), al_nan(), g != g ? g : (is_eq ? fabs(g) : (g > 0.0 ? g : 0.0))};
    const double viol = is_eq ? fabs(g) : (g > 0.0 ? g : 0.0);
    if (rho == 0.0) return AlRow{newton_mul(mu, g), mu, 0.0, viol};
    const double s = newton_add(mu, newton_mul(rho, g));
    if (is_eq || s > 0.0) return AlRow{newton_mul(newton_add(mu, newton_mul(newton_mul(0.5, rho), g)), g), s, rho, viol};
    return AlRow{-newton_div(newton_mul(mu, mu), newton_mul(2.0, rho)), 0.0, 0.0, viol};
}

// a maximum that keeps a NaN: exact, and the same in any order
NWT_HD inline double al_max(double m, double a) { return (a > m || a != a) ? a : m; }

// what one lane carries through the pass
struct AlLane { double P, active, max_viol, sum_viol2, max_dmult, penalised; };

NWT_HD inline AlLane al_lane_zero() { return AlLane{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// lane a takes row R in (the rows of a lane ascending)
NWT_HD inline AlLane al_lane_add(AlLane a, const AlRow& R, double mu, double rho) {
    a.P = newton_add(a.P, R.psi);
    a.active = newton_add(a.active, R.weight != 0.0 ? 1.0 : 0.0);
    a.max_viol = al_max(a.max_viol, R.viol);
    a.sum_viol2 = newton_add(a.sum_viol2, newton_mul(R.viol, R.viol));
    a.max_dmult = al_max(a.max_dmult, fabs(newton_sub(R.mult, mu)));
    a.penalised = newton_add(a.penalised, rho != 0.0 ? 1.0 : 0.0);
    return a;
}

// one level of the halving tree: a_l = a_l (+) a_{l+off}
NWT_HD inline AlLane al_lane_merge(AlLane a, const AlLane& b) {
    a.P = newton_add(a.P, b.P);
    a.active = newton_add(a.active, b.active);
    a.max_viol = al_max(a.max_viol, b.max_viol);
    a.sum_viol2 = newton_add(a.sum_viol2, b.sum_viol2);
    a.max_dmult = al_max(a.max_dmult, b.max_dmult);
    a.penalised = newton_add(a.penalised, b.penalised);
    return a;
}

NWT_HD inline void al_info_store(const AlLane& a, double* info) {
    info[AL_P] = a.P; info[AL_ACTIVE] = a.active; info[AL_MAX_VIOL] = a.max_viol; info[AL_SUM_VIOL2] = a.sum_viol2;
    info[AL_MAX_DMULT] = a.max_dmult; info[AL_PENALISED] = a.penalised; info[6] = 0.0; info[7] = 0.0;
}

// ---- the whole pass on host arrays (the statement of the order; the device pass is this text with the tree as six shuffles) ------------
// n rows; is_eq [n] (non-zero: equality row), g [n], mu [n] or null (zeros), rho [n]; mult and weight [n] or null; info [AL_INFO].
inline void al_rows_pass(int64_t n, const unsigned char* is_eq, const double* g, const double* mu, const double* rho, double* mult,
                         double* weight, double* info) {
    AlLane a[NEWTON_LANES];
    for (int l = 0; l < NEWTON_LANES; ++l) {
        a[l] = al_lane_zero();
        for (int64_t r = l; r < n; r += NEWTON_LANES) {
            const double m = mu ? mu[r] : 0.0;
            const AlRow R = al_row(is_eq[r] != 0, g[r], m, rho[r]);
            if (mult) mult[r] = R.mult;
            if (weight) weight[r] = R.weight;
            a[l] = al_lane_add(a[l], R, m, rho[r]);
        }
    }
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) a[l] = al_lane_merge(a[l], a[l + off]);
    al_info_store(a[0], info);
}

}  // namespace dto
