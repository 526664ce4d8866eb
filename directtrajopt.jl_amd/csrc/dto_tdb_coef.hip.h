// dto_tdb_coef.hip.h -- the scalar jet coefficients of the TimeDependentBilinearIntegrator's generator family, shared by the
// kernels that apply jets as combinations of B_q y (dto_tdb_mfma.hip, dto_tdb_kron.hip) and by the product modes of dto_tdb.hip.
#pragma once

#include "dto_kernels.h"
#include "dto_tdb_scheme.h"

namespace dto {

// Scalar coefficient of B_q in one jet of M(tau) = dt sum_j a_j(tau) (G_j + sum_c phi_c(t) H_cj), t = t_k + tau dt -- the one table
// of all three kernels.  which: 0 value; 1 + b first derivative; 1 + p + tdb_pair_rank(a, b) second derivative (a <= b).
__device__ inline double tdbm_coef(const KTdb& T, const double* zk, const double* zk1, double tk, double dt, double tau, int p, int which, int q) {
    const int m = T.m, nmod = T.nmod;
    const int j = q / (1 + nmod), c = q - j * (1 + nmod);
    int b1 = -1, b2 = -1;
    if (which >= 1 && which <= p) b1 = which - 1;
    else if (which > p) tdb_pair_unrank(which - 1 - p, p, &b1, &b2);
    // a_j and its derivative slots: wk = d a_j / d u_kj, wk1 = d a_j / d u_{k+1,j}
    double aj = 1.0, wk = 0.0, wk1 = 0.0;
    if (j >= 1) {
        const double uk = zk[T.u_off + j - 1];
        if (T.order) { const double uk1 = zk1[T.u_off + j - 1]; aj = (1.0 - tau) * uk + tau * uk1; wk = 1.0 - tau; wk1 = tau; }
        else { aj = uk; wk = 1.0; }
    }
    double ph = 1.0, ph1 = 0.0, ph2 = 0.0;
    if (c >= 1) {
        const double om = T.mod_omega[c - 1], arg = om * (tk + tau * dt);
        const double cs = cos(arg), sn = sin(arg);
        if (T.mod_kind[c - 1] == 1) { ph = cs; ph1 = -om * sn; ph2 = -om * om * cs; }
        else { ph = sn; ph1 = om * cs; ph2 = -om * om * sn; }
    }
    // parameter classes: 0 = u_k (drive jj), 1 = t, 2 = dt, 3 = u_{k+1} (drive jj)
    auto cls = [&](int b, int& jj) { if (b < m) { jj = b + 1; return 0; } if (b == m) { jj = -1; return 1; }
                                     if (b == m + 1) { jj = -1; return 2; } jj = b - m - 1; return 3; };
    if (which == 0) return dt * aj * ph;
    if (b2 < 0) {
        int jj; const int k1 = cls(b1, jj);
        if (k1 == 0) return jj == j ? dt * wk * ph : 0.0;
        if (k1 == 3) return jj == j ? dt * wk1 * ph : 0.0;
        if (k1 == 1) return dt * aj * ph1;
        return aj * ph + dt * aj * tau * ph1;
    }
    int j1, j2; const int k1 = cls(b1, j1), k2 = cls(b2, j2);
    const bool u1 = k1 == 0 || k1 == 3, u2 = k2 == 0 || k2 == 3;
    if (u1 && u2) return 0.0;
    if (u1 || u2) {
        const int ju = u1 ? j1 : j2, ku = u1 ? k1 : k2, ko = u1 ? k2 : k1;
        const double w = ku == 0 ? wk : wk1;
        if (ju != j) return 0.0;
        return ko == 1 ? dt * w * ph1 : w * (ph + dt * tau * ph1);
    }
    if (k1 == 1 && k2 == 1) return dt * aj * ph2;
    if (k1 == 2 && k2 == 2) return 2.0 * aj * tau * ph1 + dt * aj * tau * tau * ph2;
    return aj * ph1 + dt * aj * tau * ph2;   // (t, dt)
}

// Entry of the stacked pair [z_k ; z_{k+1}] that parameter b of theta = [u_k (m), t_k, dt_k, u_{k+1} (m, order 1)] lives in: where a
// J w mode reads its component of w (relative to knot k) and where a J' w mode lands its term.  Two parameters may name one entry
// (the timestep listed as the time variable).
__host__ __device__ inline int tdb_param_entry(const KTdb& T, int z, int dt_idx, int b) {
    return b < T.m ? T.u_off + b : (b == T.m ? T.t_off : (b == T.m + 1 ? dt_idx : z + T.u_off + (b - T.m - 2)));
}

// Directional coefficient row of J w: M_w = sum_b w_theta_b M_b = sum_q c_wq B_q with c_wq = sum_b w_theta_b c_{1+b, q}, b ascending.
// `table` holds rows 0 .. p of tdbm_coef at the stage time ([which][Q]); the product modes keep the result in row 1 + p.
__device__ inline double tdbm_dir_coef(const double* table, int Q, int p, int q, const double* w_theta) {
    double s = 0.0;
    for (int b = 0; b < p; ++b) s += w_theta[b] * table[(size_t)(1 + b) * Q + q];
    return s;
}

}  // namespace dto
