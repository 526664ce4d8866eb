// dto_reduced.hip -- kernels of the reduced-space operators (dto_reduced_gradient / dto_reduced_hessian_product and their _dev forms;
// index plan: dto_reduced_plan.h).  The operators are compositions of the engine's own routines -- the objective gradient, J w, J' w,
// the whole-dynamics solves, H v -- and what is here moves vectors between their layouts without leaving the device: the Z layout
// (n_vars), the constraint rows (n_cons) and the solves' [N][1][D].
//
//   k_red_gradient     g = sigma * grad f (+ t), and its state entries packed into [N][1][D]
//   k_red_multipliers  a row vector w and (optionally) the multipliers mu~ from mu and a costate array Lam [N][D]:
//                        dynamics row of interval k at position d:  w = Lam_{k+1}[d] (0 without Lam),  mu~ = -Lam_{k+1}[d]
//                        any other row:                             w = mu or 0,                       mu~ = mu (0 without mu)
//   k_red_vhat         v with the state entries of every knot set to zero
//   k_red_rhs          B [N][1][D]: knot 0 from the state entries of v, knot k + 1 from -rho in the dynamics rows of interval k
//   k_red_zhat         v with the state entries of every knot replaced by Y [N][1][D]
//   k_red_gather       the state entries of a Z-layout vector as [N][1][D]
//   k_red_finish       q - t on the free entries, Lam_0 on the states of knot 0, 0 on the dependent entries
// One thread per output entry, one writer per entry, plain 8-byte loads and stores, no atomics, no LDS.  The arithmetic is a negation,
// __dmul_rn, __dadd_rn and __dsub_rn -- each rounded on its own, never contracted -- so the results are those of the same expressions
// in NumPy, bit for bit.  Entries a kernel does not need are not read: a NaN in a dependent entry of v reaches nothing.
#include <algorithm>

#include "dto_kernels.h"
#include "dto_reduced_plan.h"

namespace dto {

namespace {

#define RED_LOOP(e, total) \
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < (total); e += (int64_t)gridDim.x * blockDim.x)

__global__ void __launch_bounds__(256) k_red_gradient(KReduced R, double sigma, const double* __restrict__ gf, const double* __restrict__ t,
                                                       double* __restrict__ g, double* __restrict__ gS) {
    RED_LOOP(e, R.n_vars) {
        double x = __dmul_rn(sigma, gf[e]);
        if (t) x = __dadd_rn(x, t[e]);
        g[e] = x;
        if (reduced_state_pos(R, e) >= 0) gS[reduced_unpack_index(R, e)] = x;
    }
}

__global__ void __launch_bounds__(256) k_red_multipliers(KReduced R, const double* __restrict__ lam, const double* __restrict__ mu,
                                                          int w_takes_mu, double* __restrict__ w, double* __restrict__ mut) {
    const int64_t n_dyn = R.n_dyn;   // = (N - 1) D, rows [0, n_dyn): checked by the host routine
    RED_LOOP(e, R.n_cons) {
        if (e < n_dyn) {
            const int64_t k = e / R.D;
            const int d = (int)(e % R.D);
            const int64_t row = reduced_dyn_row(R, k, d);
            const double l = lam ? lam[(k + 1) * R.D + d] : 0.0;
            w[row] = l;
            if (mut) mut[row] = -l;
        } else {
            const double m = mu ? mu[e] : 0.0;
            w[e] = w_takes_mu ? m : 0.0;
            if (mut) mut[e] = m;
        }
    }
}

__global__ void __launch_bounds__(256) k_red_vhat(KReduced R, const double* __restrict__ v, double* __restrict__ vh) {
    RED_LOOP(e, R.n_vars) {
        double x = 0.0;
        if (reduced_state_pos(R, e) < 0) x = v[e];
        vh[e] = x;
    }
}

__global__ void __launch_bounds__(256) k_red_rhs(KReduced R, const double* __restrict__ v, const double* __restrict__ rho,
                                                  double* __restrict__ B) {
    RED_LOOP(e, R.N * R.D) {
        const int64_t k = e / R.D;
        const int d = (int)(e % R.D);
        B[e] = k == 0 ? v[reduced_pack_index(R, 0, d)] : -rho[reduced_dyn_row(R, k - 1, d)];
    }
}

__global__ void __launch_bounds__(256) k_red_zhat(KReduced R, const double* __restrict__ v, const double* __restrict__ Y,
                                                   double* __restrict__ zh) {
    RED_LOOP(e, R.n_vars) {
        double x;
        if (reduced_state_pos(R, e) >= 0) x = Y[reduced_unpack_index(R, e)];
        else x = v[e];
        zh[e] = x;
    }
}

__global__ void __launch_bounds__(256) k_red_gather(KReduced R, const double* __restrict__ q, double* __restrict__ qS) {
    RED_LOOP(e, R.N * R.D) qS[e] = q[reduced_pack_index(R, e / R.D, (int)(e % R.D))];
}

__global__ void __launch_bounds__(256) k_red_finish(KReduced R, const double* __restrict__ q, const double* __restrict__ t,
                                                     const double* __restrict__ lam, double* __restrict__ y) {
    RED_LOOP(e, R.n_vars) {
        const int d = reduced_state_pos(R, e);
        double x = 0.0;
        if (d < 0) x = __dsub_rn(q[e], t[e]);
        else if (e < R.z) x = lam[d];
        y[e] = x;
    }
}

unsigned red_grid(int64_t total) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 4096)); }

}  // namespace

void launch_red_gradient(hipStream_t st, const KReduced& R, double sigma, const double* gf, const double* t, double* g, double* gS) {
    hipLaunchKernelGGL(k_red_gradient, dim3(red_grid(R.n_vars)), dim3(256), 0, st, R, sigma, gf, t, g, gS);
}
void launch_red_multipliers(hipStream_t st, const KReduced& R, const double* lam, const double* mu, int w_takes_mu, double* w, double* mut) {
    hipLaunchKernelGGL(k_red_multipliers, dim3(red_grid(R.n_cons)), dim3(256), 0, st, R, lam, mu, w_takes_mu, w, mut);
}
void launch_red_vhat(hipStream_t st, const KReduced& R, const double* v, double* vh) {
    hipLaunchKernelGGL(k_red_vhat, dim3(red_grid(R.n_vars)), dim3(256), 0, st, R, v, vh);
}
void launch_red_rhs(hipStream_t st, const KReduced& R, const double* v, const double* rho, double* B) {
    hipLaunchKernelGGL(k_red_rhs, dim3(red_grid(R.N * R.D)), dim3(256), 0, st, R, v, rho, B);
}
void launch_red_zhat(hipStream_t st, const KReduced& R, const double* v, const double* Y, double* zh) {
    hipLaunchKernelGGL(k_red_zhat, dim3(red_grid(R.n_vars)), dim3(256), 0, st, R, v, Y, zh);
}
void launch_red_gather(hipStream_t st, const KReduced& R, const double* q, double* qS) {
    hipLaunchKernelGGL(k_red_gather, dim3(red_grid(R.N * R.D)), dim3(256), 0, st, R, q, qS);
}
void launch_red_finish(hipStream_t st, const KReduced& R, const double* q, const double* t, const double* lam, double* y) {
    hipLaunchKernelGGL(k_red_finish, dim3(red_grid(R.n_vars)), dim3(256), 0, st, R, q, t, lam, y);
}

}  // namespace dto
