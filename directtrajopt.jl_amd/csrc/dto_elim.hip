// dto_elim.hip -- kernels of the whole-dynamics solves (dto_dynamics_solve_all / dto_dynamics_solve_all_dev; plan: dto_elim_plan.h):
// block elimination over ALL integrators' rows and state columns.  The block solves of bilinear and time-dependent integrators are
// dto_dynsolve.hip's affine scans over a product tree per integrator; what is here moves data between them.
//
//   k_elim_gather      copies the coupling blocks C_a of one (integrator, dependency) pair out of the Jacobian value slab (jac_pos) into
//                      the compact store [K][2][W_a][x_dim_a]: a's rows of interval k in the columns of S_b at knot k and knot k + 1.
//   k_elim_couple      forms the right-hand side of integrator a's own block solve, Bp [N][n_cols][x_dim_a], one thread per entry:
//                        forward   Bp_0 = B_0,  Bp_{k+1} = B_{k+1} - C_{a,k} [Y^deps_k ; Y^deps_{k+1}]
//                                  (half 0 before half 1, dependencies in list order, columns ascending)
//                        adjoint   Bp_k = B_k - sum over the dependents b of a, in list order, of
//                                  C_b[k-1][half 1][col]' Lam^b_k  then  C_b[k][half 0][col]' Lam^b_{k+1}   (rows ascending):
//                                  a reduction down one contiguous column run of the store per term.
//                      The sum is finished before it is subtracted; every entry has one writer and one order, whatever n_cols is.
//   k_deriv_scan       the block solve of a DerivativeIntegrator (E_k = I): the serial recurrence Y_{k+1} = Y_k + Bp_{k+1}, or
//                      Lam_k = Lam_{k+1} + Bp_k, one thread per (column, row), written straight into the result's slice.
//   k_elim_collect     copies a block solve's result [N][n_cols][x_dim_a] into its slice of the result [N][n_cols][D].
// Plain loads and stores only: no atomics, nothing is accumulated across threads.
#include <algorithm>

#include "dto_elim_plan.h"
#include "dto_kernels.h"

namespace dto {

namespace {

// grid: (K intervals, 2 halves)
__global__ void __launch_bounds__(256) k_elim_gather(KProb P, KElimPair G, const double* __restrict__ vals, double* __restrict__ store) {
    const int64_t k = blockIdx.x;
    const int half = blockIdx.y;
    const int64_t kn = k + half;
    const int part = half == 0 ? 1 : 0;   // the column of knot k holds interval k as its part 1, that of knot k + 1 as its part 0
    const int total = G.n_b * G.n_a;
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const int j = e / G.n_a, r = e % G.n_a;
        store[elim_block_pos(G.width, G.n_a, k, half, G.col + j) + r] = vals[jac_pos(P, P.colptr, kn, G.x_off_b + j, G.pre_a, G.n_a, part, r)];
    }
}

template <bool ADJOINT>
__global__ void __launch_bounds__(256) k_elim_couple(KElimCouple C, const double* __restrict__ store, const double* __restrict__ B,
                                                      const double* __restrict__ Y, double* __restrict__ Bp) {
    const int64_t per = (int64_t)C.n_cols * C.n_a, total = (C.K + 1) * per;
    const size_t knot = (size_t)C.n_cols * C.D;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / per;
        const int rem = (int)(e % per), c = rem / C.n_a, r = rem % C.n_a;
        const size_t at = (size_t)k * knot + (size_t)c * C.D;
        double acc = 0.0;
        if (!ADJOINT) {
            if (k >= 1) {
                for (int half = 0; half < 2; ++half)
                    for (int t = 0; t < C.n_terms; ++t) {
                        const KElimTerm T = C.terms[t];
                        const double* cb = store + T.store + elim_block_pos(T.width, T.n_rows, k - 1, half, T.col) + r;
                        const double* y = Y + (size_t)(k - 1 + half) * knot + (size_t)c * C.D + T.off;
                        for (int j = 0; j < T.n; ++j) acc += cb[(size_t)j * T.n_rows] * y[j];
                    }
            }
        } else {
            for (int t = 0; t < C.n_terms; ++t) {
                const KElimTerm T = C.terms[t];
                for (int half = 1; half >= 0; --half) {
                    const int64_t iv = half == 1 ? k - 1 : k;   // interval k - 1 reaches knot k through its half 1, interval k through half 0
                    if (iv < 0 || iv >= C.K) continue;
                    const double* cb = store + T.store + elim_block_pos(T.width, T.n_rows, iv, half, T.col + r);
                    const double* y = Y + (size_t)(iv + 1) * knot + (size_t)c * C.D + T.off;
                    for (int j = 0; j < T.n; ++j) acc += cb[j] * y[j];
                }
            }
        }
        Bp[e] = B[at + C.pre_a + r] - acc;
    }
}

// one thread per (column, row); Bp [N][n_cols][n], Y [N][n_cols][D]
__global__ void __launch_bounds__(64) k_deriv_scan(int64_t K, int n, int n_cols, int D, int pre, int adjoint, const double* __restrict__ Bp,
                                                    double* __restrict__ Y) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int per = n_cols * n;
    if (e >= per) return;
    const int c = e / n, r = e % n;
    const size_t knot = (size_t)n_cols * D, at = (size_t)c * D + pre + r;
    if (!adjoint) {
        double y = Bp[e];
        Y[at] = y;
#pragma unroll 8
        for (int64_t k = 1; k <= K; ++k) {
            y = y + Bp[(size_t)k * per + e];
            Y[(size_t)k * knot + at] = y;
        }
    } else {
        double y = Bp[(size_t)K * per + e];
        Y[(size_t)K * knot + at] = y;
#pragma unroll 8
        for (int64_t k = K - 1; k >= 0; --k) {
            y = y + Bp[(size_t)k * per + e];
            Y[(size_t)k * knot + at] = y;
        }
    }
}

__global__ void __launch_bounds__(256) k_elim_collect(int64_t N, int n, int n_cols, int D, int pre, const double* __restrict__ Yp,
                                                       double* __restrict__ Y) {
    const int64_t per = (int64_t)n_cols * n, total = N * per;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / per;
        const int rem = (int)(e % per), c = rem / n, r = rem % n;
        Y[((size_t)k * n_cols + c) * D + pre + r] = Yp[e];
    }
}

unsigned flat_grid(int64_t total) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 4096)); }

}  // namespace

void launch_elim_gather(hipStream_t st, const KProb& P, const KElimPair& G, int64_t K, const double* vals, double* store) {
    hipLaunchKernelGGL(k_elim_gather, dim3((unsigned)K, 2), dim3(256), 0, st, P, G, vals, store);
}

void launch_elim_couple(hipStream_t st, const KElimCouple& C, int adjoint, const double* store, const double* B, const double* Y, double* Bp) {
    const unsigned grid = flat_grid((C.K + 1) * C.n_cols * C.n_a);
    if (adjoint) hipLaunchKernelGGL(k_elim_couple<true>, dim3(grid), dim3(256), 0, st, C, store, B, Y, Bp);
    else hipLaunchKernelGGL(k_elim_couple<false>, dim3(grid), dim3(256), 0, st, C, store, B, Y, Bp);
}

void launch_deriv_scan(hipStream_t st, int64_t K, int n, int n_cols, int D, int pre, int adjoint, const double* Bp, double* Y) {
    hipLaunchKernelGGL(k_deriv_scan, dim3((unsigned)((n_cols * n + 63) / 64)), dim3(64), 0, st, K, n, n_cols, D, pre, adjoint, Bp, Y);
}

void launch_elim_collect(hipStream_t st, int64_t N, int n, int n_cols, int D, int pre, const double* Yp, double* Y) {
    hipLaunchKernelGGL(k_elim_collect, dim3(flat_grid(N * n_cols * n)), dim3(256), 0, st, N, n, n_cols, D, pre, Yp, Y);
}

}  // namespace dto
