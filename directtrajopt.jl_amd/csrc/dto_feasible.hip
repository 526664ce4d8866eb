// dto_feasible.hip -- kernels of the feasible-trajectory rollout and the reduced merit value (dto_feasible_trajectory /
// dto_feasible_merit and their _dev forms; schedule: dto_feasible_plan.h).  The routine is a composition of the engine's own pieces --
// the Jacobian, the rollout's product tree and descent, the objective and the constraints -- and what is here moves states into the
// Z layout [N][z] without leaving the device and sums the merit value.
//
//   k_feas_deriv    a DerivativeIntegrator's recurrence written into Zf: one thread per component r adds, serial in the knots,
//                       x = Zf[x_off + r];  for k = 0 .. K - 1:  x = x + Zf[k z + dt] * Zf[k z + xdot_off + r];  Zf[(k + 1) z + x_off + r] = x
//                   the product and the sum rounded on their own: NumPy's  x[k] + dt[k] * xdot[k],  bit for bit.  dt and xdot are read
//                   from Zf, where lower levels have already written them (an integrator whose inputs meet its own states is refused).
//                   The increments dt_k * xdot_k[r] of a chunk of knots are formed by the whole workgroup in LDS before thread r adds.
//   k_feas_scatter  knots 1 .. K of column 0 of the rollout's padded trajectory S [K + 1][col_pad][npad] into the integrator's state
//                   components of Zf.  Knot 0 is what the descent started from and stays.
//   k_feas_merit    phi = sigma f + sum over the non-dynamics rows r of mu_r g_r, by ONE wavefront in a fixed order: lane l starts from
//                   p_l = 0 and adds mu_r g_r over r = n_dyn + l, n_dyn + l + 64, .. < n_cons ascending; the 64 partials are combined by
//                   the halving tree of k_red_input_transposed, for off = 32, 16, 8, 4, 2, 1:  p_l = p_l + p_{l+off}  (l < off),  t = p_0;
//                   phi = sigma * f + t.  Without mu:  phi = sigma * f.  Every product and every sum rounded on its own.  Wavefront
//                   shuffles: no LDS, no atomics.  The dynamics-row entries of mu are never read.
// One writer per entry, plain 8-byte loads and stores; LDS in k_feas_deriv alone (the increments of a chunk of knots).
#include <algorithm>

#include "dto_kernels.h"

namespace dto {

namespace {

// each rounded on its own (see dto_reduced.hip: __dmul_rn / __dadd_rn carry the compiler's leave to contract, these do not)
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

// One workgroup per FEAS_COMPS components, FEAS_THREADS threads.  The recurrence is serial in the knots, but its inputs are not: per
// chunk of knots ALL threads load dt and xdot and form the increments dt_k * xdot_k[r] in LDS (many loads in flight: one memory latency
// per chunk, not per knot), thread r then adds its column in the order of the knots, replacing each increment by the state, and all
// threads store the states.  A chunk holds FEAS_ELEMS / (components of the workgroup) knots.
// `in` and `out` are two views of the ONE buffer Zf: what is read (dt, xdot, the state of knot 0) is never written here -- the
// integrator's inputs do not meet its own states, and the stores start at knot 1.
constexpr int FEAS_COMPS = 64, FEAS_THREADS = 256, FEAS_ELEMS = 4096;

__global__ void __launch_bounds__(FEAS_THREADS) k_feas_deriv(int64_t K, int z, int dt_idx, int x_off, int xdot_off, int d,
                                                              const double* __restrict__ in, double* __restrict__ out) {
    __shared__ double buf[FEAS_ELEMS];
    const int r0 = blockIdx.x * FEAS_COMPS, tid = threadIdx.x;
    const int dl = min(d - r0, FEAS_COMPS);   // components of this workgroup, >= 1 by the grid
    const int C = FEAS_ELEMS / dl;            // knots per chunk, >= 64
    double x = tid < dl ? in[x_off + r0 + tid] : 0.0;
    for (int64_t k0 = 0; k0 < K; k0 += C) {
        const int c = (int)min((int64_t)C, K - k0), total = c * dl;
        for (int e = tid; e < total; e += FEAS_THREADS) {
            const double* zk = in + (size_t)(k0 + e / dl) * z;
            buf[e] = mul_rn(zk[dt_idx], zk[xdot_off + r0 + e % dl]);
        }
        __syncthreads();
        if (tid < dl) {
            for (int j = 0; j < c; j += 8) {   // eight increments are read before the first sum needs one
                double inc[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) inc[t] = j + t < c ? buf[(j + t) * dl + tid] : 0.0;
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (j + t < c) {
                        x = add_rn(x, inc[t]);
                        buf[(j + t) * dl + tid] = x;
                    }
            }
        }
        __syncthreads();
        for (int e = tid; e < total; e += FEAS_THREADS) out[(size_t)(k0 + e / dl + 1) * z + x_off + r0 + e % dl] = buf[e];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_feas_scatter(KRollout R, int z, const double* __restrict__ S, double* __restrict__ Zf) {
    const int64_t total = R.K * R.n;
    const size_t blk = (size_t)R.col_pad * R.npad;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = 1 + e / R.n;
        const int r = (int)(e % R.n);
        Zf[(size_t)k * z + R.x_off + r] = S[(size_t)k * blk + r];
    }
}

__global__ void __launch_bounds__(64) k_feas_merit(int64_t n_dyn, int64_t n_cons, double sigma, const double* __restrict__ f,
                                                    const double* __restrict__ mu, const double* __restrict__ g, double* __restrict__ phi) {
    const int lane = threadIdx.x;
    double p = 0.0;
    if (mu)
        for (int64_t r = n_dyn + lane; r < n_cons; r += 64) p = add_rn(p, mul_rn(mu[r], g[r]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = add_rn(p, __shfl_down(p, off, 64));
    if (lane == 0) {
        const double sf = mul_rn(sigma, f[0]);
        phi[0] = mu ? add_rn(sf, p) : sf;
    }
}

}  // namespace

void launch_feas_deriv(hipStream_t st, int64_t K, int z, int dt_idx, const KDer& D, double* Zf) {
    hipLaunchKernelGGL(k_feas_deriv, dim3((unsigned)((D.d + FEAS_COMPS - 1) / FEAS_COMPS)), dim3(FEAS_THREADS), 0, st, K, z, dt_idx, D.x_off, D.xdot_off, D.d, Zf, Zf);
}

void launch_feas_scatter(hipStream_t st, const KRollout& R, int z, const double* S, double* Zf) {
    const int64_t total = R.K * R.n;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(k_feas_scatter, dim3(grid), dim3(256), 0, st, R, z, S, Zf);
}

void launch_feas_merit(hipStream_t st, int64_t n_dyn, int64_t n_cons, double sigma, const double* f, const double* mu, const double* g,
                       double* phi) {
    hipLaunchKernelGGL(k_feas_merit, dim3(1), dim3(64), 0, st, n_dyn, n_cons, sigma, f, mu, g, phi);
}

}  // namespace dto
