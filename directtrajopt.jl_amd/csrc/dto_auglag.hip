// dto_auglag.hip -- kernels of the augmented-Lagrangian terms of the reduced-space stack (dto_auglag_rows / _merit / _gradient /
// _hessian_products / _newton_step and their _dev forms; the row rules and the order of the sums: dto_auglag_plan.h; include/dto_engine.h,
// "Augmented-Lagrangian terms").
//
//   k_al_rows    the row pass.  Workgroup 0 is ONE wavefront over the non-dynamics rows: lane l takes r = n_dyn + l, + 64, .. ascending,
//                calls al_row, writes mult and weight of its rows and carries the six sums / maxima of dto_auglag_plan.h, which the
//                halving tree (six shuffles) combines; lane 0 writes the eight scalars and, for the merit, phi = sigma * f + P.  The
//                other workgroups write the zeros of the dynamics rows of mu_eff and weight.  No LDS, no atomics.
//   k_al_gn      the Gauss-Newton term of one constraint of kind ||v|| - c or ||v||^2 - c whose `times` and `comps` repeat nothing, for
//                all w columns in ONE launch: one thread per (column, listing, component).  It forms its row's c = (J z^)_row in
//                k_jv_knot's component order (pattern entries only), scales it by the row's weight and adds jac * (weight * c) to its
//                entry of t -- the entry's only writer in this launch -- as k_jtv_knot does.  The row's gradient is recomputed from Z.
//   k_al_scale   c_r = weight_r * c_r on the rows of one constraint (the constraints that go through the single-column launchers)
//   k_al_add     q = q + t over the w planes, one rounded addition per entry
// The products and sums of k_al_gn are written as the fused multiply-adds the product kernels (k_jv_knot, k_jtv_knot, knot_norm2) run,
// so the bits are those of dto_eval_jacobian_product / dto_eval_jacobian_transpose_product around the scaling.
#include <algorithm>

#include "dto_auglag_plan.h"
#include "dto_kernels.h"

namespace dto {

namespace {

__device__ __forceinline__ AlLane al_shfl_down(const AlLane& a, int off) {
    return AlLane{__shfl_down(a.P, off, 64),         __shfl_down(a.active, off, 64),    __shfl_down(a.max_viol, off, 64),
                  __shfl_down(a.sum_viol2, off, 64), __shfl_down(a.max_dmult, off, 64), __shfl_down(a.penalised, off, 64)};
}

__global__ void __launch_bounds__(64) k_al_rows(KAlRows A) {
    const int lane = threadIdx.x;
    if (blockIdx.x > 0) {   // the dynamics rows hold no multiplier of a penalty term and no weight
        for (int64_t r = (int64_t)(blockIdx.x - 1) * 64 + lane; r < A.n_dyn; r += (int64_t)(gridDim.x - 1) * 64) {
            if (A.mu_eff) A.mu_eff[r] = 0.0;
            if (A.weight) A.weight[r] = 0.0;
        }
        return;
    }
    AlLane a = al_lane_zero();
    for (int64_t r = A.n_dyn + lane; r < A.n_cons; r += 64) {
        const double m = A.mu ? A.mu[r] : 0.0;
        const double rho = A.rho ? A.rho[r] : 0.0;
        const AlRow R = al_row(A.is_eq[r - A.n_dyn] != 0, A.g[r], m, rho);
        if (A.mu_eff) A.mu_eff[r] = R.mult;
        if (A.weight) A.weight[r] = R.weight;
        a = al_lane_add(a, R, m, rho);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = al_lane_merge(a, al_shfl_down(a, off));
    if (lane == 0) {
        if (A.info) al_info_store(a, A.info);
        if (A.phi) A.phi[0] = newton_add(newton_mul(A.sigma, A.f[0]), a.P);
    }
}

// ||v||^2 of a listing in knot_norm2's order
__device__ __forceinline__ double al_norm2(const KCon& C, const double* zk) {
    double s = 0.0;
    for (int c = 0; c < C.n_comps; ++c) {
        const double v = zk[C.comps[c]];
        s = fma(v, v, s);
    }
    return s;
}

__global__ void __launch_bounds__(256) k_al_gn(KProb P, KCon C, int w, int64_t n_vars, const double* __restrict__ Z,
                                               const double* __restrict__ weight, const double* __restrict__ zh, double* __restrict__ t) {
    const int64_t per = C.n_times * C.n_comps;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= per * w) return;
    const int64_t j = e / per, i = e - j * per;
    if (C.jpos[i] < 0) return;
    const int64_t ti = i / C.n_comps;
    const int c_own = (int)(i - ti * C.n_comps);
    const int64_t kn = C.times[ti];
    const double* zk = Z + kn * P.z;
    const double* zj = zh + (size_t)j * n_vars + kn * P.z;
    const double nrm = C.kind == 1 ? sqrt(al_norm2(C, zk)) : 1.0;
    // c = (J z^)_row: k_jv_knot's sum, then its one addition onto the zeroed row
    double s = 0.0;
    for (int c = 0; c < C.n_comps; ++c) {
        if (C.jpos[ti * C.n_comps + c] < 0) continue;
        const double v = zk[C.comps[c]];
        s = fma(C.kind == 1 ? v / nrm : 2.0 * v, zj[C.comps[c]], s);
    }
    const double row = newton_add(0.0, s);
    const double wc = newton_mul(weight[C.mu_off + C.tidx[ti]], row);
    // t += jac * (weight c): k_jtv_knot's one addition onto the entry
    const double v = zk[C.comps[c_own]];
    const double jac = C.kind == 1 ? v / nrm : 2.0 * v;
    double* out = t + (size_t)j * n_vars + kn * P.z + C.comps[c_own];
    *out = fma(jac, wc, *out);
}

__global__ void __launch_bounds__(256) k_al_scale(int64_t n, const double* __restrict__ weight, double* __restrict__ c) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) c[r] = newton_mul(weight[r], c[r]);
}

__global__ void __launch_bounds__(256) k_al_add(int64_t n, const double* __restrict__ t, double* __restrict__ q) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) q[i] = newton_add(q[i], t[i]);
}

}  // namespace

void launch_al_rows(hipStream_t st, const KAlRows& A) {
    const unsigned zero_groups = (unsigned)std::max<int64_t>(1, std::min<int64_t>((A.n_dyn + 63) / 64, 1024));
    hipLaunchKernelGGL(k_al_rows, dim3(1 + ((A.mu_eff || A.weight) && A.n_dyn > 0 ? zero_groups : 0)), dim3(64), 0, st, A);
}

void launch_al_gn(hipStream_t st, const KProb& P, const KCon& C, int w, int64_t n_vars, const double* dZ, const double* weight, const double* zh,
                  double* t) {
    const int64_t n = C.n_times * C.n_comps * w;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_al_gn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, C, w, n_vars, dZ, weight, zh, t);
}

void launch_al_scale(hipStream_t st, int64_t n, const double* weight, double* c) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_al_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, weight, c);
}

void launch_al_add(hipStream_t st, int64_t n, const double* t, double* q) {
    if (n <= 0) return;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(k_al_add, dim3(grid), dim3(256), 0, st, n, t, q);
}

}  // namespace dto
