// dto_rollout.hip -- kernels of the open-loop rollout X_{k+1} = E_k X_k (dto_rollout / dto_rollout_dev; index plan: dto_rollout_plan.h).
//
//   k_rollout_leaves   gathers one integrator's -E_k blocks out of the Jacobian value slab, negated, into the zero-padded npad x npad
//                      leaves of the product tree (slot rev_L(k)); the leaves past K are the identity.  Addressed like k_share_E:
//                      a wavefront per column, the column's run located once with jac_pos, 8-byte loads (a run starts at any
//                      multiple of 8 bytes), contiguous stores.
//   k_rollout_start    writes the zero-padded X0 into knot 0 of the padded trajectory S [K + 1][col_pad][npad].
//   k_rollout_descend  one level of the descent: S[mid] = node * S[start] for every live item of the level, an npad x npad by
//                      npad x col_pad product on v_mfma_f64_16x16x4_f64 (the 8-byte core of dto_gemm.hip.h).  A workgroup owns a
//                      64 x TN tile of one item's output and runs the whole K range itself: every entry has one writer and is
//                      summed in ascending k, four k per MFMA step, whatever the grid, the column count or the column tile (16 or 64)
//                      -- a column has the same bits alone and among others.
//   k_rollout_compact  copies knots of S into the caller's layout [knot][n_cols][n].
// Plain loads and stores only: nothing is accumulated across workgroups.
#include <algorithm>

#include "dto_gemm.hip.h"
#include "dto_kernels.h"
#include "dto_rollout_plan.h"

namespace dto {

namespace {

__global__ void __launch_bounds__(256) k_rollout_leaves(KProb P, KRollout R, const double* __restrict__ vals, double* __restrict__ tree) {
    const int64_t slot = blockIdx.x;
    const int64_t kn = rollout_rev(R.L, slot);   // (bit reversal is its own inverse)
    const int n = R.n, npad = R.npad;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* leaf = tree + (size_t)slot * npad * npad;
    for (int col = 4 * blockIdx.y + wave; col < npad; col += 4 * gridDim.y) {
        double* dst = leaf + (size_t)col * npad;
        if (kn < R.K && col < n) {
            const double* src = vals + jac_pos(P, P.colptr, kn, R.x_off + col, R.pre, n, 1, 0);
            for (int r = lane; r < npad; r += 64) dst[r] = r < n ? -src[r] : 0.0;
        } else {
            const double diag = kn < R.K ? 0.0 : 1.0;
            for (int r = lane; r < npad; r += 64) dst[r] = r == col ? diag : 0.0;
        }
    }
}

// X0: [n_cols][n] (column-major n x n_cols), or null: the integrator's state components of knot 0 of Z (one column)
__global__ void __launch_bounds__(256) k_rollout_start(KRollout R, const double* __restrict__ dZ, const double* __restrict__ X0,
                                                        double* __restrict__ S) {
    const int64_t total = (int64_t)R.col_pad * R.npad;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e / R.npad), r = (int)(e % R.npad);
        double v = 0.0;
        if (c < R.n_cols && r < R.n) v = X0 ? X0[(size_t)c * R.n + r] : dZ[R.x_off + r];
        S[e] = v;
    }
}

template <class Shape>
__global__ void __launch_bounds__(Shape::THREADS) k_rollout_descend(KRollout R, int l, int64_t only, const double* __restrict__ tree,
                                                                    double* __restrict__ S) {
    __shared__ double smem[Shape::SMEM_DOUBLES];
    const RolloutItem it = rollout_item(R.L, R.K, l, only >= 0 ? only : (int64_t)blockIdx.x);
    if (!it.live) return;   // (the same for every thread of the workgroup)
    const int npad = R.npad;
    const size_t blk = (size_t)R.col_pad * npad;
    const int row0 = 64 * blockIdx.y, col0 = Shape::TN * blockIdx.z;
    GemmAccS<Shape> acc;
    acc.zero();
    gemm_accumulate_s<Shape>(acc, tree + (size_t)it.node * npad * npad + row0, npad, S + (size_t)it.start * blk + (size_t)col0 * npad, npad,
                             npad, nullptr, smem);
    const GemmCoordS<Shape> co;
    double* out = S + (size_t)it.mid * blk + (size_t)col0 * npad + row0;
#pragma unroll
    for (int ti = 0; ti < Shape::MT; ++ti)
#pragma unroll
        for (int tj = 0; tj < Shape::NT; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(co.col_base + 16 * tj + 4 * r) * npad + co.row_base + 16 * ti] = acc.v[ti][tj][r];
}

// knots k0 .. k0 + nk - 1 of S into X [nk][n_cols][n]
__global__ void __launch_bounds__(256) k_rollout_compact(KRollout R, int64_t k0, int64_t nk, const double* __restrict__ S, double* __restrict__ X) {
    const int64_t per = (int64_t)R.n_cols * R.n, total = nk * per;
    const size_t blk = (size_t)R.col_pad * R.npad;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / per;
        const int rem = (int)(e % per), c = rem / R.n, r = rem % R.n;
        X[e] = S[(size_t)(k0 + k) * blk + (size_t)c * R.npad + r];
    }
}

unsigned flat_grid(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 4096); }

}  // namespace

void launch_rollout_leaves(hipStream_t st, const KProb& P, const KRollout& R, const double* vals, double* tree) {
    const int gy = R.npad >= 256 ? 16 : (R.npad + 15) / 16;   // at least four columns per wavefront
    hipLaunchKernelGGL(k_rollout_leaves, dim3((unsigned)((int64_t)1 << R.L), (unsigned)gy), dim3(P.debug_bad_launch ? 4096 : 256), 0, st, P, R,
                       vals, tree);
}

void launch_rollout_start(hipStream_t st, const KRollout& R, const double* dZ, const double* X0, double* S) {
    hipLaunchKernelGGL(k_rollout_start, dim3(flat_grid((int64_t)R.col_pad * R.npad)), dim3(256), 0, st, R, dZ, X0, S);
}

void launch_rollout_descend(hipStream_t st, const KRollout& R, int l, int64_t only, const double* tree, double* S) {
    const unsigned items = only >= 0 ? 1u : (unsigned)rollout_items(R.L, l);
    const int tn = rollout_col_tile(R.n_cols);
    const dim3 grid(items, (unsigned)(R.npad / 64), (unsigned)(R.col_pad / tn));
    if (tn == 16) {
        using Sh = GemmShape<64, 16, 2, 1, 16>;
        hipLaunchKernelGGL((k_rollout_descend<Sh>), grid, dim3(Sh::THREADS), 0, st, R, l, only, tree, S);
    } else {
        using Sh = GemmShape<64, 64, 2, 2, 16>;
        hipLaunchKernelGGL((k_rollout_descend<Sh>), grid, dim3(Sh::THREADS), 0, st, R, l, only, tree, S);
    }
}

void launch_rollout_compact(hipStream_t st, const KRollout& R, int64_t k0, int64_t nk, const double* S, double* X) {
    hipLaunchKernelGGL(k_rollout_compact, dim3(flat_grid(nk * R.n_cols * R.n)), dim3(256), 0, st, R, k0, nk, S, X);
}

}  // namespace dto
