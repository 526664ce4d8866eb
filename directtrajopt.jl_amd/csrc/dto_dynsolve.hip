// dto_dynsolve.hip -- kernels of the solves with the dynamics block (dto_dynamics_solve / dto_dynamics_solve_dev): the linearised
// rollout Y_{k+1} = E_k Y_k + B_{k+1} and the costate recursion Lam_k = E_k' Lam_{k+1} + B_k as affine scans over the rollout's
// product tree (index plan: dto_rollout_plan.h; the tree itself is built by dto_rollout.hip's gather and the batched products).
//
//   k_dynsolve_load    scatters the caller's B [N][n_cols][n] into the zero-padded level-0 blocks of the offset tree (slot rev_L(i) of
//                      leaf i) and into the one knot of the padded trajectory S [K + 1][col_pad][npad] the descent starts from.
//   k_dynsolve_affine  out = op(A) X + addend, A an npad x npad node of the matrix tree, X and addend [col_pad][npad] blocks, op the
//                      identity (forward) or the transpose (adjoint), on v_mfma_f64_16x16x4_f64 through the 8-byte core of
//                      dto_gemm.hip.h.  One kernel, four launch kinds: the up-sweep of a level (out, X, addend in the offset tree) and
//                      a level of the descent (X, out knots of S, addend the node's offset), in either direction.  Grid and column
//                      tiles are k_rollout_descend's: a workgroup owns a 64 x TN tile of one item's output and runs the whole K range
//                      itself, so every entry has one writer and is summed in ascending k, four k per MFMA step, whatever the grid,
//                      the column count or the column tile.  The addend is added to the FINISHED sum: with B = [X0; 0; ...] the
//                      forward solve therefore gives dto_rollout's bits.
// The caller's layout is written by k_rollout_compact.  Plain loads and stores only: nothing is accumulated across workgroups.
#include <algorithm>

#include "dto_gemm.hip.h"
#include "dto_kernels.h"
#include "dto_rollout_plan.h"

namespace dto {

namespace {

// grid: (2^L leaves + 1 for the trajectory's knot, chunks of a block)
__global__ void __launch_bounds__(256) k_dynsolve_load(KRollout R, int adjoint, const double* __restrict__ B, double* __restrict__ off,
                                                        double* __restrict__ S) {
    const int64_t leaves = (int64_t)1 << R.L;
    const size_t blk = (size_t)R.col_pad * R.npad;
    int64_t from;
    double* dst;
    if ((int64_t)blockIdx.x < leaves) {
        from = dynsolve_leaf_knot(R.K, adjoint, blockIdx.x);
        dst = off + (size_t)(rollout_level_off(R.L, 0) + rollout_leaf_slot(R.L, blockIdx.x)) * blk;
    } else {
        const DynsolveStart s = dynsolve_start(R.L, R.K, adjoint);
        if (s.knot < 0) return;   // (the same for every thread of the workgroup)
        from = s.from;
        dst = S + (size_t)s.knot * blk;
    }
    const double* src = from >= 0 ? B + (size_t)from * R.n_cols * R.n : nullptr;
    for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < (int)blk; e += gridDim.y * blockDim.x) {
        const int c = e / R.npad, r = e % R.npad;
        dst[e] = src && c < R.n_cols && r < R.n ? src[(size_t)c * R.n + r] : 0.0;
    }
}

// kind 0: the up-sweep of level l into level l + 1 (blockIdx.x = slot of the parent); kind 1: level l of the descent (blockIdx.x =
// item, or the item `only`)
template <class Shape, bool TRANS>
__global__ void __launch_bounds__(Shape::THREADS) k_dynsolve_affine(KRollout R, int kind, int l, int64_t only, const double* __restrict__ tree,
                                                                    double* __restrict__ off, double* __restrict__ S) {
    __shared__ double smem[Shape::SMEM_DOUBLES];
    const int npad = R.npad;
    const size_t blk = (size_t)R.col_pad * npad, nn = (size_t)npad * npad;
    const double *A, *X, *add;
    double* out;
    bool x_zero = false;
    if (kind == 0) {
        const DynsolveUp u = dynsolve_up(R.L, TRANS, l, blockIdx.x);
        A = tree + (size_t)u.a * nn;
        X = off + (size_t)u.x * blk;
        add = off + (size_t)u.add * blk;
        out = off + (size_t)u.out * blk;
    } else {
        const DynsolveItem it = dynsolve_item(R.L, R.K, TRANS, l, only >= 0 ? only : (int64_t)blockIdx.x);
        if (!it.live) return;   // (the same for every thread of the workgroup)
        A = tree + (size_t)it.node * nn;
        X = S + (size_t)it.src * blk;
        add = off + (size_t)it.node * blk;
        out = S + (size_t)it.dst * blk;
        x_zero = it.src_zero;
    }
    const int row0 = 64 * blockIdx.y, col0 = Shape::TN * blockIdx.z;
    const size_t tile = (size_t)col0 * npad + row0;
    const GemmCoordS<Shape> co;
    GemmAccS<Shape> acc;
    acc.zero();
    if (!x_zero) {   // (workgroup-uniform; a knot beyond K is zero and is never read)
        if constexpr (TRANS) gemm_accumulate_st<Shape>(acc, A + (size_t)row0 * npad, npad, X + (size_t)col0 * npad, npad, npad, smem);
        else gemm_accumulate_s<Shape>(acc, A + row0, npad, X + (size_t)col0 * npad, npad, npad, nullptr, smem);
    }
#pragma unroll
    for (int ti = 0; ti < Shape::MT; ++ti)
#pragma unroll
        for (int tj = 0; tj < Shape::NT; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t e = tile + (size_t)(co.col_base + 16 * tj + 4 * r) * npad + co.row_base + 16 * ti;
                out[e] = acc.v[ti][tj][r] + add[e];
            }
}

template <bool TRANS>
void launch_affine(hipStream_t st, const KRollout& R, int kind, int l, int64_t only, unsigned items, const double* tree, double* off, double* S) {
    const int tn = rollout_col_tile(R.n_cols);
    const dim3 grid(items, (unsigned)(R.npad / 64), (unsigned)(R.col_pad / tn));
    if (tn == 16) {
        using Sh = GemmShape<64, 16, 2, 1, 16>;
        hipLaunchKernelGGL((k_dynsolve_affine<Sh, TRANS>), grid, dim3(Sh::THREADS), 0, st, R, kind, l, only, tree, off, S);
    } else {
        using Sh = GemmShape<64, 64, 2, 2, 16>;
        hipLaunchKernelGGL((k_dynsolve_affine<Sh, TRANS>), grid, dim3(Sh::THREADS), 0, st, R, kind, l, only, tree, off, S);
    }
}

}  // namespace

void launch_dynsolve_load(hipStream_t st, const KRollout& R, int adjoint, const double* B, double* off, double* S) {
    const int64_t blk = (int64_t)R.col_pad * R.npad;
    hipLaunchKernelGGL(k_dynsolve_load, dim3((unsigned)(((int64_t)1 << R.L) + 1), (unsigned)std::min<int64_t>((blk + 255) / 256, 16)), dim3(256), 0,
                       st, R, adjoint, B, off, S);
}

void launch_dynsolve_up(hipStream_t st, const KRollout& R, int adjoint, int l, const double* tree, double* off) {
    const unsigned items = (unsigned)rollout_level_len(R.L, l + 1);
    if (adjoint) launch_affine<true>(st, R, 0, l, -1, items, tree, off, nullptr);
    else launch_affine<false>(st, R, 0, l, -1, items, tree, off, nullptr);
}

void launch_dynsolve_descend(hipStream_t st, const KRollout& R, int adjoint, int l, int64_t only, const double* tree, double* off, double* S) {
    const unsigned items = only >= 0 ? 1u : (unsigned)rollout_items(R.L, l);
    if (adjoint) launch_affine<true>(st, R, 1, l, only, items, tree, off, S);
    else launch_affine<false>(st, R, 1, l, only, items, tree, off, S);
}

}  // namespace dto
