// dto_hess_product.hip -- y = H v from a compact symmetric copy of the Hessian-of-Lagrangian slab
// (dto_eval_hessian_product[_dev], MOI.eval_hessian_lagrangian_product).
//
// The engine assembles H once per point into a private slab (do_hessian), gathers the entries that can be non-zero into a
// row-major list of BOTH triangles (k_hess_gather), and every product at that point is one memory-bound launch
// (k_hess_spmv).  The index (row starts and lengths, 32-bit columns, slab positions) is built once per handle on the host
// (dto_engine.cpp, build_hp_index); every row starts at an even entry, so a lane reads two values and two columns per
// 16-byte / 8-byte load.  The row-length mix is very uneven (x rows ~ m + 2 entries, u and dt rows ~ n + m, dense blocks of
// host-evaluated integrators up to 3z), so rows are sorted into classes that give a row G = 4, 16 or 64 lanes.  Summation
// order: lane l adds the pairs l, l + G, l + 2G, ... of its row in order, then a fixed xor butterfly over the G lanes --
// a function of the row's class alone, never of the launch or of the call.  No atomics: every y[r] has one writer.
// k_hess_spmm is the same product for a block of columns (dto_eval_hessian_products[_dev], dto_projected_hessian_products[_dev]):
// the matrix is read once per tile of columns, and every column keeps k_hess_spmv's summation order and so its bits.
#include "dto_kernels.h"

namespace dto {
namespace {

// val[i] = slab[pos[i]]; pos = -1 marks the padding slot behind an odd-length row (written as 0)
__global__ void __launch_bounds__(256) k_hess_gather(const double* __restrict__ slab, const int64_t* __restrict__ pos, int64_t n,
                                                     double* __restrict__ val) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const int64_t p = pos[i];
        val[i] = p >= 0 ? slab[p] : 0.0;
    }
}

template <int G>
__device__ __forceinline__ void hess_row(const KHessProduct& p, int64_t i, bool valid, const double* __restrict__ v,
                                         double* __restrict__ y) {
    const int lane = threadIdx.x & (G - 1);
    double acc = 0.0;
    int32_t r = 0;
    if (valid) {
        r = p.rows[i];
        const int64_t s = p.start[r], e = s + p.len[r];  // s even: 16-byte aligned pairs
        for (int64_t k = s + 2 * lane; k < e; k += 2 * G) {
            const double2 a = *reinterpret_cast<const double2*>(p.val + k);
            const int2 c = *reinterpret_cast<const int2*>(p.col + k);
            acc += a.x * v[c.x];
            if (k + 1 < e) acc += a.y * v[c.y];
        }
    }
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (valid && lane == 0) y[r] = acc;
}

// one launch for every class: blocks [blk0[c], blk0[c+1]) serve the rows rows[row0[c] .. row0[c+1]) with cls_g[c] lanes each
__global__ void __launch_bounds__(256) k_hess_spmv(KHessProduct p, const double* __restrict__ v, double* __restrict__ y) {
    const int64_t b = blockIdx.x;
    int c = 0;
    while (c + 1 < p.n_cls && b >= p.blk0[c + 1]) ++c;
    const int g = p.cls_g[c];
    const int64_t i = p.row0[c] + (b - p.blk0[c]) * (256 / g) + threadIdx.x / g;
    const bool valid = i < p.row0[c + 1];
    if (g == 4) hess_row<4>(p, i, valid, v, y);
    else if (g == 16) hess_row<16>(p, i, valid, v, y);
    else hess_row<64>(p, i, valid, v, y);
}

// Block form: T columns of V per lane.  A lane loads its value pair and its column pair once and updates T accumulators (a
// compile-time tile: the loop is unrolled and acc stays in registers).  Per column the sums are hess_row's: the pairs l, l + G, ..
// in order, then the same butterfly, so column j of Y has the bits of k_hess_spmv on column j of V.  Entry (i, j) of V sits at
// v[i * B.v_es + j * B.v_cs], of Y at y[i * B.y_es + j * B.y_cs].  A tile that reaches past the last column computes that column
// again in its spare slots and stores nothing for them.
template <int G, int T>
__device__ __forceinline__ void hess_row_block(const KHessProduct& p, const KHessBlock& B, int j0, int64_t i, bool valid,
                                               const double* __restrict__ v, double* __restrict__ y) {
    const int lane = threadIdx.x & (G - 1);
    double acc[T];
    int64_t voff[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        acc[j] = 0.0;
        voff[j] = (int64_t)(j0 + j < B.w ? j0 + j : B.w - 1) * B.v_cs;
    }
    int32_t r = 0;
    if (valid) {
        r = p.rows[i];
        const int64_t s = p.start[r], e = s + p.len[r];  // s even: 16-byte aligned pairs
        for (int64_t k = s + 2 * lane; k < e; k += 2 * G) {
            const double2 a = *reinterpret_cast<const double2*>(p.val + k);
            const int2 c = *reinterpret_cast<const int2*>(p.col + k);
            const double* vx = v + (int64_t)c.x * B.v_es;
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] += a.x * vx[voff[j]];
            if (k + 1 < e) {
                const double* vy = v + (int64_t)c.y * B.v_es;
#pragma unroll
                for (int j = 0; j < T; ++j) acc[j] += a.y * vy[voff[j]];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
        for (int off = G >> 1; off > 0; off >>= 1) acc[j] += __shfl_xor(acc[j], off, 64);
    }
    if (valid && lane == 0) {
#pragma unroll
        for (int j = 0; j < T; ++j)
            if (j0 + j < B.w) y[(int64_t)r * B.y_es + (int64_t)(j0 + j) * B.y_cs] = acc[j];
    }
}

// grid: (k_hess_spmv's blocks, column tiles)
template <int T>
__global__ void __launch_bounds__(256) k_hess_spmm(KHessProduct p, KHessBlock B, const double* __restrict__ v, double* __restrict__ y) {
    const int64_t b = blockIdx.x;
    const int j0 = (int)blockIdx.y * T;
    int c = 0;
    while (c + 1 < p.n_cls && b >= p.blk0[c + 1]) ++c;
    const int g = p.cls_g[c];
    const int64_t i = p.row0[c] + (b - p.blk0[c]) * (256 / g) + threadIdx.x / g;
    const bool valid = i < p.row0[c + 1];
    if (g == 4) hess_row_block<4, T>(p, B, j0, i, valid, v, y);
    else if (g == 16) hess_row_block<16, T>(p, B, j0, i, valid, v, y);
    else hess_row_block<64, T>(p, B, j0, i, valid, v, y);
}

}  // namespace

void launch_hess_spmm(hipStream_t st, const KHessProduct& p, const KHessBlock& B, const double* v, double* y) {
    const int64_t blocks = p.blk0[p.n_cls];
    if (blocks <= 0 || B.w < 1) return;
    const int T = hess_block_tile(B.w);
    const dim3 grid((unsigned)blocks, (unsigned)((B.w + T - 1) / T));
    if (T == 8) hipLaunchKernelGGL(k_hess_spmm<8>, grid, dim3(256), 0, st, p, B, v, y);
    else if (T == 4) hipLaunchKernelGGL(k_hess_spmm<4>, grid, dim3(256), 0, st, p, B, v, y);
    else if (T == 2) hipLaunchKernelGGL(k_hess_spmm<2>, grid, dim3(256), 0, st, p, B, v, y);
    else hipLaunchKernelGGL(k_hess_spmm<1>, grid, dim3(256), 0, st, p, B, v, y);
}

void launch_hess_gather(hipStream_t st, const double* slab, const int64_t* pos, int64_t n, double* val) {
    if (n <= 0) return;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_hess_gather, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, slab, pos, n, val);
}

void launch_hess_spmv(hipStream_t st, const KHessProduct& p, const double* v, double* y) {
    const int64_t blocks = p.blk0[p.n_cls];
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_hess_spmv, dim3((unsigned)blocks), dim3(256), 0, st, p, v, y);
}

}  // namespace dto
