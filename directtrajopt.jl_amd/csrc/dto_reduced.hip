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
//
// Option "reduced_input_store" (plan and the store's layout: dto_input_plan.h) replaces J v^ / k_red_rhs and J' w / k_red_finish by
// products with the kept input blocks F_a [K][2][Wf_a][x_dim_a] (a's rows of interval k in the columns of its free inputs fin_a at
// knot k, half 0, and knot k + 1, half 1):
//   k_red_input_gather      F_a out of the Jacobian value slab (jac_pos), as k_elim_gather copies the coupling blocks
//   k_red_input_forward     B [N][1][D], one thread per entry.  B_0[d] = the knot-0 state entry of v.  For k >= 1, a the owner of d and
//                           r = d - pre_a:  acc = 0;  for half = 0, 1: for j = 0 .. Wf_a - 1:
//                               acc = acc + F_a[k-1][half][j][r] * v[(k - 1 + half) z + fin_a[j]];      B_k[d] = -acc
//                           (every product and every sum rounded on its own).  No state entry of v past knot 0 is read.
//   k_red_input_transposed  y [n_vars].  Dependent entries 0; states of knot 0 Gam_0[d]; globals and unread components q - 0.0; a READ
//                           component c of knot kn:  y = q - t, one wavefront per output.  Lane l starts from p_l = 0 and visits c's
//                           terms (a, j) in plan order, per term interval kn - 1 through half 1 (where kn >= 1) and then interval kn
//                           through half 0 (where kn < K), per (term, interval iv) the rows r = l, l + 64, .. < x_dim_a ascending:
//                               p_l = p_l + F_a[iv][half][j][r] * Gam_{iv+1}[pre_a + r]
//                           Then the 64 partials are combined by a fixed halving tree, for off = 32, 16, 8, 4, 2, 1:
//                               p_l = p_l + p_{l+off}   (l < off),          t = p_0
//                           by wavefront shuffles: no LDS, no atomics.  The order is part of the contract.
//
// Block forms (dto_projected_hessian_products[_dev]): k_red_vhat_block, k_red_rhs_block, k_red_zhat_block, k_red_gather_block,
// k_red_multipliers_block, k_red_finish_block, k_red_input_forward_block and k_red_input_transposed_block do the same for w columns per
// launch, the vectors as planes [w][n] and the solves' arrays as [N][w][D].  Per column the operations and their order are those above,
// so column j of a block result has the bits of the single form on column j.
#include <algorithm>

#include "dto_elim_plan.h"
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

// The products and sums of the two input-block kernels, each rounded on its own.  (__dmul_rn and __dadd_rn are plain operators in the
// compiler's header and carry its leave to contract: a product feeding a sum through them becomes one fused multiply-add, which NumPy
// cannot restate.  Here contraction is switched off where the operators are written.)
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double sub_rn(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}

// grid: (K intervals, 2 halves); one launch per integrator with free inputs
__global__ void __launch_bounds__(256) k_red_input_gather(KProb P, KInput In, int a, const double* __restrict__ vals, double* __restrict__ store) {
    const KInputInt T = In.integ[a];
    const int64_t k = blockIdx.x;
    const int half = blockIdx.y;
    const int64_t kn = k + half;
    const int part = half == 0 ? 1 : 0;   // the column of knot k holds interval k as its part 1, that of knot k + 1 as its part 0
    const int total = T.wf * T.n;
    for (int e = threadIdx.x; e < total; e += blockDim.x) {
        const int j = e / T.n, r = e % T.n;
        store[T.store + elim_block_pos(T.wf, T.n, k, half, j) + r] = vals[jac_pos(P, P.colptr, kn, In.fin[T.fin0 + j], T.pre, T.n, part, r)];
    }
}

__global__ void __launch_bounds__(256) k_red_input_forward(KReduced R, KInput In, const double* __restrict__ store, const double* __restrict__ v,
                                                            double* __restrict__ B) {
    RED_LOOP(e, R.N * R.D) {
        const int64_t k = e / R.D;
        const int d = (int)(e % R.D);
        if (k == 0) {
            B[e] = v[reduced_pack_index(R, 0, d)];
            continue;
        }
        const KInputInt T = In.integ[In.pos_int[d]];
        const int r = d - T.pre;
        const int32_t* fin = In.fin + T.fin0;
        double acc = 0.0;
        for (int half = 0; half < 2; ++half) {
            const double* f = store + T.store + elim_block_pos(T.wf, T.n, k - 1, half, 0) + r;
            const double* vk = v + (k - 1 + half) * R.z;
            for (int j = 0; j < T.wf; ++j) acc = add_rn(acc, mul_rn(f[(size_t)j * T.n], vk[fin[j]]));
        }
        B[e] = -acc;
    }
}

// blocks [0, wave_blocks): four wavefronts each, one per (knot, read component); the blocks behind them: one thread per other entry
__global__ void __launch_bounds__(256) k_red_input_transposed(KReduced R, KInput In, unsigned wave_blocks, const double* __restrict__ store,
                                                               const double* __restrict__ q, const double* __restrict__ gam,
                                                               double* __restrict__ y) {
    if (blockIdx.x < wave_blocks) {
        const int64_t o = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;   // uniform in a wavefront
        if (o >= R.N * In.n_read) return;
        const int lane = threadIdx.x % 64;
        const int64_t kn = o / In.n_read;
        const int c = In.read[o % In.n_read];
        double p = 0.0;
        for (int t = In.term0[c]; t < In.term0[c + 1]; ++t) {
            const KInputTerm T = In.terms[t];
            for (int half = 1; half >= 0; --half) {
                const int64_t iv = half == 1 ? kn - 1 : kn;   // interval kn - 1 reaches knot kn through its half 1, interval kn through half 0
                if (iv < 0 || iv >= In.K) continue;
                const double* f = store + T.store + elim_block_pos(T.wf, T.n, iv, half, T.j);
                const double* g = gam + (iv + 1) * R.D + T.pre;
                for (int r = lane; r < T.n; r += 64) p = add_rn(p, mul_rn(f[r], g[r]));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) p = add_rn(p, __shfl_down(p, off, 64));
        if (lane == 0) y[kn * R.z + c] = sub_rn(q[kn * R.z + c], p);
        return;
    }
    const int64_t first = (int64_t)(blockIdx.x - wave_blocks) * blockDim.x + threadIdx.x, stride = (int64_t)(gridDim.x - wave_blocks) * blockDim.x;
    for (int64_t e = first; e < R.n_vars; e += stride) {
        const int d = reduced_state_pos(R, e);
        if (d >= 0) {
            y[e] = e < R.z ? gam[d] : 0.0;
            continue;
        }
        if (e < R.N * R.z) {
            const int c = (int)(e % R.z);
            if (In.term0[c + 1] > In.term0[c]) continue;   // a read component: its wavefront writes it
        }
        y[e] = sub_rn(q[e], 0.0);
    }
}

// ---- block forms: w columns per launch (dto_projected_hessian_products[_dev]).  Every Z-layout or row vector is kept as PLANES:
// column j of a vector of n entries at j * n (the caller's V and Y, and z^, q, v^, rho, w, t inside); the solves' layout: (k, j, d) at
// (k * w + j) * D + d.  Per column every kernel computes what its single form computes, with the same operations in the same order.

__global__ void __launch_bounds__(256) k_red_vhat_block(KReduced R, int w, const double* __restrict__ v, double* __restrict__ vh) {
    RED_LOOP(i, R.n_vars * w) {
        double x = 0.0;
        if (reduced_state_pos(R, i % R.n_vars) < 0) x = v[i];
        vh[i] = x;
    }
}

__global__ void __launch_bounds__(256) k_red_rhs_block(KReduced R, int w, const double* __restrict__ v, const double* __restrict__ rho,
                                                        double* __restrict__ B) {
    RED_LOOP(i, R.N * w * R.D) {
        const int d = (int)(i % R.D);
        const int64_t kj = i / R.D, k = kj / w, j = kj % w;
        B[i] = k == 0 ? v[j * R.n_vars + reduced_pack_index(R, 0, d)] : -rho[j * R.n_cons + reduced_dyn_row(R, k - 1, d)];
    }
}

__global__ void __launch_bounds__(256) k_red_zhat_block(KReduced R, int w, const double* __restrict__ v, const double* __restrict__ Y,
                                                         double* __restrict__ zh) {
    RED_LOOP(i, R.n_vars * w) {
        const int64_t j = i / R.n_vars, e = i % R.n_vars;
        const int d = reduced_state_pos(R, e);
        double x;
        if (d >= 0) x = Y[((e / R.z) * w + j) * R.D + d];
        else x = v[i];
        zh[i] = x;
    }
}

__global__ void __launch_bounds__(256) k_red_gather_block(KReduced R, int w, const double* __restrict__ q, double* __restrict__ qS) {
    RED_LOOP(i, R.N * w * R.D) {
        const int64_t kj = i / R.D;
        qS[i] = q[(kj % w) * R.n_vars + reduced_pack_index(R, kj / w, (int)(i % R.D))];
    }
}

// the row vectors of J' w: lam_{k+1} in the dynamics rows of interval k, 0 in every other row
__global__ void __launch_bounds__(256) k_red_multipliers_block(KReduced R, int w, const double* __restrict__ lam, double* __restrict__ wv) {
    const int64_t n_dyn = R.n_dyn;
    RED_LOOP(i, R.n_cons * w) {
        const int64_t j = i / R.n_cons, e = i % R.n_cons;
        if (e < n_dyn) {
            const int64_t k = e / R.D;
            const int d = (int)(e % R.D);
            wv[j * R.n_cons + reduced_dyn_row(R, k, d)] = lam[((k + 1) * w + j) * R.D + d];
        } else {
            wv[i] = 0.0;
        }
    }
}

__global__ void __launch_bounds__(256) k_red_finish_block(KReduced R, int w, const double* __restrict__ q, const double* __restrict__ t,
                                                           const double* __restrict__ lam, double* __restrict__ y) {
    RED_LOOP(i, R.n_vars * w) {
        const int64_t j = i / R.n_vars, e = i % R.n_vars;
        const int d = reduced_state_pos(R, e);
        double x = 0.0;
        if (d < 0) x = __dsub_rn(q[i], t[i]);
        else if (e < R.z) x = lam[j * R.D + d];
        y[i] = x;
    }
}

// one thread per (knot, column, d); per column k_red_input_forward's sum: half 0 then half 1, j ascending
__global__ void __launch_bounds__(256) k_red_input_forward_block(KReduced R, KInput In, int w, const double* __restrict__ store,
                                                                  const double* __restrict__ v, double* __restrict__ B) {
    RED_LOOP(i, R.N * w * R.D) {
        const int d = (int)(i % R.D);
        const int64_t kj = i / R.D, k = kj / w;
        const double* vc = v + (kj % w) * R.n_vars;
        if (k == 0) {
            B[i] = vc[reduced_pack_index(R, 0, d)];
            continue;
        }
        const KInputInt T = In.integ[In.pos_int[d]];
        const int r = d - T.pre;
        const int32_t* fin = In.fin + T.fin0;
        double acc = 0.0;
        for (int half = 0; half < 2; ++half) {
            const double* f = store + T.store + elim_block_pos(T.wf, T.n, k - 1, half, 0) + r;
            const double* vk = vc + (k - 1 + half) * R.z;
            for (int j = 0; j < T.wf; ++j) acc = add_rn(acc, mul_rn(f[(size_t)j * T.n], vk[fin[j]]));
        }
        B[i] = -acc;
    }
}

// grid (x, column tiles).  Blocks x < wave_blocks: four wavefronts each, one per (knot, read component), which load every F element
// once and update TC partial sums, one per column of the tile -- per column k_red_input_transposed's visit order and halving tree.  A
// tile that reaches past the last column computes that column again in its spare slots and stores nothing for them.  The blocks
// behind them (tile 0 only): one thread per other entry of every column.
template <int TC>
__global__ void __launch_bounds__(256) k_red_input_transposed_block(KReduced R, KInput In, int w, unsigned wave_blocks,
                                                                     const double* __restrict__ store, const double* __restrict__ q,
                                                                     const double* __restrict__ gam, double* __restrict__ y) {
    if (blockIdx.x < wave_blocks) {
        const int64_t o = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;   // uniform in a wavefront
        if (o >= R.N * In.n_read) return;
        const int lane = threadIdx.x % 64;
        const int j0 = (int)blockIdx.y * TC;
        const int64_t kn = o / In.n_read;
        const int c = In.read[o % In.n_read];
        double p[TC];
        int64_t goff[TC];
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            p[j] = 0.0;
            goff[j] = (int64_t)(j0 + j < w ? j0 + j : w - 1) * R.D;
        }
        for (int t = In.term0[c]; t < In.term0[c + 1]; ++t) {
            const KInputTerm T = In.terms[t];
            for (int half = 1; half >= 0; --half) {
                const int64_t iv = half == 1 ? kn - 1 : kn;
                if (iv < 0 || iv >= In.K) continue;
                const double* f = store + T.store + elim_block_pos(T.wf, T.n, iv, half, T.j);
                const double* g = gam + (iv + 1) * w * R.D + T.pre;
                for (int r = lane; r < T.n; r += 64) {
                    const double fr = f[r];
#pragma unroll
                    for (int j = 0; j < TC; ++j) p[j] = add_rn(p[j], mul_rn(fr, g[goff[j] + r]));
                }
            }
        }
#pragma unroll
        for (int j = 0; j < TC; ++j) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) p[j] = add_rn(p[j], __shfl_down(p[j], off, 64));
        }
        if (lane == 0) {
            const int64_t e = kn * R.z + c;
#pragma unroll
            for (int j = 0; j < TC; ++j)
                if (j0 + j < w) y[(int64_t)(j0 + j) * R.n_vars + e] = sub_rn(q[(int64_t)(j0 + j) * R.n_vars + e], p[j]);
        }
        return;
    }
    if (blockIdx.y != 0) return;
    const int64_t first = (int64_t)(blockIdx.x - wave_blocks) * blockDim.x + threadIdx.x, stride = (int64_t)(gridDim.x - wave_blocks) * blockDim.x;
    for (int64_t i = first; i < R.n_vars * w; i += stride) {
        const int64_t j = i / R.n_vars, e = i % R.n_vars;
        const int d = reduced_state_pos(R, e);
        if (d >= 0) {
            y[i] = e < R.z ? gam[j * R.D + d] : 0.0;
            continue;
        }
        if (e < R.N * R.z) {
            const int c = (int)(e % R.z);
            if (In.term0[c + 1] > In.term0[c]) continue;   // a read component: its wavefront writes it
        }
        y[i] = sub_rn(q[i], 0.0);
    }
}

unsigned red_grid(int64_t total) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 4096)); }

}  // namespace

void launch_red_input_gather(hipStream_t st, const KProb& P, const KInput& In, int a, const double* vals, double* store) {
    hipLaunchKernelGGL(k_red_input_gather, dim3((unsigned)In.K, 2), dim3(256), 0, st, P, In, a, vals, store);
}
void launch_red_input_forward(hipStream_t st, const KReduced& R, const KInput& In, const double* store, const double* v, double* B) {
    hipLaunchKernelGGL(k_red_input_forward, dim3(red_grid(R.N * R.D)), dim3(256), 0, st, R, In, store, v, B);
}
void launch_red_input_transposed(hipStream_t st, const KReduced& R, const KInput& In, const double* store, const double* q, const double* gam,
                                 double* y) {
    const unsigned wave_blocks = (unsigned)((R.N * In.n_read + 3) / 4);
    hipLaunchKernelGGL(k_red_input_transposed, dim3(wave_blocks + red_grid(R.n_vars)), dim3(256), 0, st, R, In, wave_blocks, store, q, gam, y);
}

void launch_red_input_forward_block(hipStream_t st, const KReduced& R, const KInput& In, int w, const double* store, const double* v, double* B) {
    hipLaunchKernelGGL(k_red_input_forward_block, dim3(red_grid(R.N * w * R.D)), dim3(256), 0, st, R, In, w, store, v, B);
}
void launch_red_input_transposed_block(hipStream_t st, const KReduced& R, const KInput& In, int w, const double* store, const double* q,
                                       const double* gam, double* y) {
    const unsigned wave_blocks = (unsigned)((R.N * In.n_read + 3) / 4);
    const int T = hess_block_tile(w);   // the same tiles as the block H product: 1, 2, 4 or 8 columns
    const dim3 grid(wave_blocks + red_grid(R.n_vars * w), (unsigned)((w + T - 1) / T));
    if (T == 8) hipLaunchKernelGGL(k_red_input_transposed_block<8>, grid, dim3(256), 0, st, R, In, w, wave_blocks, store, q, gam, y);
    else if (T == 4) hipLaunchKernelGGL(k_red_input_transposed_block<4>, grid, dim3(256), 0, st, R, In, w, wave_blocks, store, q, gam, y);
    else if (T == 2) hipLaunchKernelGGL(k_red_input_transposed_block<2>, grid, dim3(256), 0, st, R, In, w, wave_blocks, store, q, gam, y);
    else hipLaunchKernelGGL(k_red_input_transposed_block<1>, grid, dim3(256), 0, st, R, In, w, wave_blocks, store, q, gam, y);
}
void launch_red_vhat_block(hipStream_t st, const KReduced& R, int w, const double* v, double* vh) {
    hipLaunchKernelGGL(k_red_vhat_block, dim3(red_grid(R.n_vars * w)), dim3(256), 0, st, R, w, v, vh);
}
void launch_red_rhs_block(hipStream_t st, const KReduced& R, int w, const double* v, const double* rho, double* B) {
    hipLaunchKernelGGL(k_red_rhs_block, dim3(red_grid(R.N * w * R.D)), dim3(256), 0, st, R, w, v, rho, B);
}
void launch_red_zhat_block(hipStream_t st, const KReduced& R, int w, const double* v, const double* Y, double* zh) {
    hipLaunchKernelGGL(k_red_zhat_block, dim3(red_grid(R.n_vars * w)), dim3(256), 0, st, R, w, v, Y, zh);
}
void launch_red_gather_block(hipStream_t st, const KReduced& R, int w, const double* q, double* qS) {
    hipLaunchKernelGGL(k_red_gather_block, dim3(red_grid(R.N * w * R.D)), dim3(256), 0, st, R, w, q, qS);
}
void launch_red_multipliers_block(hipStream_t st, const KReduced& R, int w, const double* lam, double* wv) {
    hipLaunchKernelGGL(k_red_multipliers_block, dim3(red_grid(R.n_cons * w)), dim3(256), 0, st, R, w, lam, wv);
}
void launch_red_finish_block(hipStream_t st, const KReduced& R, int w, const double* q, const double* t, const double* lam, double* y) {
    hipLaunchKernelGGL(k_red_finish_block, dim3(red_grid(R.n_vars * w)), dim3(256), 0, st, R, w, q, t, lam, y);
}

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
