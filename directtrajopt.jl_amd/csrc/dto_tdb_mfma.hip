// dto_tdb_mfma.hip -- device propagator of the TimeDependentBilinearIntegrator for 65..256 states, on v_mfma_f64_16x16x4_f64.
//
// Same mathematics, ABI family and output blocks as k_tdb (dto_tdb.hip, which keeps 1..64 states): classical RK4 with `substeps`
// fixed steps on tau in [0, 1] applied to the state together with its variational equations, parameters
// theta = [u_k (m), t_k, dt_k, u_{k+1} (m, order 1)], the (x, theta) block of the Hessian of mu' f by the discrete adjoint.  What
// differs is the organisation, because at these sizes k_tdb's per-interval slab of materialised jets (1 + p + p (p+1) / 2 matrices
// of n x n) does not fit and its scalar matrix-vector loops do not scale:
//
//   * NO MATERIALISED JETS.  Every jet of M = dt G(u(tau), t) is a scalar combination of the Q = (m+1)(1+nmod) shared matrices B_q
//     (G_j, H_cj; the engine keeps zero-padded copies B_q and B_q' of np x np, np = n rounded up to 32).  Only
//     M0 = sum_q c_q B_q is formed as a matrix, once per stage time (three per sub-step, the last is the next one's first).  A
//     derivative jet is applied as M_b y = sum_q c_bq (B_q y): U_q = B_q y is computed once per stage for the stage's few vectors
//     (x alone in a Jacobian call; x and x_b in a Hessian call; kbar_0 in the adjoint) and combined with scalars in the epilogue of
//     the M0 product.
//   * ONE WORKGROUP-LEVEL GEMM.  All M0 / B_q products with 32 columns or more go through gemm_accumulate_s (dto_gemm.hip.h:
//     LDS-staged K panels, 2 x 2 wavefronts) on TM x 64 tiles, TM x 32 for a last half tile; TM = 64 where np is a multiple of 64,
//     else 32.  Columns of one call, each of np rows (column-major, leading dimension np):
//         defect    x | zeros to 32
//         Jacobian  x, x_b (p) | zeros to 32 | Phi (np columns, starts as the identity)       -- the Phi block carries the flops
//         Hessian   x, x_b (p), x_ab (p (p+1) / 2) | zeros to a multiple of 32                 -- no Phi, no Phi_b
//     The single-vector U_q of Jacobian calls and of the adjoint is a vector pass (one thread per (q, row), B_q read once).
//   * PERSISTENT GRID.  `resident` workgroups walk the intervals (interval i of the launch goes to workgroup i mod resident); the
//     scratch is one slot per workgroup, so it is sized by the grid and not by the number of intervals.
//
//   * GROUPS.  Integrators of one system (DTO_FLAG_SHARED_GENERATORS) go through k_tdb_mfma_group further down: the same scheme with
//     the members' vector blocks side by side and everything that does not depend on the ket formed once.
//
// Numerical rules: what a workgroup computes is a function of its interval's data alone (not of the grid, the shard or the slot);
// every sum has a fixed order; there is no floating-point atomic.  Output entries that share a position (a component that serves
// twice, e.g. the timestep listed as the time variable) are added by one thread in a fixed order.  Padded rows and columns are
// computed (they are zeros) and never written to vals / jac / hess.
//
// Product modes (the PROD instantiation of the same kernel; need 3: J w, need 4: J' w; formulas in dto_tdb.hip).  The column block is
// one 32-column tile and there is no Phi block:
//         J w       x, d | zeros to 32          d' = M0 d + M_w x: the Jacobian call's epilogue with ONE jet, the directional row
//         J' w      x, x_b (p) | zeros to 32    the Jacobian call's vector block; then p dot products with w_k
// M0 is formed for the forward tile as in the value calls.  The adjoint of J' w is a single column, so it forms no M0 and runs no
// GEMM: ubar = M0' kbar = sum_q c_q (B_q' kbar) from the vector pass that the Hessian's adjoint already has.  Results go to y (J w:
// the integrator's rows, one writer per entry) or to the per-interval staging of n + p doubles that k_tdb_jtv_place adds into y.
#include <algorithm>

#include "dto_gemm.hip.h"
#include "dto_kernels.h"
#include "dto_tdb_coef.hip.h"

namespace dto {

namespace {

constexpr int TDBM_VEC = 32;          // column tile of the vector block
constexpr int TDBM_MAX_PAIRS = 160;   // p (p+1) / 2 <= 136 at 7 drives, order 1

inline __host__ __device__ int pad32(int v) { return (v + 31) / 32 * 32; }

// scratch of one resident workgroup (doubles): four column sets, M0, the U_q vectors, ubar of the adjoint, the coefficient table
struct TdbmLayout {
    int np, p, P2, Q, C, Cv, Ctot, ucols;
    size_t oY, oACC, oTA, oTB, oM0, oU, oUB, oCoef, total;
};
inline __host__ __device__ TdbmLayout tdbm_layout(const KTdb& T, int need) {
    TdbmLayout L;
    L.np = pad32(T.n);
    L.p = tdb_num_params(T.m, T.order);
    L.P2 = tdb_num_pairs(L.p);
    L.Q = tdb_num_shared(T.m, T.nmod);
    // meaningful columns of the vector block (need 3: x, d; need 4: x, x_b)
    L.C = need == 0 ? 1 : (need == 3 ? 2 : (need == 1 || need == 4 ? 1 + L.p : 1 + L.p + L.P2));
    L.Cv = pad32(L.C);
    L.Ctot = L.Cv + (need == 1 ? L.np : 0);
    L.ucols = need == 2 ? TDBM_VEC : 1;
    const size_t cols = (size_t)L.np * L.Ctot;
    L.oY = 0; L.oACC = cols; L.oTA = 2 * cols; L.oTB = 3 * cols;
    L.oM0 = 4 * cols;
    L.oU = L.oM0 + (size_t)L.np * L.np;
    L.oUB = L.oU + (size_t)L.Q * L.ucols * L.np;
    L.oCoef = L.oUB + (size_t)L.np * TDBM_VEC;
    L.total = L.oCoef + (size_t)(1 + L.p + L.P2) * L.Q;
    L.total = (L.total + 1) & ~(size_t)1;
    return L;
}

struct TdbmArgs {
    KProb P;
    KTdb T;
    const double* Bp;    // [Q][np][np] zero-padded B_q, column-major; q = j (1 + nmod) + c, c = 0: G_j, c >= 1: H_{c-1, j}
    const double* BpT;   // their transposes
    const double* Z;
    const double* mu;
    int need;
    int64_t i_lo, count;
    double* vals;        // [K][n]
    double* jac;         // [K][2z][n]
    double* hess;        // [K][2z][2z]
    double* scratch;
    int64_t scratch_stride;
    const double* w;     // product modes: the vector
    double* out;         // need 3: y (the integrator's rows are assigned); need 4: staging [K][n + p]
};

// One TM x TN tile of A (np x np, column-major) times columns c0 .. of B; epi(row, col, value) for every element of the tile.
// All threads of the workgroup call it (the core ends with a barrier).
template <class S, class Epi>
__device__ __forceinline__ void mm_tile(const double* __restrict__ A, const double* __restrict__ B, int np, int r0, int c0,
                                        double* smem, Epi&& epi) {
    GemmAccS<S> acc;
    acc.zero();
    gemm_accumulate_s<S>(acc, A + r0, np, B + (size_t)c0 * np, np, np, nullptr, smem);
    const GemmCoordS<S> co;
#pragma unroll
    for (int ti = 0; ti < S::MT; ++ti)
#pragma unroll
        for (int tj = 0; tj < S::NT; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) epi(r0 + co.row_base + 16 * ti, c0 + co.col_base + 16 * tj + 4 * r, acc.v[ti][tj][r]);
}

// A (np x np) times `ncols` (a multiple of 32) columns of B: 64-column tiles, a 32-column one for the rest
template <int TM, class Epi>
__device__ __forceinline__ void mm_cols(const double* __restrict__ A, const double* __restrict__ B, int np, int ncols, double* smem,
                                        Epi&& epi) {
    for (int r0 = 0; r0 < np; r0 += TM) {
        int c0 = 0;
        for (; c0 + 64 <= ncols; c0 += 64) mm_tile<GemmShape<TM, 64, 2, 2>>(A, B, np, r0, c0, smem, epi);
        if (c0 < ncols) mm_tile<GemmShape<TM, 32, 2, 2>>(A, B, np, r0, c0, smem, epi);
    }
}

// PROD: the instantiation that serves need 3 and 4 and nothing else (the value modes' code is unchanged by it)
template <int TM, bool PROD>
__global__ void __launch_bounds__(256, 2) k_tdb_mfma(TdbmArgs a) {
    const int n = a.T.n, z = a.P.z, need = a.need;
    const TdbmLayout L = tdbm_layout(a.T, need);
    const int np = L.np, p = L.p, P2 = L.P2, Q = L.Q, C = L.C, Ctot = L.Ctot, ucols = L.ucols;
    const int tid = threadIdx.x;
    const size_t nn = (size_t)np * np;
    __shared__ __attribute__((aligned(16))) double smem[GemmShape<TM, 64, 2, 2>::SMEM_DOUBLES];
    __shared__ double vsh[256];                                // the vector of a vector pass
    __shared__ unsigned char pair_a[TDBM_MAX_PAIRS], pair_b[TDBM_MAX_PAIRS];
    __shared__ double w_theta[PROD ? 2 * MAX_DRIVES + 2 : 1];   // J w: the entries of w at the interval's parameters
    // first-order jets that enter the epilogue of the forward tile, and the coefficient row of the first of them
    const int pj = PROD && need == 3 ? 1 : p, row1 = PROD && need == 3 ? 1 + p : 1;
    for (int e = tid; e < (PROD ? 0 : P2); e += 256) {
        int aa, bb;
        tdb_pair_unrank(e, p, &aa, &bb);
        pair_a[e] = (unsigned char)aa; pair_b[e] = (unsigned char)bb;
    }
    double* S = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    double* Y = S + L.oY;
    double* ACC = S + L.oACC;
    double* TA = S + L.oTA;
    double* TB = S + L.oTB;
    double* M0 = S + L.oM0;
    double* U = S + L.oU;       // [Q][ucols][np]
    double* UB = S + L.oUB;     // [32][np]
    double* coefs = S + L.oCoef;  // [jets][Q]
    __syncthreads();

    for (int64_t it = blockIdx.x; it < a.count; it += gridDim.x) {
        const int64_t kn = a.i_lo + it;
        const double* zk = a.Z + kn * z;
        const double* zk1 = zk + z;
        const double tk = zk[a.T.t_off], dt = zk[a.P.dt_idx];

        // coefficients of `njet` jets at tau, then M0 = sum_q c_q B_q (or B_q' for the adjoint) in the fixed order q = 0, 1, ...
        auto form_m0 = [&](double tau, int njet, const double* __restrict__ B) {
            for (int e = tid; e < njet * Q; e += 256) coefs[e] = tdbm_coef(a.T, zk, zk1, tk, dt, tau, p, e / Q, e % Q);
            __syncthreads();
            if (PROD && need == 3) {   // the directional row, behind rows 0 .. p (read by the epilogue, after the barriers below)
                for (int q = tid; q < Q; q += 256) coefs[(size_t)(1 + p) * Q + q] = tdbm_dir_coef(coefs, Q, p, q, w_theta);
            }
            for (size_t e = 2 * (size_t)tid; e < nn; e += 512) {
                d2 acc = d2{0.0, 0.0};
                for (int q = 0; q < Q; ++q) {
                    const double cf = coefs[q];
                    const d2 b = *reinterpret_cast<const d2*>(B + q * nn + e);
                    acc.x += cf * b.x; acc.y += cf * b.y;
                }
                *reinterpret_cast<d2*>(M0 + e) = acc;
            }
            __syncthreads();
        };
        // U[q][0][:] = B_q v for one vector v (np rows): thread per (q, row), four partial sums over k mod 4 joined in a fixed order
        auto vec_pass = [&](const double* __restrict__ B, const double* __restrict__ v) {
            for (int r = tid; r < np; r += 256) vsh[r] = v[r];
            __syncthreads();
            for (int e = tid; e < Q * np; e += 256) {
                const int q = e / np, r = e - q * np;
                const double* col = B + q * nn + r;
                double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
                for (int k = 0; k < np; k += 4) {
                    s0 += col[(size_t)k * np] * vsh[k];
                    s1 += col[(size_t)(k + 1) * np] * vsh[k + 1];
                    s2 += col[(size_t)(k + 2) * np] * vsh[k + 2];
                    s3 += col[(size_t)(k + 3) * np] * vsh[k + 3];
                }
                U[(size_t)q * ucols * np + r] = (s0 + s1) + (s2 + s3);
            }
            __syncthreads();
        };

        if (PROD && need == 3 && tid < p) w_theta[tid] = a.w[kn * z + tdb_param_entry(a.T, z, a.P.dt_idx, tid)];
        // initial values: x = x_k, Phi = I (d = w_x(k) in a J w call), everything else (padding included) 0
        for (size_t e = tid; e < (size_t)np * Ctot; e += 256) {
            const int c = (int)(e / np), r = (int)(e - (size_t)c * np);
            double v = 0.0;
            if (c == 0) v = r < n ? zk[a.T.x_off + r] : 0.0;
            else if (PROD && need == 3 && c == 1) v = r < n ? a.w[kn * z + a.T.x_off + r] : 0.0;
            else if (c >= L.Cv) v = (c - L.Cv == r && r < n) ? 1.0 : 0.0;
            Y[e] = v;
        }
        __syncthreads();

        const double h = 1.0 / a.T.substeps;
        const int njet_fwd = PROD ? 1 + p : (need == 0 ? 1 : (need == 1 ? 1 + p : 1 + p + P2));
        for (int step = 0; step < a.T.substeps; ++step) {
            for (int stage = 0; stage < 4; ++stage) {
                const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
                const double* IN = stage == 0 ? Y : (stage == 2 ? TB : TA);
                double* OUT = stage == 0 ? TA : (stage == 1 ? TB : (stage == 2 ? TA : Y));
                if (stage != 2) form_m0(tau, njet_fwd, a.Bp);   // stages 1 and 2 share their time
                // U_q = B_q y for the vectors whose jets enter this call: x (Jacobian), x and x_b (Hessian)
                if (PROD || need == 1) vec_pass(a.Bp, IN);
                else if (!PROD && need == 2) {
                    for (int q = 0; q < Q; ++q)
                        mm_cols<TM>(a.Bp + q * nn, IN, np, TDBM_VEC, smem,
                                    [&](int row, int col, double v) { U[((size_t)q * TDBM_VEC + col) * np + row] = v; });
                    __syncthreads();
                }
                const double w_acc = (stage == 0 || stage == 3) ? h / 6.0 : h / 3.0;
                const double w_tmp = stage == 2 ? h : 0.5 * h;
                // K = M0 IN (+ the jets' terms), then the RK4 update of this stage
                mm_cols<TM>(M0, IN, np, Ctot, smem, [&](int row, int col, double K) {
                    if (need >= 1 && col >= 1 && col <= pj) {
                        const double* cf = coefs + (size_t)(row1 + col - 1) * Q;   // jet 1 + b, b = col - 1 (J w: the directional row)
                        double s = 0.0;
                        for (int q = 0; q < Q; ++q) s += cf[q] * U[(size_t)q * ucols * np + row];
                        K += s;
                    } else if (!PROD && need == 2 && col > p && col < C) {
                        const int e = col - 1 - p, aa = pair_a[e], bb = pair_b[e];
                        const double *ca = coefs + (size_t)(1 + aa) * Q, *cb = coefs + (size_t)(1 + bb) * Q, *cab = coefs + (size_t)(1 + p + e) * Q;
                        double s = 0.0;
                        for (int q = 0; q < Q; ++q) {
                            const double* uq = U + (size_t)q * TDBM_VEC * np + row;
                            s += ca[q] * uq[(size_t)(1 + bb) * np] + cb[q] * uq[(size_t)(1 + aa) * np] + cab[q] * uq[0];
                        }
                        K += s;
                    }
                    const size_t e = (size_t)col * np + row;
                    const double y0 = Y[e];
                    if (stage == 0) { ACC[e] = y0 + w_acc * K; OUT[e] = y0 + w_tmp * K; }
                    else if (stage < 3) { ACC[e] += w_acc * K; OUT[e] = y0 + w_tmp * K; }
                    else OUT[e] = ACC[e] + w_acc * K;
                });
                __syncthreads();
            }
        }

        if (PROD) {
            if (need == 3) {
                for (int r = tid; r < n; r += 256) a.out[a.T.row_off + kn * n + r] = a.w[(kn + 1) * z + a.T.x_off + r] - Y[np + r];
            } else {
                const double* wk = a.w + a.T.row_off + kn * n;
                double* out = a.out + kn * (int64_t)(n + p);
                for (int b = tid; b < p; b += 256) {   // w_k' (dPhi_k / dtheta_b) x_k
                    double s = 0.0;
                    const double* xb = Y + (size_t)(1 + b) * np;
                    for (int r = 0; r < n; ++r) s += wk[r] * xb[r];
                    out[n + b] = s;
                }
                // lambda = Phi_k' w_k: one adjoint column, backward through the steps; ubar = sum_q c_q (B_q' kbar), q in order
                double* W = TA;
                double* WN = TB;
                double* KB = ACC;
                for (int e = tid; e < np; e += 256) { W[e] = e < n ? wk[e] : 0.0; UB[e] = 0.0; }
                __syncthreads();
                for (int step = a.T.substeps - 1; step >= 0; --step) {
                    for (int e = tid; e < np; e += 256) WN[e] = W[e];
                    for (int stage = 3; stage >= 0; --stage) {
                        const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
                        if (stage != 1)   // stages 2 and 1 share their time
                            for (int q = tid; q < Q; q += 256) coefs[q] = tdbm_coef(a.T, zk, zk1, tk, dt, tau, p, 0, q);
                        const double cw = (stage == 3 || stage == 0) ? h / 6.0 : h / 3.0;
                        const double cu = stage == 3 ? 0.0 : (stage == 2 ? h : 0.5 * h);
                        for (int e = tid; e < np; e += 256) KB[e] = cw * W[e] + (cu != 0.0 ? cu * UB[e] : 0.0);
                        __syncthreads();
                        vec_pass(a.BpT, KB);   // U_q = B_q' kbar
                        for (int r = tid; r < np; r += 256) {
                            double u = 0.0;
                            for (int q = 0; q < Q; ++q) u += coefs[q] * U[(size_t)q * np + r];
                            UB[r] = u;
                            WN[r] += u;
                        }
                        __syncthreads();
                    }
                    for (int e = tid; e < np; e += 256) W[e] = WN[e];
                    __syncthreads();
                }
                for (int i = tid; i < n; i += 256) out[i] = W[i];
            }
            __syncthreads();   // the slot is reused by this workgroup's next interval
            continue;
        }
        // ---- outputs (blocks of a generic integrator, laid out as k_tdb writes them)
        for (int r = tid; r < n; r += 256) a.vals[kn * n + r] = zk1[a.T.x_off + r] - Y[r];
        auto zz_of = [&](int b) { return tdb_param_entry(a.T, z, a.P.dt_idx, b); };
        if (need == 1) {
            double* J = a.jac + kn * (int64_t)n * 2 * z;
            for (int64_t e = tid; e < (int64_t)n * 2 * z; e += 256) J[e] = 0.0;
            __syncthreads();
            const double* PHI = Y + (size_t)L.Cv * np;
            for (int e = tid; e < n * n; e += 256) {
                const int i = e / n, r = e - i * n;
                J[(int64_t)(a.T.x_off + i) * n + r] = -PHI[(size_t)i * np + r];
            }
            for (int r = tid; r < n; r += 256) J[(int64_t)(z + a.T.x_off + r) * n + r] = 1.0;
            __syncthreads();
            // parameter columns ADD (a component may serve twice); row r belongs to one thread, b in order
            for (int r = tid; r < n; r += 256)
                for (int b = 0; b < p; ++b) J[(int64_t)zz_of(b) * n + r] -= Y[(size_t)(1 + b) * np + r];
        } else if (need == 2) {
            // discrete adjoint lambda = Phi' mu and its parameter sensitivities lambda_b, backward through the steps (k_tdb's
            // recursion).  Columns 0 .. p of W: lambda, lambda_b; Y keeps x_ab for the (theta, theta) block.
            const double* muk = a.mu + a.T.row_off + kn * n;
            double* W = TA;
            double* WN = TB;
            double* KB = ACC;
            const int CA = 1 + p, nv = np * TDBM_VEC;
            for (int e = tid; e < nv; e += 256) { W[e] = e < n ? muk[e] : 0.0; UB[e] = 0.0; }
            __syncthreads();
            for (int step = a.T.substeps - 1; step >= 0; --step) {
                for (int e = tid; e < nv; e += 256) WN[e] = W[e];
                for (int stage = 3; stage >= 0; --stage) {
                    const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
                    if (stage != 1) form_m0(tau, CA, a.BpT);   // stages 2 and 1 share their time
                    const double cw = (stage == 3 || stage == 0) ? h / 6.0 : h / 3.0;
                    const double cu = stage == 3 ? 0.0 : (stage == 2 ? h : 0.5 * h);
                    for (int e = tid; e < nv; e += 256) KB[e] = cw * W[e] + (cu != 0.0 ? cu * UB[e] : 0.0);
                    __syncthreads();
                    vec_pass(a.BpT, KB);   // U_q = B_q' kbar_0 (ucols = 32 in a Hessian call: column 0 of each q)
                    // ubar_c = M0' kbar_c (+ M_b' kbar_0 for the sensitivity columns)
                    mm_cols<TM>(M0, KB, np, TDBM_VEC, smem, [&](int row, int col, double u) {
                        if (col >= 1 && col <= p) {
                            const double* cf = coefs + (size_t)col * Q;
                            double s = 0.0;
                            for (int q = 0; q < Q; ++q) s += cf[q] * U[(size_t)q * ucols * np + row];
                            u += s;
                        }
                        const size_t e = (size_t)col * np + row;
                        UB[e] = u;
                        WN[e] += u;
                    });
                    __syncthreads();
                }
                for (int e = tid; e < nv; e += 256) W[e] = WN[e];
                __syncthreads();
            }

            const int ld = 2 * z;
            double* Hb = a.hess + kn * (int64_t)4 * z * z;
            for (int64_t e = tid; e < (int64_t)4 * z * z; e += 256) Hb[e] = 0.0;
            __syncthreads();
            // (x_i, theta_b) = -d lambda_i / d theta_b: thread i owns row x_i in the first pass and column x_i in the second, b in order
            for (int i = tid; i < n; i += 256)
                for (int b = 0; b < p; ++b) Hb[(a.T.x_off + i) + (int64_t)ld * zz_of(b)] -= W[(size_t)(1 + b) * np + i];
            __syncthreads();
            for (int i = tid; i < n; i += 256)
                for (int b = 0; b < p; ++b) Hb[zz_of(b) + (int64_t)ld * (a.T.x_off + i)] -= W[(size_t)(1 + b) * np + i];
            __syncthreads();
            // (theta_a, theta_b) = -mu' x_ab: the dot products in parallel (into UB), then one thread adds them in order
            for (int e = tid; e < P2; e += 256) {
                double s = 0.0;
                const double* xab = Y + (size_t)(1 + p + e) * np;
                for (int r = 0; r < n; ++r) s += muk[r] * xab[r];
                UB[e] = s;
            }
            __syncthreads();
            if (tid == 0)
                for (int e = 0; e < P2; ++e) {
                    const int ra = zz_of(pair_a[e]), rb = zz_of(pair_b[e]);
                    Hb[ra + (int64_t)ld * rb] -= UB[e];
                    if (pair_a[e] != pair_b[e]) Hb[rb + (int64_t)ld * ra] -= UB[e];
                }
        }
        __syncthreads();   // the slot is reused by this workgroup's next interval
    }
}


// ---- the group form (DTO_FLAG_SHARED_GENERATORS): `Pm` integrators of one system -- equal B_q, controls, time and
// scheme, each with its own state component and rows -- in ONE launch.  Everything that does not depend on the ket is done once per
// stage time or stage: the coefficient table, M0 / M0', and in a Jacobian call the Phi block.  Columns of one call:
//         defect    x^1 .. x^Pm | zeros to 32
//         Jacobian  [x^i, x^i_b (p)] member after member | zeros to a multiple of 32 | Phi (np columns, one for the group)
//         Hessian   [x^i, x^i_b, x^i_ab | zeros to a multiple of 32] member after member; the adjoint: one 32-column tile
//                   [lambda^i, lambda^i_b] per member, from that member's mu rows
// A member's columns go through the arithmetic they have in k_tdb_mfma: a GEMM column is a chain of MFMAs over k that does not
// depend on its neighbours or on the tile it sits in, the epilogues and the vector pass keep their expressions and sum orders.  So a
// member's output has the bits of the lone kernel's, whatever the group, the member's position, the grid or the slot.
struct TdbgLayout {
    int np, p, P2, Q, C1, cstride, Cv, Ctot, ustep, ucols;
    size_t oY, oACC, oTA, oTB, oM0, oU, oUB, oCoef, total;
};
inline __host__ __device__ TdbgLayout tdbg_layout(const KTdb& T, int need, int Pm) {
    TdbgLayout L;
    L.np = pad32(T.n);
    L.p = tdb_num_params(T.m, T.order);
    L.P2 = tdb_num_pairs(L.p);
    L.Q = tdb_num_shared(T.m, T.nmod);
    L.C1 = need == 0 ? 1 : (need == 1 ? 1 + L.p : 1 + L.p + L.P2);   // meaningful columns of one member
    L.cstride = need == 2 ? pad32(L.C1) : L.C1;                       // columns from one member to the next
    L.Cv = pad32(Pm * L.cstride);
    L.Ctot = L.Cv + (need == 1 ? L.np : 0);
    L.ustep = need == 2 ? TDBM_VEC : 1;                               // U columns of one member and q
    L.ucols = Pm * L.ustep;
    const size_t cols = (size_t)L.np * L.Ctot;
    L.oY = 0; L.oACC = cols; L.oTA = 2 * cols; L.oTB = 3 * cols;
    L.oM0 = 4 * cols;
    L.oU = L.oM0 + (size_t)L.np * L.np;
    L.oUB = L.oU + (size_t)L.Q * L.ucols * L.np;
    L.oCoef = L.oUB + (need == 2 ? (size_t)L.np * TDBM_VEC * Pm : 0);
    L.total = L.oCoef + (size_t)(1 + L.p + L.P2) * L.Q;
    L.total = (L.total + 1) & ~(size_t)1;
    return L;
}

struct TdbgArgs {
    KProb P;
    KTdb T;           // the leader's: everything but x_off and row_off is the group's
    KTdbGroup G;
    const double* Bp;
    const double* BpT;
    const double* Z;
    const double* mu;
    int need;
    int64_t i_lo, count;
    double* scratch;
    int64_t scratch_stride;
};

template <int TM>
__global__ void __launch_bounds__(256, 2) k_tdb_mfma_group(TdbgArgs a) {
    const int n = a.T.n, z = a.P.z, need = a.need, Pm = a.G.count;
    const TdbgLayout L = tdbg_layout(a.T, need, Pm);
    const int np = L.np, p = L.p, P2 = L.P2, Q = L.Q, C1 = L.C1, cstride = L.cstride, Ctot = L.Ctot, ustep = L.ustep, ucols = L.ucols;
    const int tid = threadIdx.x;
    const size_t nn = (size_t)np * np;
    __shared__ __attribute__((aligned(16))) double smem[GemmShape<TM, 64, 2, 2>::SMEM_DOUBLES];
    __shared__ double vsh[TDB_SHARE_MAX * 256];                // the members' vectors of a vector pass
    __shared__ unsigned char pair_a[TDBM_MAX_PAIRS], pair_b[TDBM_MAX_PAIRS];
    for (int e = tid; e < P2; e += 256) {
        int aa, bb;
        tdb_pair_unrank(e, p, &aa, &bb);
        pair_a[e] = (unsigned char)aa; pair_b[e] = (unsigned char)bb;
    }
    double* S = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    double* Y = S + L.oY;
    double* ACC = S + L.oACC;
    double* TA = S + L.oTA;
    double* TB = S + L.oTB;
    double* M0 = S + L.oM0;
    double* U = S + L.oU;         // [Q][Pm][ustep][np]
    double* UB = S + L.oUB;       // [Pm][32][np] (Hessian calls)
    double* coefs = S + L.oCoef;  // [jets][Q]
    __syncthreads();

    for (int64_t it = blockIdx.x; it < a.count; it += gridDim.x) {
        const int64_t kn = a.i_lo + it;
        const double* zk = a.Z + kn * z;
        const double* zk1 = zk + z;
        const double tk = zk[a.T.t_off], dt = zk[a.P.dt_idx];

        // as in k_tdb_mfma, once for the group
        auto form_m0 = [&](double tau, int njet, const double* __restrict__ B) {
            for (int e = tid; e < njet * Q; e += 256) coefs[e] = tdbm_coef(a.T, zk, zk1, tk, dt, tau, p, e / Q, e % Q);
            __syncthreads();
            for (size_t e = 2 * (size_t)tid; e < nn; e += 512) {
                d2 acc = d2{0.0, 0.0};
                for (int q = 0; q < Q; ++q) {
                    const double cf = coefs[q];
                    const d2 b = *reinterpret_cast<const d2*>(B + q * nn + e);
                    acc.x += cf * b.x; acc.y += cf * b.y;
                }
                *reinterpret_cast<d2*>(M0 + e) = acc;
            }
            __syncthreads();
        };
        // U[q][i][0][:] = B_q v^i for the members' vectors v^i = v + i vstride: thread per (q, row), every B_q entry read once and
        // used for all members; per vector the four partial sums over k mod 4 of k_tdb_mfma's pass, joined in its order
        auto vec_pass = [&](const double* __restrict__ B, const double* __restrict__ v, size_t vstride) {
            for (int i = 0; i < Pm; ++i)
                for (int r = tid; r < np; r += 256) vsh[i * 256 + r] = v[i * vstride + r];
            __syncthreads();
            for (int e = tid; e < Q * np; e += 256) {
                const int q = e / np, r = e - q * np;
                const double* col = B + q * nn + r;
                double s0[TDB_SHARE_MAX], s1[TDB_SHARE_MAX], s2[TDB_SHARE_MAX], s3[TDB_SHARE_MAX];
#pragma unroll
                for (int i = 0; i < TDB_SHARE_MAX; ++i) s0[i] = s1[i] = s2[i] = s3[i] = 0.0;
                for (int k = 0; k < np; k += 4) {
                    const double b0 = col[(size_t)k * np], b1 = col[(size_t)(k + 1) * np], b2 = col[(size_t)(k + 2) * np],
                                 b3 = col[(size_t)(k + 3) * np];
#pragma unroll
                    for (int i = 0; i < TDB_SHARE_MAX; ++i)
                        if (i < Pm) {
                            const double* vv = vsh + i * 256 + k;
                            s0[i] += b0 * vv[0];
                            s1[i] += b1 * vv[1];
                            s2[i] += b2 * vv[2];
                            s3[i] += b3 * vv[3];
                        }
                }
#pragma unroll
                for (int i = 0; i < TDB_SHARE_MAX; ++i)
                    if (i < Pm) U[((size_t)q * ucols + (size_t)i * ustep) * np + r] = (s0[i] + s1[i]) + (s2[i] + s3[i]);
            }
            __syncthreads();
        };

        // initial values: x^i = x^i_k, Phi = I, everything else (padding included) 0
        for (size_t e = tid; e < (size_t)np * Ctot; e += 256) {
            const int c = (int)(e / np), r = (int)(e - (size_t)c * np);
            Y[e] = (c >= L.Cv && c - L.Cv == r && r < n) ? 1.0 : 0.0;
        }
        __syncthreads();
        for (int i = 0; i < Pm; ++i)
            for (int r = tid; r < n; r += 256) Y[(size_t)i * cstride * np + r] = zk[a.G.m[i].x_off + r];
        __syncthreads();

        const double h = 1.0 / a.T.substeps;
        const int njet_fwd = need == 0 ? 1 : (need == 1 ? 1 + p : 1 + p + P2);
        for (int step = 0; step < a.T.substeps; ++step) {
            for (int stage = 0; stage < 4; ++stage) {
                const TdbFwdStage sg = tdb_fwd_stage(step, stage, h);
                const double* IN = tdb_fwd_in(stage, Y, TA, TB);
                double* OUT = tdb_fwd_out(stage, Y, TA, TB);
                if (tdb_fwd_new_jets(stage)) form_m0(sg.tau, njet_fwd, a.Bp);
                // U_q = B_q y for the vectors whose jets enter this call: x^i (Jacobian), x^i and x^i_b (Hessian)
                if (need == 1) vec_pass(a.Bp, IN, (size_t)cstride * np);
                else if (need == 2) {
                    for (int q = 0; q < Q; ++q)
                        for (int i = 0; i < Pm; ++i)
                            mm_cols<TM>(a.Bp + q * nn, IN + (size_t)i * cstride * np, np, TDBM_VEC, smem, [&](int row, int col, double v) {
                                U[((size_t)q * ucols + (size_t)i * TDBM_VEC + col) * np + row] = v;
                            });
                    __syncthreads();
                }
                // K = M0 IN (+ the jets' terms of the column's member), then the RK4 update of this stage
                mm_cols<TM>(M0, IN, np, Ctot, smem, [&](int row, int col, double K) {
                    if (need >= 1 && col < Pm * cstride) {
                        const int i = col / cstride, lc = col - i * cstride;   // member, and the column inside its block
                        const double* ui = U + (size_t)i * ustep * np + row;
                        if (lc >= 1 && lc <= p) {
                            const double* cf = coefs + (size_t)lc * Q;   // jet 1 + b, b = lc - 1
                            double s = 0.0;
                            for (int q = 0; q < Q; ++q) s += cf[q] * ui[(size_t)q * ucols * np];
                            K += s;
                        } else if (need == 2 && lc > p && lc < C1) {
                            const int e = lc - 1 - p, aa = pair_a[e], bb = pair_b[e];
                            const double *ca = coefs + (size_t)(1 + aa) * Q, *cb = coefs + (size_t)(1 + bb) * Q, *cab = coefs + (size_t)(1 + p + e) * Q;
                            double s = 0.0;
                            for (int q = 0; q < Q; ++q) {
                                const double* uq = ui + (size_t)q * ucols * np;
                                s += ca[q] * uq[(size_t)(1 + bb) * np] + cb[q] * uq[(size_t)(1 + aa) * np] + cab[q] * uq[0];
                            }
                            K += s;
                        }
                    }
                    const size_t e = (size_t)col * np + row;
                    const double y0 = Y[e];
                    if (stage == 0) { ACC[e] = y0 + sg.w_acc * K; OUT[e] = y0 + sg.w_tmp * K; }
                    else if (stage < 3) { ACC[e] += sg.w_acc * K; OUT[e] = y0 + sg.w_tmp * K; }
                    else OUT[e] = ACC[e] + sg.w_acc * K;
                });
                __syncthreads();
            }
        }

        // ---- outputs: every member's own blocks, laid out as k_tdb_mfma writes them
        for (int i = 0; i < Pm; ++i) {
            const int xo = a.G.m[i].x_off;
            const double* yi = Y + (size_t)i * cstride * np;
            for (int r = tid; r < n; r += 256) a.G.m[i].vals[kn * n + r] = zk1[xo + r] - yi[r];
        }
        auto zz_of = [&](int b) { return tdb_param_entry(a.T, z, a.P.dt_idx, b); };
        if (need == 1) {
            for (int i = 0; i < Pm; ++i) {
                double* J = a.G.m[i].jac + kn * (int64_t)n * 2 * z;
                for (int64_t e = tid; e < (int64_t)n * 2 * z; e += 256) J[e] = 0.0;
            }
            __syncthreads();
            const double* PHI = Y + (size_t)L.Cv * np;
            for (int i = 0; i < Pm; ++i) {   // -Phi to every member, the identity at its own z_{k+1} columns
                const int xo = a.G.m[i].x_off;
                double* J = a.G.m[i].jac + kn * (int64_t)n * 2 * z;
                for (int e = tid; e < n * n; e += 256) {
                    const int c = e / n, r = e - c * n;
                    J[(int64_t)(xo + c) * n + r] = -PHI[(size_t)c * np + r];
                }
                for (int r = tid; r < n; r += 256) J[(int64_t)(z + xo + r) * n + r] = 1.0;
            }
            __syncthreads();
            // parameter columns ADD (a component may serve twice); row r belongs to one thread, b in order
            for (int i = 0; i < Pm; ++i) {
                double* J = a.G.m[i].jac + kn * (int64_t)n * 2 * z;
                const double* yi = Y + (size_t)i * cstride * np;
                for (int r = tid; r < n; r += 256)
                    for (int b = 0; b < p; ++b) J[(int64_t)zz_of(b) * n + r] -= yi[(size_t)(1 + b) * np + r];
            }
        } else if (need == 2) {
            // the discrete adjoint of k_tdb_mfma, one 32-column tile [lambda^i, lambda^i_b] per member; Y keeps x^i_ab
            double* W = TA;
            double* WN = TB;
            double* KB = ACC;
            const int CA = 1 + p, nv = np * TDBM_VEC, nvg = nv * Pm;
            for (int e = tid; e < nvg; e += 256) { W[e] = 0.0; UB[e] = 0.0; }
            __syncthreads();
            for (int i = 0; i < Pm; ++i) {
                const double* muk = a.mu + a.G.m[i].row_off + kn * n;
                for (int r = tid; r < n; r += 256) W[(size_t)i * nv + r] = muk[r];
            }
            __syncthreads();
            for (int step = a.T.substeps - 1; step >= 0; --step) {
                for (int e = tid; e < nvg; e += 256) WN[e] = W[e];
                for (int stage = 3; stage >= 0; --stage) {
                    const TdbBwdStage sg = tdb_bwd_stage(step, stage, h);
                    if (tdb_bwd_new_jets(stage)) form_m0(sg.tau, CA, a.BpT);
                    const double cw = sg.cw, cu = sg.cu;
                    for (int e = tid; e < nvg; e += 256) KB[e] = cw * W[e] + (cu != 0.0 ? cu * UB[e] : 0.0);
                    __syncthreads();
                    vec_pass(a.BpT, KB, (size_t)nv);   // U_q = B_q' kbar^i_0 (column 0 of each member and q)
                    // ubar_c = M0' kbar_c (+ M_b' kbar_0 of the column's member for the sensitivity columns)
                    mm_cols<TM>(M0, KB, np, TDBM_VEC * Pm, smem, [&](int row, int col, double u) {
                        const int i = col / TDBM_VEC, lc = col - i * TDBM_VEC;
                        if (lc >= 1 && lc <= p) {
                            const double* cf = coefs + (size_t)lc * Q;
                            const double* ui = U + (size_t)i * ustep * np + row;
                            double s = 0.0;
                            for (int q = 0; q < Q; ++q) s += cf[q] * ui[(size_t)q * ucols * np];
                            u += s;
                        }
                        const size_t e = (size_t)col * np + row;
                        UB[e] = u;
                        WN[e] += u;
                    });
                    __syncthreads();
                }
                for (int e = tid; e < nvg; e += 256) W[e] = WN[e];
                __syncthreads();
            }

            const int ld = 2 * z;
            for (int i = 0; i < Pm; ++i) {
                double* Hb = a.G.m[i].hess + kn * (int64_t)4 * z * z;
                for (int64_t e = tid; e < (int64_t)4 * z * z; e += 256) Hb[e] = 0.0;
            }
            __syncthreads();
            // (x_i, theta_b) = -d lambda_i / d theta_b: thread r owns row x_r in the first pass and column x_r in the second, b in order
            for (int i = 0; i < Pm; ++i) {
                const int xo = a.G.m[i].x_off;
                double* Hb = a.G.m[i].hess + kn * (int64_t)4 * z * z;
                const double* Wi = W + (size_t)i * nv;
                for (int r = tid; r < n; r += 256)
                    for (int b = 0; b < p; ++b) Hb[(xo + r) + (int64_t)ld * zz_of(b)] -= Wi[(size_t)(1 + b) * np + r];
            }
            __syncthreads();
            for (int i = 0; i < Pm; ++i) {
                const int xo = a.G.m[i].x_off;
                double* Hb = a.G.m[i].hess + kn * (int64_t)4 * z * z;
                const double* Wi = W + (size_t)i * nv;
                for (int r = tid; r < n; r += 256)
                    for (int b = 0; b < p; ++b) Hb[zz_of(b) + (int64_t)ld * (xo + r)] -= Wi[(size_t)(1 + b) * np + r];
            }
            __syncthreads();
            // (theta_a, theta_b) = -mu' x_ab: the dot products in parallel (into UB), then one thread per member adds them in order
            for (int i = 0; i < Pm; ++i) {
                const double* muk = a.mu + a.G.m[i].row_off + kn * n;
                for (int e = tid; e < P2; e += 256) {
                    double s = 0.0;
                    const double* xab = Y + ((size_t)i * cstride + 1 + p + e) * np;
                    for (int r = 0; r < n; ++r) s += muk[r] * xab[r];
                    UB[(size_t)i * nv + e] = s;
                }
            }
            __syncthreads();
            if (tid < Pm) {
                double* Hb = a.G.m[tid].hess + kn * (int64_t)4 * z * z;
                const double* dots = UB + (size_t)tid * nv;
                for (int e = 0; e < P2; ++e) {
                    const int ra = zz_of(pair_a[e]), rb = zz_of(pair_b[e]);
                    Hb[ra + (int64_t)ld * rb] -= dots[e];
                    if (pair_a[e] != pair_b[e]) Hb[rb + (int64_t)ld * ra] -= dots[e];
                }
            }
        }
        __syncthreads();   // the slot is reused by this workgroup's next interval
    }
}

}  // namespace

int tdb_mfma_npad(int n) { return pad32(n); }

const char* tdb_mfma_refusal(const KTdb& T) {
    if (T.n < 1 || T.n > 256) return "time-dependent bilinear integrator: the device kernels take 1..256 states";
    if (T.substeps < 1) return "time-dependent bilinear integrator: substeps must be >= 1";
    if (T.nmod < 0) return "time-dependent bilinear integrator: n_mod must be >= 0";
    if (!tdb_table_fits(T.m, T.order, T.nmod))
        return "time-dependent bilinear integrator: coefficient table (1 + p + p (p+1) / 2) (m+1) (1 + n_mod) exceeds 6144 entries";
    return nullptr;
}

bool tdb_mfma_supported(const KTdb& T) { return T.n > 64 && tdb_mfma_refusal(T) == nullptr; }

size_t tdb_mfma_scratch_doubles(const KTdb& T, int need) { return tdbm_layout(T, need).total; }

// MFMA and vector-pass flops of one interval as executed (padding included): per stage the M0 product over all columns and the
// U_q products; per stage time the formation of M0
double tdb_mfma_flops(const KTdb& T, int need) {
    const TdbmLayout L = tdbm_layout(T, need);
    const double np2 = (double)L.np * L.np, S = T.substeps;
    const double form = 2.0 * L.Q * np2;
    double fwd = 4.0 * 2.0 * np2 * L.Ctot + 3.0 * form;
    if (need == 1 || need >= 3) fwd += 4.0 * 2.0 * L.Q * np2;
    if (need == 2) fwd += 4.0 * 2.0 * L.Q * np2 * TDBM_VEC;
    double bwd = 0.0;
    if (need == 2) bwd = 4.0 * (2.0 * np2 * TDBM_VEC + 2.0 * L.Q * np2) + 3.0 * form;
    if (need == 4) bwd = 4.0 * 2.0 * L.Q * np2;   // the one-column adjoint: vector passes only
    return S * (fwd + bwd);
}

hipError_t launch_tdb_mfma(hipStream_t st, const KProb& P, const KTdb& T, const double* Bp, const double* BpT, const double* dZ,
                           const double* dmu, int need, int64_t i_lo, int64_t count, double* vals, double* jac, double* hess,
                           double* scratch, size_t scratch_stride, int resident) {
    if (count <= 0) return hipSuccess;
    if (resident < 1 || tdbm_layout(T, need).total > scratch_stride) return hipErrorInvalidValue;
    TdbmArgs a{};
    a.P = P; a.T = T; a.Bp = Bp; a.BpT = BpT; a.Z = dZ; a.mu = dmu; a.need = need; a.i_lo = i_lo; a.count = count;
    a.vals = vals; a.jac = jac; a.hess = hess; a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride;
    const unsigned grid = (unsigned)std::min<int64_t>(count, resident);
    if (pad32(T.n) % 64 == 0) hipLaunchKernelGGL((k_tdb_mfma<64, false>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_tdb_mfma<32, false>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tdb_mfma_product(hipStream_t st, const KProb& P, const KTdb& T, const double* Bp, const double* BpT, const double* dZ,
                                   const double* dw, int need, double* out, double* scratch, size_t scratch_stride, int resident) {
    if (P.K <= 0) return hipSuccess;
    if ((need != 3 && need != 4) || resident < 1 || tdbm_layout(T, need).total > scratch_stride) return hipErrorInvalidValue;
    TdbmArgs a{};
    a.P = P; a.T = T; a.Bp = Bp; a.BpT = BpT; a.Z = dZ; a.need = need; a.i_lo = 0; a.count = P.K;
    a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride; a.w = dw; a.out = out;
    const unsigned grid = (unsigned)std::min<int64_t>(P.K, resident);
    if (pad32(T.n) % 64 == 0) hipLaunchKernelGGL((k_tdb_mfma<64, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_tdb_mfma<32, true>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

size_t tdb_mfma_group_scratch_doubles(const KTdb& T, int need, int members) { return tdbg_layout(T, need, members).total; }

// as tdb_mfma_flops, for one interval of a group launch: M0 and (Jacobian) the Phi block once, the vector blocks of all members
double tdb_mfma_group_flops(const KTdb& T, int need, int members) {
    const TdbgLayout L = tdbg_layout(T, need, members);
    const double np2 = (double)L.np * L.np, S = T.substeps;
    const double form = 2.0 * L.Q * np2;
    double fwd = 4.0 * 2.0 * np2 * L.Ctot + 3.0 * form;
    if (need == 1) fwd += 4.0 * 2.0 * L.Q * np2 * members;
    if (need == 2) fwd += 4.0 * 2.0 * L.Q * np2 * TDBM_VEC * members;
    double bwd = 0.0;
    if (need == 2) bwd = 4.0 * (2.0 * np2 * TDBM_VEC * members + 2.0 * L.Q * np2 * members) + 3.0 * form;
    return S * (fwd + bwd);
}

hipError_t launch_tdb_mfma_group(hipStream_t st, const KProb& P, const KTdb& T, const KTdbGroup& G, const double* Bp, const double* BpT,
                                 const double* dZ, const double* dmu, int need, int64_t i_lo, int64_t count, double* scratch,
                                 size_t scratch_stride, int resident) {
    if (count <= 0) return hipSuccess;
    if (need < 0 || need > 2 || G.count < 2 || G.count > TDB_SHARE_MAX || resident < 1 || tdbg_layout(T, need, G.count).total > scratch_stride)
        return hipErrorInvalidValue;
    TdbgArgs a{};
    a.P = P; a.T = T; a.G = G; a.Bp = Bp; a.BpT = BpT; a.Z = dZ; a.mu = dmu; a.need = need; a.i_lo = i_lo; a.count = count;
    a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride;
    const unsigned grid = (unsigned)std::min<int64_t>(count, resident);
    if (pad32(T.n) % 64 == 0) hipLaunchKernelGGL((k_tdb_mfma_group<64>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_tdb_mfma_group<32>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace dto
