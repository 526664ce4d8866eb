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
//     else 32.
//   * PERSISTENT GRID.  `resident` workgroups walk the intervals (interval i of the launch goes to workgroup i mod resident); the
//     scratch is one slot per workgroup, so it is sized by the grid and not by the number of intervals.
//   * ONE BODY FOR ONE INTEGRATOR AND FOR A GROUP.  A launch evaluates `Pm` integrators of one system (DTO_FLAG_SHARED_GENERATORS,
//     DESIGN 4.22): equal B_q, controls, time and scheme, each with its own state component and rows.  Everything that does not
//     depend on the ket is done once per stage time or stage: the coefficient table, M0 / M0', and in a Jacobian call the Phi
//     block.  A lone integrator is the group of one: k_tdb_mfma<TM, 1, .> has the member count as the constant 1, the group
//     instance k_tdb_mfma<TM, TDB_SHARE_MAX, false> reads it from its arguments.  Columns of one call, each of np rows
//     (column-major, leading dimension np; layout in dto_tdb_mfma_layout.h):
//         defect    x^1 .. x^Pm | zeros to 32
//         Jacobian  [x^i, x^i_b (p)] member after member | zeros to a multiple of 32 | Phi (np columns, starts as the identity,
//                   one for the group)                                                          -- the Phi block carries the flops
//         Hessian   [x^i, x^i_b, x^i_ab (p (p+1) / 2) | zeros to a multiple of 32] member after member    -- no Phi, no Phi_b
//                   the adjoint: one 32-column tile [lambda^i, lambda^i_b] per member, from that member's mu rows
//     The single-vector U_q of Jacobian calls and of the adjoint is a vector pass (one thread per (q, row), B_q read once and used
//     for all members).  A GEMM column is a chain of MFMAs over k that does not depend on its neighbours or on the tile it sits in,
//     and the epilogues and the vector pass apply one expression and one sum order to every member.  So a member's output does not
//     depend on the group, the member's position, the grid or the slot: bit for bit what the integrator gives alone.
//
// Numerical rules: what a workgroup computes is a function of its interval's data alone (not of the grid, the shard or the slot);
// every sum has a fixed order; there is no floating-point atomic.  Output entries that share a position (a component that serves
// twice, e.g. the timestep listed as the time variable) are added by one thread in a fixed order.  Padded rows and columns are
// computed (they are zeros) and never written to vals / jac / hess.
//
// Product modes (the PROD instantiation of the same kernel, one member; need 3: J w, need 4: J' w; formulas in dto_tdb.hip).  The
// column block is one 32-column tile and there is no Phi block:
//         J w       x, d | zeros to 32          d' = M0 d + M_w x: the Jacobian call's epilogue with ONE jet, the directional row
//         J' w      x, x_b (p) | zeros to 32    the Jacobian call's vector block; then p dot products with w_k
// M0 is formed for the forward tile as in the value calls.  The adjoint of J' w is a single column, so it forms no M0 and runs no
// GEMM: ubar = M0' kbar = sum_q c_q (B_q' kbar) from the vector pass that the Hessian's adjoint already has.  Results go to y (J w:
// the integrator's rows, one writer per entry) or to the per-interval staging of n + p doubles that k_tdb_jtv_place adds into y.
//
// The stage loops take the RK4 tableau from dto_tdb_scheme.h (tdb_fwd_stage, tdb_bwd_stage and their companions).
#include <algorithm>

#include "dto_gemm.hip.h"
#include "dto_kernels.h"
#include "dto_tdb_coef.hip.h"
#include "dto_tdb_mfma_layout.h"

namespace dto {

namespace {

constexpr int TDBM_MAX_PAIRS = 160;   // p (p+1) / 2 <= 136 at 7 drives, order 1

inline TdbmLayout tdbm_layout_of(const KTdb& T, int need, int members) { return tdbm_layout(T.n, T.m, T.order, T.nmod, need, members); }

struct TdbmArgs {
    KProb P;
    KTdb T;              // of any member: everything but x_off and row_off is the group's
    KTdbGroup G;         // the members' state components, rows and blocks (product modes: one member, no blocks)
    const double* Bp;    // [Q][np][np] zero-padded B_q, column-major; q = j (1 + nmod) + c, c = 0: G_j, c >= 1: H_{c-1, j}
    const double* BpT;   // their transposes
    const double* Z;
    const double* mu;
    int need;
    int64_t i_lo, count;
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

// MAXM: compile-time bound on the members of a launch, 1 (the member count is the constant 1) or TDB_SHARE_MAX (it is a.G.count).
// PROD: the instantiation that serves need 3 and 4 and nothing else (the value modes' code is unchanged by it).
template <int TM, int MAXM, bool PROD>
__global__ void __launch_bounds__(256, 2) k_tdb_mfma(TdbmArgs a) {
    static_assert(MAXM == 1 || (MAXM == TDB_SHARE_MAX && !PROD), "the product modes take one integrator");
    const int n = a.T.n, z = a.P.z, need = a.need, Pm = MAXM == 1 ? 1 : a.G.count;
    const TdbmLayout L = tdbm_layout(a.T.n, a.T.m, a.T.order, a.T.nmod, need, Pm);
    const int np = L.np, p = L.p, P2 = L.P2, Q = L.Q, C1 = L.C1, cstride = L.cstride, Ctot = L.Ctot, ustep = L.ustep, ucols = L.ucols;
    const int tid = threadIdx.x;
    const size_t nn = (size_t)np * np;
    __shared__ __attribute__((aligned(16))) double smem[GemmShape<TM, 64, 2, 2>::SMEM_DOUBLES];
    __shared__ double vsh[MAXM * 256];                         // the members' vectors of a vector pass
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
    double* U = S + L.oU;         // [Q][Pm][ustep][np]
    double* UB = S + L.oUB;       // [Pm][32][np] (Hessian calls; one member: every call)
    double* coefs = S + L.oCoef;  // [jets][Q]
    __syncthreads();

    for (int64_t it = blockIdx.x; it < a.count; it += gridDim.x) {
        const int64_t kn = a.i_lo + it;
        const double* zk = a.Z + kn * z;
        const double* zk1 = zk + z;
        const double tk = zk[a.T.t_off], dt = zk[a.P.dt_idx];

        // coefficients of `njet` jets at tau, then M0 = sum_q c_q B_q (or B_q' for the adjoint) in the fixed order q = 0, 1, ...;
        // once for the group
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
        // U[q][i][0][:] = B_q v^i for the members' vectors v^i = v + i vstride (np rows): thread per (q, row), every B_q entry read
        // once and used for all members; per vector four partial sums over k mod 4, joined in a fixed order
        auto vec_pass = [&](const double* __restrict__ B, const double* __restrict__ v, size_t vstride) {
            for (int i = 0; i < Pm; ++i)
                for (int r = tid; r < np; r += 256) vsh[i * 256 + r] = v[i * vstride + r];
            __syncthreads();
            for (int e = tid; e < Q * np; e += 256) {
                const int q = e / np, r = e - q * np;
                const double* col = B + q * nn + r;
                double s0[MAXM], s1[MAXM], s2[MAXM], s3[MAXM];
#pragma unroll
                for (int i = 0; i < MAXM; ++i) s0[i] = s1[i] = s2[i] = s3[i] = 0.0;
                for (int k = 0; k < np; k += 4) {
                    const double b0 = col[(size_t)k * np], b1 = col[(size_t)(k + 1) * np], b2 = col[(size_t)(k + 2) * np],
                                 b3 = col[(size_t)(k + 3) * np];
#pragma unroll
                    for (int i = 0; i < MAXM; ++i)
                        if (i < Pm) {
                            const double* vv = vsh + i * 256 + k;
                            s0[i] += b0 * vv[0];
                            s1[i] += b1 * vv[1];
                            s2[i] += b2 * vv[2];
                            s3[i] += b3 * vv[3];
                        }
                }
#pragma unroll
                for (int i = 0; i < MAXM; ++i)
                    if (i < Pm) U[((size_t)q * ucols + (size_t)i * ustep) * np + r] = (s0[i] + s1[i]) + (s2[i] + s3[i]);
            }
            __syncthreads();
        };

        if (PROD && need == 3 && tid < p) w_theta[tid] = a.w[kn * z + tdb_param_entry(a.T, z, a.P.dt_idx, tid)];
        // initial values: x^i = x^i_k, Phi = I (d = w_x(k) in a J w call), everything else (padding included) 0
        for (size_t e = tid; e < (size_t)np * Ctot; e += 256) {
            const int c = (int)(e / np), r = (int)(e - (size_t)c * np);
            double v = 0.0;
            if (c < Pm * cstride) {
                const int i = MAXM == 1 ? 0 : c / cstride, lc = c - i * cstride;   // member, and the column inside its block
                if (lc == 0) v = r < n ? zk[a.G.m[i].x_off + r] : 0.0;
                else if (PROD && need == 3 && lc == 1) v = r < n ? a.w[kn * z + a.G.m[0].x_off + r] : 0.0;
            } else if (c >= L.Cv) v = (c - L.Cv == r && r < n) ? 1.0 : 0.0;
            Y[e] = v;
        }
        __syncthreads();

        const double h = 1.0 / a.T.substeps;
        const int njet_fwd = PROD ? 1 + p : (need == 0 ? 1 : (need == 1 ? 1 + p : 1 + p + P2));
        for (int step = 0; step < a.T.substeps; ++step) {
            for (int stage = 0; stage < 4; ++stage) {
                const TdbFwdStage sg = tdb_fwd_stage(step, stage, h);
                const double* IN = tdb_fwd_in(stage, Y, TA, TB);
                double* OUT = tdb_fwd_out(stage, Y, TA, TB);
                if (tdb_fwd_new_jets(stage)) form_m0(sg.tau, njet_fwd, a.Bp);   // stages 1 and 2 share their time
                // U_q = B_q y for the vectors whose jets enter this call: x^i (Jacobian), x^i and x^i_b (Hessian)
                if (PROD || need == 1) vec_pass(a.Bp, IN, (size_t)cstride * np);
                else if (!PROD && need == 2) {
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
                        const int i = MAXM == 1 ? 0 : col / cstride, lc = col - i * cstride;
                        const double* ui = U + (size_t)i * ustep * np + row;
                        if (lc >= 1 && lc <= pj) {
                            const double* cf = coefs + (size_t)(row1 + lc - 1) * Q;   // jet 1 + b, b = lc - 1 (J w: the directional row)
                            double s = 0.0;
                            for (int q = 0; q < Q; ++q) s += cf[q] * ui[(size_t)q * ucols * np];
                            K += s;
                        } else if (!PROD && need == 2 && lc > p && lc < C1) {
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
                    tdb_fwd_update(stage, sg.w_acc, sg.w_tmp, Y[e], K, ACC[e], OUT[e]);
                });
                __syncthreads();
            }
        }

        if (PROD) {
            const KTdbMember& mb = a.G.m[0];
            if (need == 3) {
                for (int r = tid; r < n; r += 256) a.out[mb.row_off + kn * n + r] = a.w[(kn + 1) * z + mb.x_off + r] - Y[np + r];
            } else {
                const double* wk = a.w + mb.row_off + kn * n;
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
                        const TdbBwdStage sg = tdb_bwd_stage(step, stage, h);
                        if (tdb_bwd_new_jets(stage))   // stages 2 and 1 share their time
                            for (int q = tid; q < Q; q += 256) coefs[q] = tdbm_coef(a.T, zk, zk1, tk, dt, sg.tau, p, 0, q);
                        for (int e = tid; e < np; e += 256) KB[e] = tdb_bwd_kbar(sg.cw, sg.cu, W[e], UB[e]);
                        __syncthreads();
                        vec_pass(a.BpT, KB, 0);   // U_q = B_q' kbar
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
        // ---- outputs: every member's own blocks (those of a generic integrator, laid out as k_tdb writes them)
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
            // discrete adjoint lambda = Phi' mu and its parameter sensitivities lambda_b, backward through the steps (k_tdb's
            // recursion): one 32-column tile [lambda^i, lambda^i_b] per member in W; Y keeps x^i_ab for the (theta, theta) block
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
                    if (tdb_bwd_new_jets(stage)) form_m0(sg.tau, CA, a.BpT);   // stages 2 and 1 share their time
                    for (int e = tid; e < nvg; e += 256) KB[e] = tdb_bwd_kbar(sg.cw, sg.cu, W[e], UB[e]);
                    __syncthreads();
                    vec_pass(a.BpT, KB, (size_t)nv);   // U_q = B_q' kbar^i_0 (column 0 of each member and q)
                    // ubar_c = M0' kbar_c (+ M_b' kbar_0 of the column's member for the sensitivity columns)
                    mm_cols<TM>(M0, KB, np, TDBM_VEC * Pm, smem, [&](int row, int col, double u) {
                        const int i = MAXM == 1 ? 0 : col / TDBM_VEC, lc = col - i * TDBM_VEC;
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
            // (x_r, theta_b) = -d lambda_r / d theta_b: thread r owns row x_r in the first pass and column x_r in the second, b in order
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

template <int MAXM, bool PROD>
hipError_t tdbm_launch(hipStream_t st, const TdbmArgs& a, int resident) {
    const unsigned grid = (unsigned)std::min<int64_t>(a.count, resident);
    if (tdbm_pad32(a.T.n) % 64 == 0) hipLaunchKernelGGL((k_tdb_mfma<64, MAXM, PROD>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_tdb_mfma<32, MAXM, PROD>), dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace

int tdb_mfma_npad(int n) { return tdbm_pad32(n); }

const char* tdb_mfma_refusal(const KTdb& T) {
    if (T.n < 1 || T.n > 256) return "time-dependent bilinear integrator: the device kernels take 1..256 states";
    if (T.substeps < 1) return "time-dependent bilinear integrator: substeps must be >= 1";
    if (T.nmod < 0) return "time-dependent bilinear integrator: n_mod must be >= 0";
    if (!tdb_table_fits(T.m, T.order, T.nmod))
        return "time-dependent bilinear integrator: coefficient table (1 + p + p (p+1) / 2) (m+1) (1 + n_mod) exceeds 6144 entries";
    return nullptr;
}

bool tdb_mfma_supported(const KTdb& T) { return T.n > 64 && tdb_mfma_refusal(T) == nullptr; }

size_t tdb_mfma_scratch_doubles(const KTdb& T, int need, int members) { return tdbm_layout_of(T, need, members).total; }

// MFMA and vector-pass flops of one interval of a launch as executed (padding included): per stage the M0 product over all columns
// (the Phi block of a Jacobian call once for the group) and the U_q products of every member; per stage time the formation of M0
double tdb_mfma_flops(const KTdb& T, int need, int members) {
    const TdbmLayout L = tdbm_layout_of(T, need, members);
    const double np2 = (double)L.np * L.np, S = T.substeps;
    const double form = 2.0 * L.Q * np2;
    double fwd = 4.0 * 2.0 * np2 * L.Ctot + 3.0 * form;
    if (need == 1 || need >= 3) fwd += 4.0 * 2.0 * L.Q * np2 * members;
    if (need == 2) fwd += 4.0 * 2.0 * L.Q * np2 * TDBM_VEC * members;
    double bwd = 0.0;
    if (need == 2) bwd = 4.0 * (2.0 * np2 * TDBM_VEC * members + 2.0 * L.Q * np2 * members) + 3.0 * form;
    if (need == 4) bwd = 4.0 * 2.0 * L.Q * np2;   // the one-column adjoint: vector passes only
    return S * (fwd + bwd);
}

hipError_t launch_tdb_mfma(hipStream_t st, const KProb& P, const KTdb& T, const KTdbGroup& G, const double* Bp, const double* BpT,
                           const double* dZ, const double* dmu, int need, int64_t i_lo, int64_t count, double* scratch,
                           size_t scratch_stride, int resident) {
    if (count <= 0) return hipSuccess;
    if (need < 0 || need > 2 || G.count < 1 || G.count > TDB_SHARE_MAX || resident < 1 || tdbm_layout_of(T, need, G.count).total > scratch_stride)
        return hipErrorInvalidValue;
    TdbmArgs a{};
    a.P = P; a.T = T; a.G = G; a.Bp = Bp; a.BpT = BpT; a.Z = dZ; a.mu = dmu; a.need = need; a.i_lo = i_lo; a.count = count;
    a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride;
    return G.count == 1 ? tdbm_launch<1, false>(st, a, resident) : tdbm_launch<TDB_SHARE_MAX, false>(st, a, resident);
}

hipError_t launch_tdb_mfma_product(hipStream_t st, const KProb& P, const KTdb& T, const double* Bp, const double* BpT, const double* dZ,
                                   const double* dw, int need, double* out, double* scratch, size_t scratch_stride, int resident) {
    if (P.K <= 0) return hipSuccess;
    if ((need != 3 && need != 4) || resident < 1 || tdbm_layout_of(T, need, 1).total > scratch_stride) return hipErrorInvalidValue;
    TdbmArgs a{};
    a.P = P; a.T = T; a.Bp = Bp; a.BpT = BpT; a.Z = dZ; a.need = need; a.i_lo = 0; a.count = P.K;
    a.G.count = 1;
    a.G.m[0] = KTdbMember{T.x_off, T.row_off, nullptr, nullptr, nullptr};
    a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride; a.w = dw; a.out = out;
    return tdbm_launch<1, true>(st, a, resident);
}

}  // namespace dto
