// dto_kernels.h -- launch interface between the host engine (dto_engine.cpp) and the HIP kernels
// (dto_kernels.hip).  Plain structs passed by value to kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "dto_minimize_plan.h" // options, flags and scalars of the reduced-space minimize call (KMinimize)
#include "dto_reduced_plan.h"  // index plan of the reduced-space operators (KReduced)
#include "dto_rollout_plan.h"  // index plan of the rollout's tree (KRollout's padding and level count)
#include "dto_slab_layout.h"  // where every Jacobian and Hessian entry sits in its value slab
#include "dto_sweep_plan.h"   // sweep planning: step budget, launch shapes (SweepTypes, the *SweepPlan structs and planners), form choice

namespace dto {

constexpr int TAYLOR_M = 16;                 // degree of the matrix Taylor polynomial
constexpr double THETA_16 = 0.78028743;      // backward-error radius of T_16 in double (Al-Mohy & Higham 2011, Table 3.1 method)
constexpr int COEF_STRIDE = 32;              // doubles per interval in the coefficient table
// T_16(B) = sum_{r<=16} B^r/r! with TWO products once B..B^4 are known (they come from the generator subspace):
//   Y = B^4 K(B),   T_16(B) = (Y + Pa(B)) (Y + Pb(B)) + Pc(B),   K, Pa, Pb, Pc of degree <= 4
// (Paterson-Stockmeyer needs three).  Constants from tools/expm_two_product_coeffs.py: the polynomial identity solved to
// 1e-50, factors without cancellation (sum of |terms| / exp = 1.03 at the radius); rounding error at ||B||_1 = 0.78:
// 6e-16 against 2e-16 for the Horner form.  Table layout per interval (each entry times its power of sigma = 2^-s):
constexpr int COEF_PC = 0, COEF_PA = 5, COEF_PB = 10, COEF_K = 15;
constexpr double EXPM2_K[5] = {0.0021247619694343247, 0.00021337327385069214, 1.9238573871783716e-05, 1.748961261071247e-06, 2.1862015763390587e-07};
constexpr double EXPM2_A[5] = {0.15657629060017847, 0.11131927651852432, 0.04459108138499527, 0.00629379053080652, -0.00037523326035530425};
constexpr double EXPM2_B[5] = {6.392946474783064, 1.8714151425525498, 0.2847453199197648, 0.035205562271892026, 0.0005680709246076226};
constexpr double EXPM2_C[5] = {-0.000983845027019532, -0.004677417588383601, -0.03797734224052902, 0.005772376398520401, 0.0016659351281941514};
// THREE products reach order 26 (degree 32): with Ya = Y + Pa, Yb = Y + Pb as above,
//   Y2 = Ya Yb,   L = Y2 + al Y + Pc,   R = Y2 + be Y + Pd,   r(B) = L R + Pe = exp(B) + O(B^27)
// Backward-error radius 2.819 against 0.780 for T_16: one product more buys 1.85 squarings, so the engine takes this form
// whenever the chunk's squaring counts drop by two for (nearly) every interval (alpha above ~3.1).  Of the free parameters
// left at order 26, a4 = c4 = d4 = 0 were imposed: the second product (two outputs, HBM-bound) then streams one matrix
// less.  Constants, radius and the rounding check (1.5e-15 at the radius, i.e. what T_16 shows after two squarings) from
// tools/expm_three_product_coeffs.py.  Table layout: Pe at 0, Pa, Pb, K as above, then the epilogue polynomials of the
// second product in terms of what that launch can read (Ya, not Y): L = Y2 + al Ya + (Pc - al Pa), R likewise.
constexpr double THETA_3P = 2.8188;
constexpr int COEF_L = 20, COEF_R = 26;      // 5 polynomial coefficients + the weight of Ya, each
constexpr double EXPM3_K[5] = {0.00010379876595047617, 6.073095185901804e-06, 3.1522969877676845e-07, -5.57963065580417e-09, 1.6549758371825144e-09};
constexpr double EXPM3_A[5] = {0.06925346208946212, 0.1399878337730723, 0.008815043145043342, -1.5454750321185654e-05, 0.0};
constexpr double EXPM3_B[5] = {7.864692916335445, 1.1432871789700823, 0.08599260924787294, 0.006001949142362251, 0.000114009585419753};
constexpr double EXPM3_C[5] = {1.4279329585415197, -0.648965244154349, -0.10937992097592901, -0.0031202517331481694, 0.0};
constexpr double EXPM3_D[5] = {0.0035917931833685884, -0.8738586720421705, -0.10354040058330033, 0.0006117561678190711, 0.0};
constexpr double EXPM3_E[5] = {-0.0814706004657684, 0.10462167443095102, 0.008296003021444887, 0.0020999533880951024, 0.00010675255813813872};
constexpr double EXPM3_AL = 0.009959087291030108, EXPM3_BE = 3.6322128429901483;
static_assert(EXPM3_A[4] == 0.0 && EXPM3_C[4] == 0.0 && EXPM3_D[4] == 0.0, "the second product's epilogue does not read A^4");
constexpr int PAIR_DCAP = 80;               // Taylor terms the Hessian's pairing path can store per sweep (rows / columns of its Beta table)
constexpr int MAX_DRIVES = 7;

// Problem-level constants every kernel may need.
struct KProb {
    int64_t N, K;       // knots, intervals (K = N-1)
    int32_t z, dt_idx;  // components per knot, timestep component
    int32_t D;          // sum of integrator state dims (Jacobian rows per interval)
    int32_t debug_bad_launch;  // option "debug_bad_launch" (tests of the error path): launches are given an invalid configuration
    int64_t kn_lo;      // first owned knot (0-based)
    int64_t n_knots;    // owned knots
    int64_t n_int;      // owned intervals: knots kn_lo .. kn_lo+n_int-1 (each < K)
    const int64_t* colptr;  // device, global Jacobian column pointers (0-based), n_vars+1
    int64_t jac_lo;     // first Jacobian value owned
    int64_t hess_lo;    // first Hessian value owned
    int64_t grad_lo;    // first gradient entry owned (= kn_lo*z)
    // Hessian entries in global-variable columns (the tail of the CSC order; only host-evaluated Global* terms have any)
    const int64_t* tail_colptr;  // device [gd+1]
    const int64_t* tail_rows;    // device, 0-based global row indices, ascending per column
    int64_t tail_lo;             // local position of the tail's first value in this handle's slab, -1: not owned
};

// position of entry (global row R, global-variable column j) in the local Hessian slab, -1 if absent / not owned
__host__ __device__ inline int64_t hess_pos_tail(const KProb& P, int64_t R, int j) {
    if (P.tail_lo < 0) return -1;
    int64_t lo = P.tail_colptr[j], hi = P.tail_colptr[j + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (P.tail_rows[mid] < R) lo = mid + 1; else hi = mid;
    }
    return (lo < P.tail_colptr[j + 1] && P.tail_rows[lo] == R) ? P.tail_lo + lo : -1;
}

// One BilinearIntegrator (src/integrators/bilinear_integrator.jl:61-85) on the device.
struct KBil {
    int32_t n, m, npad;
    int32_t x_off, u_off;
    int32_t pre;          // rows of earlier integrators per interval
    int64_t row_off;      // 0-based global row offset of the integrator (evaluator.jl:213-217)
    int64_t lrow_off;     // offset of its rows inside the shard-local constraint buffer
    const double* G;      // (m+1) padded npad x npad generators, column-major
    const double* GT;     // their transposes
};

struct KDer {  // DerivativeIntegrator (derivative_integrator.jl:26-49)
    int32_t d, x_off, xdot_off, pre;
    int64_t row_off, lrow_off;
};

// Positions inside the shard-local value slabs.  The layout is stated in dto_slab_layout.h; its functions read N, K, z, D of whatever
// they are handed, and the kernels hand them their KProb, so no field is loaded that was not loaded before.
// Jacobian entry (row r of integrator block, column `comp` of knot kn); part 0 = rows of interval kn-1, part 1 = rows of interval kn.
__host__ __device__ inline int64_t jac_pos(const KProb& P, const int64_t* colptr, int64_t kn, int comp,
                                           int pre, int d_i, int part, int r) {
    const int cnt = jac_knot_cnt(P, kn);
    return colptr[kn * P.z + comp] + jac_part_off_cnt(cnt, kn, pre, d_i, part) + r - P.jac_lo;
}

// Hessian entry (row a of knot kn-1, column b of knot kn) of the off-diagonal block, kn >= 1.  This is hess_inner_col_pos of
// dto_slab_layout.h spelled out: as a forward to it, k_extint_hess adds the two halves of its last address in the other order
// (DESIGN 3.1).  tests/test_slab_layout_header.py holds the two together.
__host__ __device__ inline int64_t hess_pos_off(const KProb& P, int64_t kn, int a, int b) {
    const int64_t z = P.z;
    const int64_t tri = z * (z + 1) / 2;
    return tri + (kn - 1) * (z * z + tri) + (int64_t)b * z + (int64_t)b * (b + 1) / 2 + a - P.hess_lo;
}
// upper-triangular Hessian entry (a <= b, knot-local comps) of diagonal block kn
__host__ __device__ inline int64_t hess_pos(const KProb& P, int64_t kn, int a, int b) {
    return hess_diag_pos(P, kn, b) + a - P.hess_lo;
}

// ------------------------------------------------------------------ launch wrappers (dto_kernels.hip)
struct ChainWork {   // per-chunk workspace of the propagator chain: C matrices npad x npad each
    double* W[9];    // A, A2, A3, A4, then Y+Pa / squaring ping, K / polynomial / squaring pong, Y+Pb, L, R
    double* norms;   // [C][4]
    double* colsum;  // [3][C][npad][npad/64] column abs-sums of A^2..A^4 per 64-row chunk (basis path; added in fixed order)
    double* coef;    // [C][COEF_STRIDE]
    int32_t* s;      // [C] squarings per interval (of the evaluation form in use)
    int32_t* s3;     // [C] squarings per interval with the three-product form
    int32_t* smax;   // [0] max, [1] sum of s over the chunk for the two-product form, [4], [5] for the three-product form
                     // (read back by the host, which then picks the form; [2..3] hold d2max)
    unsigned long long* d2max;  // bit pattern of max_k ||A_k^2||_1^(1/2) over the chunk (exact; plans the sweep)
};

void launch_build_A(hipStream_t st, const KProb& P, const KBil& B, const double* dZ, int64_t int0, int nb, double* A);
void launch_bgemm_plain(hipStream_t st, int npad, int nb, const double* A, const double* Bm, double* C);
void launch_norm1(hipStream_t st, int npad, int nb, const ChainWork& w);
// 1-norm of matrix `which` only; also folds max_k sqrt(norm) into w.d2max (used when the chain is not run)
void launch_norm1_one(hipStream_t st, int npad, int nb, const ChainWork& w, int which);
void launch_expm_params(hipStream_t st, int nb, int s_cap, const ChainWork& w);
// Coefficient table (and w.s) for the evaluation form: 2 = two products (degree 16), 3 = three products (order 26),
// 0 = decided ON THE DEVICE from the squaring counts k_expm_params left in w.smax (three products when they save more than
// 1.5 squarings per interval); the form taken lands in w.smax[6] for the host's readback.
void launch_expm_coef(hipStream_t st, int nb, const ChainWork& w, int form);
void launch_poly_h3(hipStream_t st, int npad, int nb, const ChainWork& w);
// where exp(A_k) of the intervals that need no squaring goes: the x_k columns of the Jacobian slab
struct SlabDest {
    KProb P;
    KBil B;
    int64_t int0;
    double* vals;
};
// W[dst] = W[srcA] W[srcB] + poly(coef_base);  dst2 >= 0: also W[dst2] = W[srcA] W[srcB] + poly(coef_base2);
// with_srcA: each polynomial has a sixth coefficient, the weight of W[srcA] itself;
// slab (single-output form, the LAST polynomial product): intervals with s_k = 0 store -result into the Jacobian slab
void launch_bgemm_poly(hipStream_t st, int npad, int nb, const ChainWork& w, int srcA, int srcB, int dst, int coef_base,
                       int dst2, int coef_base2, bool with_srcA = false, const SlabDest* slab = nullptr);
void launch_bgemm_square(hipStream_t st, int npad, int nb, const ChainWork& w, int src, int dst, int it,
                         const KProb& P, const KBil& B, int64_t int0, double* vals);

// ---- the whole propagator chain of a 33..64-state integrator in ONE launch (dto_chain64.hip): a workgroup per interval keeps
// A .. A^4, the polynomial factors and the squarings in LDS and registers, chooses the evaluation form per interval and stores
// -E_k into the slab; norms [n_int][4] (INF, ||A^2||, ||A^3||, ||A^4||: k_hump's input), smax[0] = largest squaring count,
// d2max = max_k min(d2, max(d3, d4)) (bit pattern), sk [n_int] squarings used
hipError_t chain64_prepare();
hipError_t launch_chain64(hipStream_t st, const KProb& P, const KBil& B, const double* dZ, double* vals, double* norms, int32_t* smax,
                          unsigned long long* d2max, int32_t* sk, int s_cap, int force_form, int n_cu);

struct SweepBuf {      // generator sweep ("expmv") workspace for one bilinear integrator
    int32_t npad, Kpad, TN;   // Kpad multiple of TN
    double* Z[2];      // [T][Kpad][npad] ping-pong terms
    double* S;         // [T][Kpad][npad] sums
    double* GY;        // [Kpad][npad]   G(u) * S0
    double* W;         // [(m+1)][Kpad][npad]  G_j' mu   (Hessian)
    double* scaleA;    // [(m+1)][Kpad]  dt*ubar_j/q
    double* scaleU;    // [(m+1)][Kpad]  ubar_j
    double* scaleE;    // [2][Kpad]      dt/q and 2*dt/q (the i == j second-order terms)
    unsigned long long* termnorm;  // [3][T][Kpad]
    unsigned long long* sumnorm;   // [T][Kpad]
    int32_t* active;   // [Kpad/TN]
    int32_t* stats;    // [0] active blocks after the last check, [1] terms used (max)
    // term store (Hessian pairing path): every Taylor term of the sweep is kept, [dcap][T][Kpad][npad]
    double* Zt;
    int32_t dcap, T_alloc;  // T_alloc: column types the Z/S buffers were sized for
    int32_t* nterms;   // [Kpad/TN] number of valid terms of a converged column block (0: use all launched)
    // option reuse_forward_sweep: the Taylor terms of the p column kept by an earlier callback at the same point
    // ([dcap][Kpad][npad] at the head of Zt) let a later sweep run its tangent columns alone (types first_type..T-1)
    int32_t* nterms_p;       // [Kpad/TN] valid stored p terms per column block (0: all frozen_total)
    const double* frozen;    // stored p terms (nullptr: the sweep computes its own p column)
    int32_t frozen_total;    // terms 0 .. frozen_total-1 were stored
    int32_t first_type;      // first column type the sweep computes (1 with frozen p terms, else 0)
    int32_t nblk;            // intervals per entry of nterms / nterms_p (the last sweep's convergence blocks: TN for the
                             // step-per-launch form, the workgroup's interval count for the fused form)
};

// src_kind: 0 = state x_k of the integrator (forward sweep), 1 = multipliers mu_k (adjoint sweep)
void launch_sweep_init(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& w, const SweepTypes& ty,
                       const double* dZ, const double* dmu, int src_kind, int q);
void launch_sweep_restart(hipStream_t st, const SweepBuf& w, int T);
// term 0 (and sum) of column type `type` := v[kn*z + x_off + :]  (a second start vector, Z layout): exp(A) v rides
// along the same sweep as an extra column type
void launch_sweep_set_type(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& w, int T, int type, const double* v);
// matrix-free Jacobian-vector products (evaluator.jl:406-456 without materialising J)
//   Jw:  y[rows of the integrator] = -exp(A)w_x - sum_j c_j w_uj - G(u)y w_dt + w_x(k+1)   (type_ew = column type of exp(A) w_x)
//   Jtw: y[knot entries] += -exp(A')w_k (+ w_{k-1}), -c_j'w_k, -(G(u)y)'w_k                 (ad.S[0] = exp(A') w_k)
void launch_jv_bilinear(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& fw, int type_ew, const double* w, double* y);
void launch_jtv_bilinear(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& fw, const SweepBuf& ad, const double* w, double* y);
void launch_jv_derivative(hipStream_t st, const KProb& P, const KDer& D, const double* dZ, const double* w, double* y, int transpose);

// ---- the whole sweep in one persistent launch (dto_sweep_fused.hip): a workgroup owns `ipw` intervals, all rows, all types
// (FusedSweepPlan and sweep_fused_plan: dto_sweep_plan.h)
hipError_t sweep_fused_prepare();  // per-device opt-in to the kernels' dynamic LDS (dto_create)
// Runs q rounds of at most d_ub Taylor steps (termination test from step tc on, per workgroup), terms into w.Zt (store) or
// ping-pong w.Z[0/1], sums into w.S, scale factors into w.scale*, valid term counts into w.nterms[workgroup],
// w.stats[0] += workgroups that did not converge, w.stats[1] = max terms used (the caller zeroes w.stats).
hipError_t launch_sweep_fused(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& w, const SweepTypes& ty,
                              const FusedSweepPlan& pl, const double* dZ, const double* dmu, int src_kind, int transposed,
                              int q, int d_ub, int tc, bool store, double tol, const int32_t* plan_dev = nullptr);
// {q, d_ub, tc} of a sweep from the norm bound (bit pattern in bounds[0]), computed on the device by device_plan (dto_sweep_plan.h) with
// the host's theta_v: launch_sweep_fused(..., plan_dev)
void launch_plan_dev(hipStream_t st, const unsigned long long* bounds, int32_t* out);

// ---- the same sweep with the rows of the matrix split over a cluster of R workgroups that exchange their slices of every new
// term through global memory (dto_sweep_fused.hip): short shards, single-column sweeps, 512+ states
// (ClusterSweepPlan, sweep_cluster_plan and sweep_cluster_workspace_doubles: dto_sweep_plan.h)
hipError_t sweep_cluster_prepare();
hipError_t launch_sweep_cluster(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& w, const SweepTypes& ty,
                                const ClusterSweepPlan& pl, double* X, unsigned* arrive, const double* dZ, const double* dmu,
                                int src_kind, int transposed, int q, int d_ub, int tc, bool store, double tol);

// ---- the sweep with the generators STATIONARY in registers (dto_sweep_gs.hip, round 4): a cluster of npad / 32 workgroups shares an
// interval group, each member holding 32 rows of every generator for the whole launch; only the term slices move (through the
// sweep's own term slabs, sc1 on both sides).  128 and 256 states, at most 4 drives, no sub-stepping (q = 1).
// (GsSweepPlan, sweep_gs_plan and sweep_gs_norm_doubles, the exchange slab of the partial column norms: dto_sweep_plan.h)
hipError_t sweep_gs_prepare();
// arrive: n_groups (rounded up to 4) counters, zeroed by the launch; terms into w.Zt (store) or ping-pong w.Z[0/1], sums into w.S,
// valid term counts into w.nterms[group], w.stats as launch_sweep_fused
hipError_t launch_sweep_gs(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& w, const SweepTypes& ty, const GsSweepPlan& pl,
                           double* Xn, unsigned* arrive, const double* dZ, const double* dmu, int src_kind, int transposed, int d_ub,
                           int tc, bool store, double tol);

void launch_sweep_step(hipStream_t st, const KBil& B, const SweepBuf& w, const SweepTypes& ty, int transposed,
                       int t, int in_buf, int split_store = 0);
void launch_sweep_check(hipStream_t st, const SweepBuf& w, int T, int t, double tol);
// start of a sweep over types first_type..T-1 only: their terms, sums and norms are cleared, type 0 keeps its sums
void launch_sweep_init_tangents(hipStream_t st, const SweepBuf& w, int T);
// out[j] = G_j (or G_j') * V for every generator j (no summation): out [(m+1)][Kpad][npad]
void launch_apply_generators(hipStream_t st, const KBil& B, const SweepBuf& w, int transposed, const double* V,
                             double* out);
// out[g] = G_{gen_first+g} * V over `cols` columns (cols multiple of the sweep tile): the pairing path's E_j * terms
void launch_apply_generators_cols(hipStream_t st, const KBil& B, const SweepBuf& w, int transposed, const double* V,
                                  double* out, int gen_first, int gen_count, int64_t cols, int64_t seg_cols = 0,
                                  int64_t seg_stride = 0);
// U[a][type][k][:] = sum_b Btab[a][b] * terms[b][type][k][:]   (Beta-function weights of the pairing formula)
void launch_pair_combine(hipStream_t st, const SweepBuf& ad, int T, int n_types, int nf_used, int na_used,
                         const int32_t* nterms_f, int nblk_f, const double* Btab, double* U);
// (u_i,u_j) block of the bilinear Hessian from the pairing formula (see k_hess_pair)
void launch_hess_pair(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& fw, int nf_used, const double* EP,
                      double* H);
// GY = sum_j ubar_j G_j (or G_j') * V
void launch_apply_Gu(hipStream_t st, const KBil& B, const SweepBuf& w, int transposed, const double* V, double* out);

void launch_cons_bilinear(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& w, const double* dZ, double* g);
void launch_cons_derivative(hipStream_t st, const KProb& P, const KDer& Dv, const double* dZ, double* g);
void launch_jac_bilinear(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& w, double* vals);
void launch_jac_derivative(hipStream_t st, const KProb& P, const KDer& Dv, const double* dZ, double* vals);

struct KCon {  // NonlinearKnotPointConstraint with a built-in g
    int32_t kind, n_comps;
    double c;
    const int32_t* comps;    // device [n_comps]
    const int64_t* times;    // device, owned 0-based knots [n_times]
    const int64_t* lrow;     // device, local row of each owned time in the shard-local g buffer
    const int64_t* jpos;     // device [n_times][n_comps] local Jacobian positions (-1: not in pattern)
    int64_t n_times;
    int64_t mu_off;          // global 0-based row of the constraint's first row (for mu), evaluator.jl:219-223
    const int64_t* tidx;     // device, index of each owned time inside the constraint's full `times`
    const int32_t* hess_on;  // device, 0 where a LATER entry of `times` names the same knot: the reference's
                             // ForwardDiff.hessian! into the block view overwrites (knot_point_constraint.jl:285-291)
    int32_t g_dim, external; // outputs per listed time (1 for the built-in kinds); external: values come from the host
    int32_t repeats, comp_repeats;  // the owned `times` name a knot twice / `comps` name a component twice (J' w then adds in listing order)
    const double* M;         // device, QUADFORM_MINUS_C (kind 5): the symmetric n_comps x n_comps matrix, column-major
};
void launch_cons_knot(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, double* g);
void launch_jv_knot(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, const double* w, double* y, int transpose);
void launch_jac_knot(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, double* vals);
void launch_hess_knot(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, const double* dmu, double* H);
// kind 5, g(v) = v' M v - c (dto_quadform.hip): the four launchers above hand such a constraint to these
void launch_qf_cons(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, double* g);
void launch_qf_jac(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, double* vals);
void launch_qf_jv(hipStream_t st, const KProb& P, const KCon& C, const double* dZ, const double* w, double* y, int transpose);
void launch_qf_hess(hipStream_t st, const KProb& P, const KCon& C, const double* dmu, double* H);

// host-evaluated integrator (DTO_INTEGRATOR_EXTERNAL): placement of the caller's per-interval blocks
struct KExtInt {
    int32_t d, pre;        // rows per interval; rows of the integrators before it (per interval)
    int64_t row_off, lrow_off;
};
void launch_extint_cons(hipStream_t st, const KProb& P, const KExtInt& E, const double* vals, double* g);
void launch_extint_jac(hipStream_t st, const KProb& P, const KExtInt& E, const double* blocks, double* vals);
void launch_extint_hess(hipStream_t st, const KProb& P, const KExtInt& E, const double* blocks, double* H);

// TimeDependentBilinearIntegrator with a parametrised generator family, evaluated on the device (dto_tdb.hip): fills the same
// per-interval blocks as a host-evaluated integrator, which k_extint_* then place
struct KTdb {
    int32_t n, m, x_off, u_off, t_off, order, substeps, nmod;
    int64_t row_off;             // 0-based global row offset of the integrator (for mu)
    const double* G;             // (m+1) compact n x n matrices, column-major
    const double* H;             // [nmod][(m+1)] compact n x n matrices
    const int32_t* mod_kind;     // [nmod] 1 = cos(omega t), 2 = sin(omega t)
    const double* mod_omega;     // [nmod]
};
bool tdb_supported(const KTdb& T);
size_t tdb_scratch_doubles(const KTdb& T, int need);
// blocks of intervals i_lo .. i_lo + count - 1 (global, 0-based) into vals [K][n], jac [K][2z][n], hess [K][2z][2z]
hipError_t launch_tdb(hipStream_t st, const KProb& P, const KTdb& T, const double* dZ, const double* dmu, int need, int64_t i_lo,
                      int64_t count, double* vals, double* jac, double* hess, double* scratch, size_t scratch_stride);
// Product modes of the same integrator, no block and no slab: need 3 assigns the integrator's rows of J w in `out` = y; need 4 stages
// per interval [Phi_k' w_k (n), w_k' (dPhi_k / dtheta_b) x_k (p)] in `out` = [K][n + p], which launch_tdb_jtv_place (either
// kernel's staging) then ADDS into y, every entry by one thread.  All K intervals (products need an unsharded handle).
// tdb_scratch_doubles covers need 3 and 4; tdb_product_flops: flops of one interval as executed.
double tdb_product_flops(const KTdb& T, int need);
hipError_t launch_tdb_product(hipStream_t st, const KProb& P, const KTdb& T, const double* dZ, const double* dw, int need, double* out,
                              double* scratch, size_t scratch_stride);
hipError_t launch_tdb_jtv_place(hipStream_t st, const KProb& P, const KTdb& T, const double* dw, const double* stage, double* dy);
// The same integrator at 65..256 states (dto_tdb_mfma.hip): FP64 MFMA products against M0 = sum_q c_q B_q, the derivative jets
// applied as scalar combinations of B_q y; a persistent grid of `resident` workgroups, one scratch slot of `scratch_stride` doubles
// each.  Bp / BpT: the Q = (m+1)(1+nmod) matrices G_j, H_cj (q = j (1 + nmod) + c) and their transposes, zero-padded to
// tdb_mfma_npad(n) rows and columns, column-major.  tdb_mfma_refusal: nullptr, or which limit of the device kernels (either of
// them: 1..256 states, substeps, coefficient table) a description exceeds.
// One launch evaluates `G.count` integrators of one system (1 .. TDB_SHARE_MAX; more than one under DTO_FLAG_SHARED_GENERATORS):
// members that differ in their state component and rows only, with every M0, coefficient table and (Jacobian) the Phi block formed
// once.  T is any member's description; each member's blocks go to its own vals / jac / hess, bit for bit what a launch of that
// member alone writes.  need 0 .. 2.  tdb_mfma_scratch_doubles: the slot of one workgroup; tdb_mfma_flops: flops of one interval as
// executed; both for a launch of `members`, and at one member also for the product modes.
constexpr int TDB_SHARE_MAX = 8;
struct KTdbMember {
    int32_t x_off;
    int64_t row_off;
    double *vals, *jac, *hess;
};
struct KTdbGroup {
    int32_t count;
    KTdbMember m[TDB_SHARE_MAX];
};
int tdb_mfma_npad(int n);
const char* tdb_mfma_refusal(const KTdb& T);
bool tdb_mfma_supported(const KTdb& T);
size_t tdb_mfma_scratch_doubles(const KTdb& T, int need, int members = 1);
double tdb_mfma_flops(const KTdb& T, int need, int members = 1);
hipError_t launch_tdb_mfma(hipStream_t st, const KProb& P, const KTdb& T, const KTdbGroup& G, const double* Bp, const double* BpT,
                           const double* dZ, const double* dmu, int need, int64_t i_lo, int64_t count, double* scratch,
                           size_t scratch_stride, int resident);
// ... and the product modes of one integrator (need 3 / 4, `out` as launch_tdb_product's)
hipError_t launch_tdb_mfma_product(hipStream_t st, const KProb& P, const KTdb& T, const double* Bp, const double* BpT, const double* dZ,
                                   const double* dw, int need, double* out, double* scratch, size_t scratch_stride, int resident);

// BilinearIntegrator with replicated-block generators G_j = I_r (x) B_j (dto_kron.hip): one workgroup per interval sweeps b-row
// column groups against the b x b blocks and writes defect, Jacobian block or Hessian block of mu_k' f straight to their positions
struct KKron {
    int32_t b, r;        // finest structure found (what dto_integrator_blocks reports)
    int32_t bw, rw, bp;  // working block (a few finest blocks grouped while they fit 16 rows), its replicas, bw padded to 16
    const double* Bm;    // (m+1) working blocks (time-dependent family: Q of them), bp x bp column-major, zero-padded
    const double* BmT;   // their transposes
    int32_t* stats;      // [0] += workgroups whose sweep exhausted its budget, [1] = max terms used (the caller zeroes them)
};
hipError_t kron_prepare();
bool kron_supported(const KKron& K, int m, bool hessian);
size_t kron_scratch_doubles(const KKron& K, int m, int need);
// need: 0 defect into g, 1 Jacobian block into vals (and the identity of the z_{k+1} half), 2 Hessian block added into H,
// 3 the integrator's rows of J w into g (dmu = w), 4 its part of J' w added into g (dmu = w, g zero-filled by the caller)
hipError_t launch_kron(hipStream_t st, const KProb& P, const KBil& B, const KKron& K, const double* dZ, const double* dmu, int need,
                       double* g, double* vals, double* H, double* scratch, size_t stride);

// TimeDependentBilinearIntegrator whose G_j and H_cj are all I_r (x) B_q (dto_tdb_kron.hip): k_tdb_mfma's discrete map on b x b
// blocks, into the same staged blocks.  K.Bm / K.BmT hold the Q = (m+1)(1+nmod) working blocks (q = j (1 + nmod) + c) and their
// transposes; K.stats is unused.  `need` and the interval range as launch_tdb_mfma; the kernel assigns only the entries it owns
// (the caller zero-fills jac and hess once).  tdb_kron_supported: every condition of the path that the description and the blocks
// decide (32 < n <= 512, r >= 2, b <= 64, substeps, coefficient table).  tdb_kron_flops: flops of one interval as executed.
bool tdb_kron_supported(const KTdb& T, const KKron& K);
size_t tdb_kron_scratch_doubles(const KTdb& T, const KKron& K, int need);
double tdb_kron_flops(const KTdb& T, const KKron& K, int need);
hipError_t launch_tdb_kron(hipStream_t st, const KProb& P, const KTdb& T, const KKron& K, const double* dZ, const double* dmu, int need,
                           int64_t i_lo, int64_t count, double* vals, double* jac, double* hess, double* scratch, size_t scratch_stride,
                           int resident);
// ... and its product modes (k_tdb_kron_product; need 3 / 4, `out` as launch_tdb_product's, all K intervals): no Phi~, no block, no
// slab.  tdb_kron_scratch_doubles and tdb_kron_flops cover need 3 and 4 as well; the J' w staging goes through launch_tdb_jtv_place.
hipError_t launch_tdb_kron_product(hipStream_t st, const KProb& P, const KTdb& T, const KKron& K, const double* dZ, const double* dw, int need,
                                   double* out, double* scratch, size_t scratch_stride, int resident);

// host-evaluated knot terms (DTO_CONSTRAINT_EXTERNAL / DTO_OBJECTIVE_EXTERNAL_KNOT): scatter of caller-supplied blocks
void launch_ext_cons(hipStream_t st, const KCon& C, const double* vals, double* g);
void launch_ext_jac(hipStream_t st, const KCon& C, const double* blocks, double* vals);
// One host-evaluated term's placement data: per listing i the variables [z_t[comps] ; global_data[gcomps]]
// (times[i] == N: no knot part).  `knot_on` / `glob_on`: this handle places the listing's knot part / its entries in
// global-variable columns; `count`: this handle adds the listing's value to the objective.
struct KExtTerm {
    int32_t nc, ng;
    const int32_t* comps;    // device [nc]
    const int32_t* gcomps;   // device [ng]
    const int64_t* times;    // device [n_list] 0-based knots
    const int64_t* tidx;     // device [n_list] index of the listing in the caller's arrays
    const int32_t* knot_on;  // device [n_list]
    const int32_t* count;    // device [n_list]
    int32_t glob_on, pad;
    int64_t n_list;
};
void launch_ext_hess(hipStream_t st, const KProb& P, const KExtTerm& E, double scale, const double* blocks, double* H);
void launch_ext_objective(hipStream_t st, const KExtTerm& E, double weight, const double* vals, double* f);
void launch_ext_gradient(hipStream_t st, const KProb& P, const KExtTerm& E, double weight, const double* blocks, double* grad);

struct KObj {  // objective term
    int32_t kind, comp_off, comp_dim, has_baseline;
    double weight, D;
    const double* R;         // device [comp_dim]
    const double* baseline;  // device [comp_dim x N] or null
    const int64_t* times;    // device, owned 0-based knots
    int64_t n_times;
    // KNOT_SQDIST (kind 4): l(v, p) = ||v - p||^2 on a component list, per-time targets and weights
    const int32_t* comps;    // device [n_comps]
    int32_t n_comps, pad1;
    const double* params;    // device [n_times][n_comps] (owned times) or null
    const double* Qs;        // device [n_times]
    const int32_t* last;     // device [n_times]: 0 where a later listed time names the same knot -- the reference's
                             // gradient!/hessian! overwrite per listed time (knot_point_objectives.jl:198, 235)
};
void launch_objective(hipStream_t st, const KProb& P, const KObj& O, const double* dZ, double* partial, double* f);
void launch_gradient(hipStream_t st, const KProb& P, const KObj& O, const double* dZ, double* grad);
void launch_hess_objective(hipStream_t st, const KProb& P, const KObj& O, const double* dZ, double sigma, double* H);
void launch_hess_derivative(hipStream_t st, const KProb& P, const KDer& Dv, const double* dmu, double* H);
void launch_hess_bilinear(hipStream_t st, const KProb& P, const KBil& B, const SweepBuf& fw, const SweepBuf& ad,
                          const double* dmu, double* H, int with_uu);

// DTO_FLAG_SHARED_GENERATORS (dto_share.hip): the -E_k blocks of intervals int0 .. int0 + nb - 1 (global, 0-based), n x n each, are
// copied from the leader's positions in the Jacobian slab ([0]) to the followers' ([1 .. nf]); x_off / pre as in KBil
constexpr int SHARE_MAX_FOLLOWERS = 15;
struct KShare {
    int32_t n, nf;
    int32_t x_off[1 + SHARE_MAX_FOLLOWERS];
    int32_t pre[1 + SHARE_MAX_FOLLOWERS];
};
void launch_share_E(hipStream_t st, const KProb& P, const KShare& S, int64_t int0, int nb, double* vals);

// Open-loop rollout X_{k+1} = E_k X_k of one integrator (dto_rollout.hip; index plan: dto_rollout_plan.h).  The -E_k blocks are read
// from the x_k columns of a Jacobian value slab (x_off / pre as in KBil, KExtInt), the product tree holds 2^(L+1) - 1 matrices of
// npad x npad, the padded trajectory S is [K + 1][col_pad][npad].
struct KRollout {
    int32_t n, npad, x_off, pre;
    int32_t n_cols, col_pad;
    int32_t L;      // tree levels: 2^L >= K
    int64_t K;      // intervals
    KRollout() = default;
    KRollout(int32_t n_, int32_t x_off_, int32_t pre_, int32_t n_cols_, int64_t K_)
        : n(n_), npad((n_ + 63) / 64 * 64), x_off(x_off_), pre(pre_), n_cols(n_cols_), col_pad(rollout_col_pad(n_cols_)),
          L(rollout_levels(K_ > 1 ? K_ : 1)), K(K_) {}
};
void launch_rollout_leaves(hipStream_t st, const KProb& P, const KRollout& R, const double* vals, double* tree);
void launch_rollout_start(hipStream_t st, const KRollout& R, const double* dZ, const double* X0, double* S);
// level l of the descent (L + 1: the root's item, then L .. 1); only >= 0: that item alone
void launch_rollout_descend(hipStream_t st, const KRollout& R, int l, int64_t only, const double* tree, double* S);
void launch_rollout_compact(hipStream_t st, const KRollout& R, int64_t k0, int64_t nk, const double* S, double* X);

// Solves with the dynamics block, Y_{k+1} = E_k Y_k + B_{k+1} or (adjoint) Lam_k = E_k' Lam_{k+1} + B_k (dto_dynsolve.hip; index plan:
// dto_rollout_plan.h): affine scans over the rollout's tree and an offset tree `off` of 2^(L+1) - 1 blocks [col_pad][npad].
// B: [K + 1][n_cols][n], the caller's layout
void launch_dynsolve_load(hipStream_t st, const KRollout& R, int adjoint, const double* B, double* off, double* S);
// level l of the offsets into level l + 1, l = 0 .. L - 1
void launch_dynsolve_up(hipStream_t st, const KRollout& R, int adjoint, int l, const double* tree, double* off);
// level l of the descent (L + 1: the root's item, then L .. 1); only >= 0: that item alone
void launch_dynsolve_descend(hipStream_t st, const KRollout& R, int adjoint, int l, int64_t only, const double* tree, double* off, double* S);

// Whole-dynamics solves (dto_elim.hip; plan and the coupling store's layout: dto_elim_plan.h).
struct KElimPair {   // the coupling blocks of integrator a in the state columns of its dependency b
    int32_t n_a, pre_a, x_off_b, n_b;
    int32_t col, width;   // first column of S_b inside a's W_a columns, and W_a
};
struct KElimTerm {   // one contraction of k_elim_couple: a store and the slice of the result it meets
    int64_t store;               // first double of the store read (C_a forward, C_b of a dependent b adjoint)
    int32_t width, n_rows, col;  // that store's W and rows, and the first column read
    int32_t off, n;              // the other integrator's slice [off, off + n) of the D axis
};
struct KElimCouple {
    int32_t n_a, pre_a, D, n_cols, n_terms;
    int64_t K;
    const KElimTerm* terms;   // device
};
void launch_elim_gather(hipStream_t st, const KProb& P, const KElimPair& G, int64_t K, const double* vals, double* store);
// Bp [K + 1][n_cols][n_a] from B and the finished slices of Y, both [K + 1][n_cols][D]
void launch_elim_couple(hipStream_t st, const KElimCouple& C, int adjoint, const double* store, const double* B, const double* Y, double* Bp);
// the block solve of a DerivativeIntegrator into its slice [pre, pre + n) of Y
void launch_deriv_scan(hipStream_t st, int64_t K, int n, int n_cols, int D, int pre, int adjoint, const double* Bp, double* Y);
void launch_elim_collect(hipStream_t st, int64_t N, int n, int n_cols, int D, int pre, const double* Yp, double* Y);

// Reduced-space operators (dto_reduced.hip; index plan: dto_reduced_plan.h): the packers between the Z layout (n_vars), the
// constraint rows (n_cons) and the solves' [N][1][D].  R's tables are device pointers.
// g = sigma * gf (+ t, nullable) [n_vars]; gS: its state entries as [N][1][D]
void launch_red_gradient(hipStream_t st, const KReduced& R, double sigma, const double* gf, const double* t, double* g, double* gS);
// w [n_cons]: lam_{k+1} (nullable: 0) in the dynamics rows of interval k, mu (w_takes_mu, mu not null) or 0 in the other rows;
// mut [n_cons] (nullable): -lam_{k+1} in the dynamics rows, mu (null: 0) in the other rows
void launch_red_multipliers(hipStream_t st, const KReduced& R, const double* lam, const double* mu, int w_takes_mu, double* w, double* mut);
void launch_red_vhat(hipStream_t st, const KReduced& R, const double* v, double* vh);                                  // states zeroed
void launch_red_rhs(hipStream_t st, const KReduced& R, const double* v, const double* rho, double* B);                 // [v_S0 ; -rho_dyn]
void launch_red_zhat(hipStream_t st, const KReduced& R, const double* v, const double* Y, double* zh);                 // states <- Y
void launch_red_gather(hipStream_t st, const KReduced& R, const double* q, double* qS);                                // states of q
void launch_red_finish(hipStream_t st, const KReduced& R, const double* q, const double* t, const double* lam, double* y);
// Block forms for w columns (dto_projected_hessian_products[_dev]).  Two layouts: PLANES [w][n] (column j at j * n: the caller's V and
// Y, z^, q and the vectors J v^ and J' w take one at a time) and the solves' [N][w][D].  One thread per output entry, the arithmetic
// of the single forms.
void launch_red_vhat_block(hipStream_t st, const KReduced& R, int w, const double* v, double* vh);                      // planes -> planes
void launch_red_rhs_block(hipStream_t st, const KReduced& R, int w, const double* v, const double* rho, double* B);     // planes, planes [w][n_cons] -> [N][w][D]
void launch_red_zhat_block(hipStream_t st, const KReduced& R, int w, const double* v, const double* Y, double* zh);     // planes, [N][w][D] -> planes
void launch_red_gather_block(hipStream_t st, const KReduced& R, int w, const double* q, double* qS);                    // planes -> [N][w][D]
void launch_red_multipliers_block(hipStream_t st, const KReduced& R, int w, const double* lam, double* wv);             // [N][w][D] -> planes [w][n_cons]
void launch_red_finish_block(hipStream_t st, const KReduced& R, int w, const double* q, const double* t, const double* lam, double* y);  // planes, planes, [N][w][D] -> planes

// Input-block store of the reduced-space operators (option "reduced_input_store"; dto_reduced.hip; plan and layout: dto_input_plan.h).
struct KInputInt {   // one integrator: its store F_a [K][2][wf][n] and its free inputs fin[fin0 .. fin0 + wf)
    int64_t store;
    int32_t pre, n, wf, fin0;
};
struct KInputTerm {   // one reader of a knot component: column j of F_a, the rows [pre, pre + n) of the D axis
    int64_t store;
    int32_t wf, n, j, pre;
};
struct KInput {   // every table is a device pointer
    const KInputInt* integ;    // [n_int]
    const int32_t* fin;        // [sum of wf]
    const int32_t* pos_int;    // [D] the integrator that owns a D position
    const int32_t* term0;      // [z + 1] a component's terms are terms[term0[c] .. term0[c + 1])
    const KInputTerm* terms;
    const int32_t* read;       // [n_read] the components with terms, ascending
    int32_t n_read, n_int;
    int64_t K;
};
// F_a of integrator a from the Jacobian value slab
void launch_red_input_gather(hipStream_t st, const KProb& P, const KInput& In, int a, const double* vals, double* store);
// B [N][1][D]: knot 0 the knot-1 state entries of v, knot k >= 1 minus the input blocks of interval k - 1 times the free inputs of v
void launch_red_input_forward(hipStream_t st, const KReduced& R, const KInput& In, const double* store, const double* v, double* B);
// y [n_vars]: q - F' Gam on the read components, q on the unread ones and the globals, Gam_0 on the states of knot 0, 0 on the dependent entries
void launch_red_input_transposed(hipStream_t st, const KReduced& R, const KInput& In, const double* store, const double* q, const double* gam,
                                 double* y);
// the two products for w columns: v, q and y PLANES, B and gam [N][w][D]; per column the sums of the single forms in their order
void launch_red_input_forward_block(hipStream_t st, const KReduced& R, const KInput& In, int w, const double* store, const double* v, double* B);
void launch_red_input_transposed_block(hipStream_t st, const KReduced& R, const KInput& In, int w, const double* store, const double* q,
                                       const double* gam, double* y);

// Feasible-trajectory rollout and reduced merit value (dto_feasible.hip; schedule: dto_feasible_plan.h).  Zf is a Z-layout vector
// [N][z] (+ globals) that the kernels update in place.
// a DerivativeIntegrator's recurrence x_{k+1} = x_k + dt_k xdot_k over K intervals, product and sum rounded on their own
void launch_feas_deriv(hipStream_t st, int64_t K, int z, int dt_idx, const KDer& D, double* Zf);
// knots 1 .. K of column 0 of the rollout's padded trajectory S into R's state components of Zf
void launch_feas_scatter(hipStream_t st, const KRollout& R, int z, const double* S, double* Zf);
// *phi = sigma * *f + sum over the rows r >= n_dyn of mu[r] g[r], one wavefront in a fixed order; mu null: *phi = sigma * *f
void launch_feas_merit(hipStream_t st, int64_t n_dyn, int64_t n_cons, double sigma, const double* f, const double* mu, const double* g,
                       double* phi);

// Truncated-Newton step (dto_newton.hip; dot order, decision and the layouts of `part` and `state`: dto_newton_plan.h).  All vectors
// [n] in the Z layout; g is the reduced gradient, mask the caller's free mask (null: all free), w holds y = T'HT d on entry to
// launch_newton_curv and w = M (y + shift d) behind it.
struct KNewton {
    int64_t n, nb;             // n_vars, newton_chunks(n_vars)
    double *p, *r, *d, *w;
    const double *g, *mask;
    double *part, *state;      // [NEWTON_SLOTS][nb], [NEWTON_STATE]
    double *info, *trace;      // [8], [max_iter][4] or null
    double radius, shift, rtol, atol;
    int combined;              // 0: every workgroup combines the partial sums itself; 1 (A/B, TUNING builds): launch_newton_combine did
};
// r = M g, p = 0, d = -r, the partial sums of r . r
void launch_newton_start(hipStream_t st, const KReduced& R, const KNewton& A);
// w = M (y + shift d) in place of y, the partial sums of d . w, d . d, p . d, p . p
void launch_newton_curv(hipStream_t st, const KReduced& R, const KNewton& A);
// iteration j >= 1: the decision, p += s d, r += s w, the partial sums behind the update, the first three entries of the trace row
void launch_newton_step(hipStream_t st, const KReduced& R, const KNewton& A, int j);
// j = 0 behind the start, j >= 1 behind the step: rr', the convergence test, d = beta d - r, status and iteration count, `info` on exit
void launch_newton_dir(hipStream_t st, const KNewton& A, int j, int max_iter);
// the A/B form of stage 2: one workgroup combines the slots slot0 .. slot0 + count - 1 (count <= 4) into state[NWS_DOTS ..] for the next launch
void launch_newton_combine(hipStream_t st, const KNewton& A, int slot0, int count);

// Bound-constrained truncated-Newton step (dto_newton_box.hip; the entry rules, the decision, the loop and the layouts of `part` and
// `state`: dto_newton_box_plan.h).  As KNewton; Z the point, lo / hi the bounds (null: none), es the state bytes, zp and es_out the
// optional outputs (null: not written).
struct KNewtonBox {
    int64_t n, nb;
    double *p, *r, *d, *w;
    const double *g, *mask, *Z, *lo, *hi;
    unsigned char* es;         // [n]
    double *part, *state;      // [NEWTON_BOX_SLOTS][nb], [NEWTON_BOX_STATE]
    double *info, *trace;      // [12], [max_iter][6] or null
    double *zp, *es_out;       // [n] or null
    double radius, shift, rtol, atol;
};
// the states, r = g on F0, p = 0, d = -r, the partial sums of r . r and the counts of free and held entries
void launch_newton_box_start(hipStream_t st, const KReduced& R, const KNewtonBox& A);
// w = y + shift d on F0 in place of y, the partial sums of d . w, d . d, p . d, p . p and the chunk's smallest breakpoint
void launch_newton_box_curv(hipStream_t st, const KNewtonBox& A);
// iteration j >= 1: the decision, the update with its clamps, the states, the optional outputs, the partial results behind the update
void launch_newton_box_step(hipStream_t st, const KNewtonBox& A, int j);
// j = 0 behind the start, j >= 1 behind the step: the convergence test, the restart or the beta step, status, counts, `info` on exit
void launch_newton_box_dir(hipStream_t st, const KNewtonBox& A, int j, int max_iter);

// L-BFGS-preconditioned truncated-Newton step (dto_precond.hip; the pair store, the preparation, the application, the loop and the
// layouts of `part`, `state` and `pc`: dto_precond_plan.h).  B as for the box step, with `part` [PRECOND_SLOTS][nb], `state`
// [PRECOND_STATE], info [16] and trace [max_iter][8].  S / Y: the current bank's vectors, a ring of m slots of n doubles with pair k in
// slot (head + k) % m; HS / HY: the other bank (null without harvest).
struct KPrecond {
    KNewtonBox B;
    double* z;                 // [n]
    double *uv, *gram, *pc;    // [2 cnt][nb], [precond_gram_count(cnt)][nb], [PRECOND_PC]
    const double *S, *Y;
    double *HS, *HY;
    int m, head, cnt, harvest;
};
// the entry states of dto_newton_precondition: free where the entry is independent and the mask leaves it, fixed elsewhere
void launch_precond_states(hipStream_t st, const KReduced& R, const KNewtonBox& A);
// the partial sums of the Gram entries over the free entries; then one workgroup: their stage 2, admission, gamma, R and M into pc
void launch_precond_gram(hipStream_t st, const KPrecond& A);
void launch_precond_prep(hipStream_t st, const KPrecond& A);
// the partial sums of s~_k . r_F and y~_k . r_F for every pair
void launch_precond_dots(hipStream_t st, const KPrecond& A, const double* r);
// stage 2 of those, the triangular solves, z and the partial sums of r . z; j: the iteration the application stands behind (0: the start)
void launch_precond_comb(hipStream_t st, const KPrecond& A, const double* r, double* z, int j);
// iteration j >= 1: the box step's launch with rz in the decision, the harvest copy and the multi-dot pass on the new r
void launch_precond_step(hipStream_t st, const KPrecond& A, int j);
// j = 0 behind the start's application, j >= 1 behind that of iteration j: the convergence test, the fallback, d, the counts, `info`
void launch_precond_dir(hipStream_t st, const KPrecond& A, int j, int max_iter);
// dst = src, n doubles
void launch_precond_copy(hipStream_t st, int64_t n, const double* src, double* dst);

// Augmented-Lagrangian terms (dto_auglag.hip; the row rules, the order of the sums and the eight scalars: dto_auglag_plan.h).
struct KAlRows {
    int64_t n_dyn, n_cons;
    const unsigned char* is_eq;      // [n_cons - n_dyn], non-zero: equality row
    const double *g, *mu, *rho;      // [n_cons]; mu null: zeros; the dynamics rows are not read
    double *mu_eff, *weight;         // [n_cons] or null: mult / weight in the non-dynamics rows, 0 in the dynamics rows
    double* info;                    // [AL_INFO] or null
    double sigma;                    // the merit: phi = sigma * f + P where phi is given
    const double* f;
    double* phi;
};
// the row pass: one wavefront over the non-dynamics rows, further workgroups for the zeros of the dynamics rows
void launch_al_rows(hipStream_t st, const KAlRows& A);
// t_j += J_c' (weight .* (J_c z^_j)) for the w columns of one constraint of kind 1 or 2 without repeats; z^ and t planes [w][n_vars]
void launch_al_gn(hipStream_t st, const KProb& P, const KCon& C, int w, int64_t n_vars, const double* dZ, const double* weight, const double* zh,
                  double* t);
// c_r = weight_r * c_r, r < n
void launch_al_scale(hipStream_t st, int64_t n, const double* weight, double* c);
// q = q + t, n entries
void launch_al_add(hipStream_t st, int64_t n, const double* t, double* q);

// Reduced-space minimize (dto_minimize.hip; the rules, the scalars' layout, the history rows and the mailbox: dto_minimize_plan.h).
// One record serves both launches; a launch reads bank_in and writes bank_out, the other bank.
struct KMinimize {
    int64_t n, n_dyn, n_cons;
    double* Z;                        // [n]: the trial launch copies Zt into it where the trial is accepted
    const double* Zt;
    const double* bank_in;            // [MINIMIZE_STATE]
    double* bank_out;
    const double *sinfo, *phi_t;      // the trial: the step's info, the trial point's merit value (one double)
    const double *rinfo, *rinfo0;     // the outer iteration: the row pass's scalars behind the inner loop, and the first pass's
    double *mu, *rho;                 // [n_cons], the outer iteration: mu <- mu_eff and the new rho on the non-dynamics rows
    const double* mu_eff;
    double *row, *mail, *info;        // the history row (or null), the mailbox [4], info [16]
    MinimizeOptions opt;
    MinimizeTrialFlags F;
    int first_outer, last_outer;
};
void launch_minimize_trial(hipStream_t st, const KMinimize& A);
void launch_minimize_outer(hipStream_t st, const KMinimize& A);

void launch_fill(hipStream_t st, double* p, int64_t n, double v);
void launch_zero_runs(hipStream_t st, const int64_t* start, const int64_t* len, int64_t n_runs, double* dst);

// Small-state path (dto_small.hip): one wavefront per interval, everything in LDS.  mode bits: 1 constraint
// values, 2 Jacobian block, 4 Hessian block.  Gs = compact (m+1) x n x n generators.
size_t small_lds_bytes(int n, int m, int T_fw, int T_ad);
hipError_t small_prepare(size_t lds_bytes);  // per-device opt-in to > 64 KB of dynamic LDS (dto_create)
hipError_t launch_small(hipStream_t st, const KProb& P, const KBil& B, const double* Gs, const SweepTypes& ty_fw,
                        const SweepTypes& ty_ad, const double* dZ, const double* dmu, double* cons, double* jac, double* hess,
                        int mode);

// y = J w / y = J' w from the value slab in CSC order (A3: evaluator.jl:406-456; the reference also
// materialises the Jacobian values first, on the host).  One wavefront per column.
struct KIntegTable {
    int32_t n;
    int32_t d[8];
    int64_t off[8];
};
void launch_jac_spmv(hipStream_t st, const KProb& P, const KIntegTable& T, const int64_t* conbase, const int64_t* con_rows,
                     const double* vals, const double* w, double* y, int transpose, int64_t global_cols = 0);
// y = J w from the value slab row by row (fixed summation order; the transpose takes launch_jac_spmv, one wavefront per column)
void launch_jac_rowgather(hipStream_t st, const KProb& P, const KIntegTable& T, int64_t n_con_rows, const int64_t* rptr, const int64_t* rcol,
                          const int64_t* rpos, int64_t n_dyn, const double* vals, const double* w, double* y);
void launch_add(hipStream_t st, double* dst, const double* src, int64_t n);  // dst += src
// *flag = 0 if a and b differ in any bit (flag preset to 1 by the caller)
void launch_bits_equal(hipStream_t st, const double* a, const double* b, int64_t n, int32_t* flag);

// Hessian-vector products (dto_hess_product.hip): y = H v from a row-major copy of both triangles of the Hessian slab.
// Rows are sorted into up to three classes of 4 / 16 / 64 lanes per row; class c owns rows[row0[c] .. row0[c+1]) and the
// blocks [blk0[c], blk0[c+1]) of the launch (256 threads each).  Every row starts at an even entry (an odd-length row is
// followed by one padding entry, which the kernel never adds).
struct KHessProduct {
    const int64_t* start;   // [n_vars] first entry of each row (even)
    const int32_t* len;     // [n_vars] entries of each row
    const int32_t* col;     // [nnz, even]
    const double* val;      // [nnz]
    const int32_t* rows;    // [n_vars] row ids, class by class
    int64_t row0[4], blk0[4];
    int32_t cls_g[3];
    int32_t n_cls;
};
// val[i] = slab[pos[i]] (pos -1: padding, written as 0)
void launch_hess_gather(hipStream_t st, const double* slab, const int64_t* pos, int64_t n, double* val);
void launch_hess_spmv(hipStream_t st, const KHessProduct& p, const double* v, double* y);
// Y = H V for w columns in one launch: entry (i, j) of V at v[i * v_es + j * v_cs], of Y at y[i * y_es + j * y_cs].  Column j of Y has
// the bits of launch_hess_spmv on column j of V.  The kernel is instantiated for tiles of 1, 2, 4 and 8 columns per lane.
struct KHessBlock {
    int32_t w;
    int64_t v_es, v_cs, y_es, y_cs;
};
inline int hess_block_tile(int w) { return w >= 5 ? 8 : w >= 3 ? 4 : w == 2 ? 2 : 1; }
void launch_hess_spmm(hipStream_t st, const KHessProduct& p, const KHessBlock& B, const double* v, double* y);

// Powers of A_k from the generator subspace: A_k = dt*sum_j ubar_j G_j lives in an (m+1)-dimensional
// matrix space, so A_k^r = sum over multisets alpha of size r of (dt^r prod ubar_alpha) * S_alpha with
// S_alpha = sum of the distinct orderings of the product G_alpha1 ... G_alphar, shared by all knots.
// One GEMM  [vec(S_alpha)] (npad^2 x cnt) x coef (cnt x intervals)  then yields A_k^r for every
// interval of the chunk -- 2*npad^2*cnt flops per interval instead of 2*npad^3.
struct BasisSet {
    int32_t r, cnt, cntpad;     // degree, number of multisets, padded to 16
    const double* S;            // device [cntpad][npad^2]
    const int32_t* idx;         // device [cnt][r] generator indices of each multiset (-1 = unused slot)
    double* coef;               // device [capacity][cntpad] per-interval coefficients
};
void launch_basis_coef(hipStream_t st, const KProb& P, const KBil& B, const BasisSet& bs, const double* dZ,
                       int64_t int0, int nb, int nbpad, const double* taylor);
void launch_jac_zero(hipStream_t st, const KProb& P, const KBil& B, double* vals);
// colsum (nullable): [nb][npad] accumulators of the column abs-sums of every output matrix (zeroed by
// the caller); the exact 1-norms then cost no extra pass over the matrices.
void launch_basis_gemm(hipStream_t st, int npad, int nb, int nbpad, const BasisSet& bs, double* out, double* colsum);
// the same for several basis sets in ONE launch (A^2, A^3, A^4): their tiles are interleaved, so the write-bound sets
// (few multisets, short K loop) overlap with the MFMA-bound ones instead of running one after the other
void launch_basis_gemm_multi(hipStream_t st, int npad, int nb, int nbpad, int nsets, const BasisSet* bs, double* const* out,
                             double* const* colsum);
// coefficients of several basis sets in one launch
void launch_basis_coef_multi(hipStream_t st, const KProb& P, const KBil& B, int nsets, const BasisSet* bs, const double* dZ,
                             int64_t int0, int nb, int nbpad);
// norms[b*4 + 1 + r] = max column sum of set r, r < nsets (one launch)
void launch_norm_from_colsum_multi(hipStream_t st, int npad, int nb, int nsets, double* const* colsum, double* norms);
// norms[b*4 + which] = max_c colsum[b][c]
void launch_beta_from_norms(hipStream_t st, int nb, const ChainWork& w);
void launch_hump(hipStream_t st, const KProb& P, const KBil& B, const double* dZ, const double* g1, int64_t int0, int nb,
                 const double* norms, unsigned long long* out);
void launch_norm_from_colsum(hipStream_t st, int npad, int nb, const double* colsum, double* norms, int which,
                             unsigned long long* d2max = nullptr);
// out2[0] = max_k min(b1_k, b2_k), out2[1] = max_k b1_k (bit patterns of non-negative doubles), where
// b1_k >= ||A_k||_1 and b2_k >= ||A_k^2||_1^(1/2) follow from the generator norms g1[j] = ||G_j||_1,
// n2[i][j] = ||G_i G_j||_1 and the triangle inequality.
void launch_norm_bounds(hipStream_t st, const KProb& P, const KBil& B, const double* dZ, const double* g1,
                        const double* n2, unsigned long long* out2);

}  // namespace dto
