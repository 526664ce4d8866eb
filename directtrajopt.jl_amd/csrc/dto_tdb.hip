// dto_tdb.hip -- device propagator of the TimeDependentBilinearIntegrator for a PARAMETRISED generator family
// (reference: src/integrators/time_dependent_bilinear_integrator.jl:60-244).
//
// The reference integrates  dx/dtau = dt_k G(u(tau), t_k + tau dt_k) x  on tau in [0, 1] with an arbitrary Julia closure
// G(u, t) (adaptive Tsit5, differentiated through the solver by ForwardDiff).  A closure cannot cross the C ABI; what can is
// the family that covers the reference's own uses (carrier-modulated drives, rotating-frame terms, its test
// G(a) + 0.1 cos(t) I):
//
//     G(u, t) = sum_{j=0..m} ubar_j ( G_j + sum_c phi_c(t) H_cj ),   ubar_0 = 1,  phi_c(t) = cos(omega_c t) | sin(omega_c t)
//
// with the controls held (spline order 0) or linearly interpolated to u_{k+1} (order 1).  One workgroup per interval runs
// classical RK4 with a fixed number of sub-steps on the state TOGETHER with its exact forward sensitivities, so that the
// Jacobian block and the Hessian of mu_k' f are the derivatives of the discrete map itself (for an explicit Runge-Kutta
// method with fixed steps, differentiating the scheme equals applying the scheme to the variational equations):
//
//     parameters theta = [u_k (m), t_k, dt_k, u_{k+1} (m, order 1 only)]   -- the state x_k enters linearly through Phi
//     forward columns  x, Phi (n; Jacobian calls only), x_b (p), x_ab (p (p+1) / 2; Hessian calls only),   each of length n
//     right-hand side  (M y)_0 = M0 y0,  (M y)_b = M0 y_b + M_b y0,  (M y)_ab = M0 y_ab + M_a y_b + M_b y_a + M_ab y0
//
// The (x, theta) block of the Hessian of mu' f is -d(Phi' mu)/dtheta.  Round 3: instead of carrying the n p columns Phi_b
// forward (1536 matrix-vector products per RK4 step at 32 states, p = 6), the kernel runs the DISCRETE ADJOINT of the scheme:
// the step is a linear map y+ = R y (the ODE is linear in the state), so lambda = Phi' mu = R_1' R_2' ... R_S' mu is a backward
// recursion through the same stages with transposed matrices -- it needs no stored trajectory -- and its parameter
// sensitivities lambda_b ride along (1 + 2 p products per stage).  52 instead of 1536 products per step for that block; the
// (theta, theta) block keeps the forward second-order columns x_ab.  Per stage, backward (k4 first):
//     kbar_4 = h/6 w,  kbar_3 = h/3 w + h M4' kbar_4,  kbar_2 = h/3 w + h/2 M2' kbar_3,  kbar_1 = h/6 w + h/2 M2' kbar_2,
//     w- = w + M4' kbar_4 + M2' kbar_3 + M2' kbar_2 + M1' kbar_1          (and the product rule for the b-derivatives)
//
// where M = dt_k G(u(tau), t) and its parameter derivatives M_b, M_ab are linear combinations of the shared matrices G_j, H_cj
// (formed once per stage).  Outputs are the per-interval dense blocks of a generic integrator -- defect (n), Jacobian block
// (n x 2z), Hessian block of mu_k' f (2z x 2z) -- which the engine places with the same kernels as host-evaluated
// integrators (k_extint_*: by column ownership, so sharded handles need no halo exchange).
//
// Bound: this is small-state work (quantum-control systems in a rotating frame have 4..32 states); the kernel keeps its
// columns in an L2-resident scratch slab per workgroup and is latency-, not bandwidth- or MFMA-bound.
//
// Product modes (k_tdb_product; need 3: J w, need 4: J' w).  The discrete map is linear in the state, so a product needs no Phi:
//     J w   rows of interval k:  w_x(k+1) - d(1),  d the scheme applied to d' = M d + M_w x, d(0) = w_x(k), beside x' = M x;
//           M_w = sum_b w_theta_b M_b is ONE jet (directional coefficient row, dto_tdb_coef.hip.h).  Columns x, d; jets M, M_w.
//     J' w  per interval: the forward columns x, x_b (jets M, M_b), the p dot products w_k' x_b(1), then the one-column adjoint
//           lambda = Phi_k' w_k (the recursion above without its sensitivity columns; jet M only).  The n + p results are staged
//           per interval and k_tdb_jtv_place adds them into y, one thread per entry of y in a fixed order.
// No second-order jet, no n-column block, no staged Jacobian block, no value slab.
#include "dto_kernels.h"
#include "dto_tdb_coef.hip.h"

namespace dto {

namespace {

__host__ __device__ inline bool tdb_uses_adjoint(int n) { return n >= 12; }

__device__ __forceinline__ int pair_idx(int a, int b, int p) {  // a <= b < p, row-major upper triangle
    return a * p - a * (a - 1) / 2 + (b - a);
}

struct TdbArgs {
    KProb P;
    KTdb T;
    const double* Z;
    const double* mu;
    int need;          // 0 defect, 1 + Jacobian block, 2 + Hessian block
    int64_t i_lo;      // first interval (global, 0-based) of this launch
    double* vals;      // [K][n]
    double* jac;       // [K][2z][n]
    double* hess;      // [K][2z][2z]
    double* scratch;
    int64_t scratch_stride;
};

__global__ void __launch_bounds__(256) k_tdb(TdbArgs a) {
    const int n = a.T.n, m = a.T.m, z = a.P.z, nmod = a.T.nmod, order = a.T.order;
    const int p = m + 2 + (order ? m : 0);
    const int need = a.need;
    const int64_t kn = a.i_lo + blockIdx.x;
    const double* zk = a.Z + kn * z;
    const double* zk1 = zk + z;
    const double tk = zk[a.T.t_off], dt = zk[a.P.dt_idx];
    const int tid = threadIdx.x;
    const int P2 = p * (p + 1) / 2;
    // forward column layout: x | Phi (Jacobian calls; small-state Hessian calls) | x_b | Phi_b (small-state Hessian calls) | x_ab
    // (Hessian calls).  The (x, theta) block of a Hessian call comes from the discrete adjoint (below) from 12 states on; below,
    // the n p forward columns Phi_b are cheaper than a second pass through the stages (4 states x 1000 knots: 1.8 against 2.2 ms)
    const bool adjoint = need == 2 && tdb_uses_adjoint(n);
    const int nphi = (need == 1 || (need == 2 && !adjoint)) ? n : 0;
    const int nphib = (need == 2 && !adjoint) ? n * p : 0;
    const int c_x = 0, c_phi = 1, c_xb = 1 + nphi, c_phib = 1 + nphi + p, c_xab = 1 + nphi + p + nphib;
    const int C = need == 0 ? 1 : (need == 1 ? 1 + n + p : 1 + nphi + p + nphib + P2);
    const int nM = need == 0 ? 1 : (need == 1 ? 1 + p : 1 + p + P2);
    double* S = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    double* Y = S;
    double* ACC = Y + (int64_t)C * n;
    double* TA = ACC + (int64_t)C * n;
    double* TB = TA + (int64_t)C * n;
    double* MJ = TB + (int64_t)C * n;   // [nM][n*n] column-major jets of M
    const int nn = n * n;
    const int Q = (m + 1) * (1 + nmod);  // shared matrices B_q, q = j * (1 + nmod) + c; c = 0: G_j, c >= 1: H_{c-1, j}
    auto Bq = [&](int j, int c) { return c == 0 ? a.T.G + (int64_t)j * nn : a.T.H + ((int64_t)(c - 1) * (m + 1) + j) * nn; };
    __shared__ double coefs[TDB_MAX_COEFS];  // [nM][Q] scalar coefficient of B_q in each jet of M at the current stage time

    // jets of M(tau) = dt * sum_j a_j(tau) (G_j + sum_c phi_c(t) H_cj),  t = t_k + tau dt: first the scalar coefficient of
    // every shared matrix B_q in every jet (value / first / second derivative), then the matrices; `njet` jets are formed
    auto form_jets = [&](double tau, int njet) {
        for (int e = tid; e < njet * Q; e += 256) {
            const int which = e / Q, q = e - which * Q;
            coefs[e] = tdbm_coef(a.T, zk, zk1, tk, dt, tau, p, which, q);
        }
        __syncthreads();
        for (int e = tid; e < njet * nn; e += 256) {
            const int which = e / nn, off = e - which * nn;
            double acc = 0.0;
            for (int q = 0; q < Q; ++q) {
                const double cf = coefs[which * Q + q];
                if (cf != 0.0) acc += cf * Bq(q / (1 + nmod), q % (1 + nmod))[off];
            }
            MJ[e] = acc;
        }
        __syncthreads();
    };

    // initial values: x = x_k, Phi = I, everything else 0
    for (int e = tid; e < C * n; e += 256) {
        const int c = e / n, r = e - c * n;
        double v = 0.0;
        if (c == c_x) v = zk[a.T.x_off + r];
        else if (nphi && c >= c_phi && c < c_phi + n) v = (c - c_phi == r) ? 1.0 : 0.0;
        Y[e] = v;
    }
    __syncthreads();

    const double h = 1.0 / a.T.substeps;
    for (int step = 0; step < a.T.substeps; ++step) {
        for (int stage = 0; stage < 4; ++stage) {
            const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
            const double* IN = stage == 0 ? Y : (stage == 2 ? TB : TA);
            if (stage != 2) form_jets(tau, nM);   // stages 1 and 2 share their time
            // ---- K = F(IN), then the RK4 update of this stage
            const double* M0 = MJ;
            double* OUT = stage == 0 ? TA : (stage == 1 ? TB : (stage == 2 ? TA : Y));
            const double w_acc = (stage == 0 || stage == 3) ? h / 6.0 : h / 3.0;
            const double w_tmp = stage == 2 ? h : 0.5 * h;
            for (int e = tid; e < C * n; e += 256) {
                const int c = e / n, r = e - c * n;
                auto mv = [&](const double* M, int col) {   // (M * IN[col])[r]
                    double s = 0.0;
                    const double* y = IN + (int64_t)col * n;
                    for (int k = 0; k < n; ++k) s += M[r + k * n] * y[k];
                    return s;
                };
                double K = mv(M0, c);
                if (need >= 1 && c >= c_xb && c < c_xb + p) K += mv(MJ + (int64_t)(1 + c - c_xb) * nn, c_x);
                else if (nphib && c >= c_phib && c < c_phib + nphib) {
                    const int b = (c - c_phib) / n, i = (c - c_phib) - b * n;
                    K += mv(MJ + (int64_t)(1 + b) * nn, c_phi + i);
                } else if (need >= 2 && c >= c_xab) {
                    int rem = c - c_xab, aa = 0;
                    while (rem >= p - aa) { rem -= p - aa; ++aa; }
                    const int bb = aa + rem;
                    K += mv(MJ + (int64_t)(1 + aa) * nn, c_xb + bb) + mv(MJ + (int64_t)(1 + bb) * nn, c_xb + aa) +
                         mv(MJ + (int64_t)(1 + p + pair_idx(aa, bb, p)) * nn, c_x);
                }
                const double y0 = Y[e];
                if (stage == 0) { ACC[e] = y0 + w_acc * K; OUT[e] = y0 + w_tmp * K; }
                else if (stage < 3) { ACC[e] += w_acc * K; OUT[e] = y0 + w_tmp * K; }
                else OUT[e] = ACC[e] + w_acc * K;
            }
            __syncthreads();
        }
    }

    // ---- outputs (blocks of a generic integrator: _integrators.jl:49-77)
    for (int r = tid; r < n; r += 256) a.vals[kn * n + r] = zk1[a.T.x_off + r] - Y[c_x * n + r];
    if (need < 1) return;
    auto zz_of = [&](int b) { return tdb_param_entry(a.T, z, a.P.dt_idx, b); };
    if (need == 1) {
        double* J = a.jac + kn * (int64_t)n * 2 * z;
        for (int e = tid; e < n * 2 * z; e += 256) J[e] = 0.0;
        __syncthreads();
        for (int e = tid; e < n * n; e += 256) {
            const int i = e / n, r = e - i * n;
            J[(int64_t)(a.T.x_off + i) * n + r] = -Y[(int64_t)(c_phi + i) * n + r];
        }
        for (int r = tid; r < n; r += 256) J[(int64_t)(z + a.T.x_off + r) * n + r] = 1.0;
        __syncthreads();
        // parameter columns ADD (a component may serve twice, e.g. the timestep listed as the time variable)
        if (tid < n)
            for (int b = 0; b < p; ++b) J[(int64_t)zz_of(b) * n + tid] -= Y[(int64_t)(c_xb + b) * n + tid];
        return;
    }

    const double* muk = a.mu + a.T.row_off + kn * n;
    const int ld = 2 * z;
    double* Hb = a.hess + kn * (int64_t)4 * z * z;
    auto theta_block = [&]() {   // (theta_a, theta_b): -mu' x_ab.  Entries that land on the same (row, col) meet by atomics
        for (int e = tid; e < P2; e += 256) {
            int rem = e, aa = 0;
            while (rem >= p - aa) { rem -= p - aa; ++aa; }
            const int bb = aa + rem;
            double s = 0.0;
            for (int r = 0; r < n; ++r) s += muk[r] * Y[(int64_t)(c_xab + e) * n + r];
            const int ra = zz_of(aa), rb = zz_of(bb);
            atomicAdd(&Hb[ra + (int64_t)ld * rb], -s);
            if (aa != bb) atomicAdd(&Hb[rb + (int64_t)ld * ra], -s);
        }
    };
    if (!adjoint) {
        // small state: (x_i, theta_b) = -mu' dPhi_i/dtheta_b from the forward columns Phi_b
        for (int e = tid; e < 4 * z * z; e += 256) Hb[e] = 0.0;
        __syncthreads();
        for (int e = tid; e < n * p; e += 256) {
            const int b = e / n, i = e - b * n;
            double s = 0.0;
            for (int r = 0; r < n; ++r) s += muk[r] * Y[(int64_t)(c_phib + b * n + i) * n + r];
            const int ri = a.T.x_off + i, cb = zz_of(b);
            atomicAdd(&Hb[ri + (int64_t)ld * cb], -s);
            atomicAdd(&Hb[cb + (int64_t)ld * ri], -s);
        }
        theta_block();
        return;
    }
    // ---- Hessian call: discrete adjoint lambda = Phi' mu and its parameter sensitivities lambda_b, backward through the steps.
    // Columns 0 .. p of W: lambda, lambda_b.  The forward arrays are free now (Y keeps x_ab for the (theta, theta) block).
    const int CA = 1 + p;
    double* W = TA;                              // current adjoint columns
    double* WN = TB;                             // w- being accumulated
    double* KB = ACC;                            // kbar of the stage at hand
    double* UB = ACC + (int64_t)CA * n;          // ubar = M' kbar (and product rule)
    for (int e = tid; e < CA * n; e += 256) W[e] = e < n ? muk[e] : 0.0;
    __syncthreads();
    for (int step = a.T.substeps - 1; step >= 0; --step) {
        for (int e = tid; e < CA * n; e += 256) WN[e] = W[e];
        // stage 3 (k4, time tau + h), stages 2 and 1 (k3, k2, time tau + h/2), stage 0 (k1, time tau)
        for (int stage = 3; stage >= 0; --stage) {
            const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
            if (stage != 1) form_jets(tau, CA);   // stages 2 and 1 share their time (form_jets ends with a barrier)
            // kbar of this stage from w and the previous stage's ubar
            const double cw = (stage == 3 || stage == 0) ? h / 6.0 : h / 3.0;
            const double cu = stage == 3 ? 0.0 : (stage == 2 ? h : 0.5 * h);
            for (int e = tid; e < CA * n; e += 256) KB[e] = cw * W[e] + (cu != 0.0 ? cu * UB[e] : 0.0);
            __syncthreads();
            // ubar_c = M' kbar_c (+ M_b' kbar_0 for the sensitivity columns)
            for (int e = tid; e < CA * n; e += 256) {
                const int c = e / n, r = e - c * n;
                auto mvT = [&](const double* M, int col) {   // (M' * KB[col])[r] = column r of M . KB[col]
                    double s = 0.0;
                    const double* y = KB + (int64_t)col * n;
                    const double* mc = M + (int64_t)r * n;
                    for (int k = 0; k < n; ++k) s += mc[k] * y[k];
                    return s;
                };
                double u = mvT(MJ, c);
                if (c >= 1) u += mvT(MJ + (int64_t)c * nn, 0);
                UB[e] = u;   // (KB is read, UB written: no hazard inside this loop; UB's old values were consumed above)
                WN[e] += u;
            }
            __syncthreads();
        }
        for (int e = tid; e < CA * n; e += 256) W[e] = WN[e];
        __syncthreads();
    }

    for (int e = tid; e < 4 * z * z; e += 256) Hb[e] = 0.0;
    __syncthreads();
    // (x_i, theta_b): -d lambda_i / d theta_b, one thread per entry
    for (int e = tid; e < n * p; e += 256) {
        const int b = e / n, i = e - b * n;
        const double s = W[(int64_t)(1 + b) * n + i];
        const int ri = a.T.x_off + i, cb = zz_of(b);
        atomicAdd(&Hb[ri + (int64_t)ld * cb], -s);
        atomicAdd(&Hb[cb + (int64_t)ld * ri], -s);
    }
    theta_block();
}

// (1 + p) rows of first-order coefficients and the directional row: (2 + p) Q <= 2/3 (1 + p + p (p+1)/2) Q for p >= 2
constexpr int TDB_PRODUCT_COEFS = TDB_MAX_COEFS * 2 / 3;

struct TdbProductArgs {
    KProb P;
    KTdb T;
    const double* Z;
    const double* w;
    int need;          // 3: J w, 4: J' w
    double* out;       // need 3: y (the integrator's rows are assigned); need 4: staging [K][n + p]
    double* scratch;
    int64_t scratch_stride;
};

__global__ void __launch_bounds__(256) k_tdb_product(TdbProductArgs a) {
    const int n = a.T.n, m = a.T.m, z = a.P.z, nmod = a.T.nmod, order = a.T.order;
    const int p = m + 2 + (order ? m : 0);
    const int need = a.need;
    const int64_t kn = blockIdx.x;
    const double* zk = a.Z + kn * z;
    const double* zk1 = zk + z;
    const double tk = zk[a.T.t_off], dt = zk[a.P.dt_idx];
    const int tid = threadIdx.x;
    // columns: x, d (J w) | x, x_b (J' w); jet c belongs to column c: M, then M_w | M_b
    const int C = need == 3 ? 2 : 1 + p;
    double* S = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    double* Y = S;
    double* ACC = Y + (int64_t)C * n;
    double* TA = ACC + (int64_t)C * n;
    double* TB = TA + (int64_t)C * n;
    double* MJ = TB + (int64_t)C * n;   // [C][n*n] column-major jets of M
    const int nn = n * n;
    const int Q = (m + 1) * (1 + nmod);
    auto Bq = [&](int j, int c) { return c == 0 ? a.T.G + (int64_t)j * nn : a.T.H + ((int64_t)(c - 1) * (m + 1) + j) * nn; };
    __shared__ double coefs[TDB_PRODUCT_COEFS];   // rows 0 .. p of tdbm_coef, row 1 + p: the directional row (J w)
    __shared__ double w_theta[2 * MAX_DRIVES + 2];
    if (need == 3 && tid < p) w_theta[tid] = a.w[kn * z + tdb_param_entry(a.T, z, a.P.dt_idx, tid)];

    // `njet` jets at tau: the coefficient rows, then the matrices (jet s from row s; in a J w call jet 1 from the directional row)
    auto form_jets = [&](double tau, int njet) {
        const int rows = need == 3 ? 1 + p : njet;
        for (int e = tid; e < rows * Q; e += 256) coefs[e] = tdbm_coef(a.T, zk, zk1, tk, dt, tau, p, e / Q, e % Q);
        __syncthreads();
        if (need == 3) {
            for (int q = tid; q < Q; q += 256) coefs[(1 + p) * Q + q] = tdbm_dir_coef(coefs, Q, p, q, w_theta);
            __syncthreads();
        }
        for (int e = tid; e < njet * nn; e += 256) {
            const int s = e / nn, off = e - s * nn;
            const double* cf = coefs + (need == 3 && s == 1 ? 1 + p : s) * Q;
            double acc = 0.0;
            for (int q = 0; q < Q; ++q)
                if (cf[q] != 0.0) acc += cf[q] * Bq(q / (1 + nmod), q % (1 + nmod))[off];
            MJ[e] = acc;
        }
        __syncthreads();
    };

    // initial values: x = x_k, d = w_x(k), x_b = 0
    for (int e = tid; e < C * n; e += 256) {
        const int c = e / n, r = e - c * n;
        Y[e] = c == 0 ? zk[a.T.x_off + r] : (need == 3 ? a.w[kn * z + a.T.x_off + r] : 0.0);
    }
    __syncthreads();

    const double h = 1.0 / a.T.substeps;
    for (int step = 0; step < a.T.substeps; ++step) {
        for (int stage = 0; stage < 4; ++stage) {
            const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
            const double* IN = stage == 0 ? Y : (stage == 2 ? TB : TA);
            if (stage != 2) form_jets(tau, C);   // stages 1 and 2 share their time
            double* OUT = stage == 0 ? TA : (stage == 1 ? TB : (stage == 2 ? TA : Y));
            const double w_acc = (stage == 0 || stage == 3) ? h / 6.0 : h / 3.0;
            const double w_tmp = stage == 2 ? h : 0.5 * h;
            for (int e = tid; e < C * n; e += 256) {
                const int c = e / n, r = e - c * n;
                auto mv = [&](const double* M, int col) {   // (M * IN[col])[r]
                    double s = 0.0;
                    const double* y = IN + (int64_t)col * n;
                    for (int k = 0; k < n; ++k) s += M[r + k * n] * y[k];
                    return s;
                };
                double K = mv(MJ, c);
                if (c >= 1) K += mv(MJ + (int64_t)c * nn, 0);
                const double y0 = Y[e];
                if (stage == 0) { ACC[e] = y0 + w_acc * K; OUT[e] = y0 + w_tmp * K; }
                else if (stage < 3) { ACC[e] += w_acc * K; OUT[e] = y0 + w_tmp * K; }
                else OUT[e] = ACC[e] + w_acc * K;
            }
            __syncthreads();
        }
    }

    if (need == 3) {
        for (int r = tid; r < n; r += 256) a.out[a.T.row_off + kn * n + r] = a.w[(kn + 1) * z + a.T.x_off + r] - Y[n + r];
        return;
    }
    const double* wk = a.w + a.T.row_off + kn * n;
    double* out = a.out + kn * (int64_t)(n + p);
    for (int b = tid; b < p; b += 256) {   // w_k' (dPhi_k / dtheta_b) x_k
        double s = 0.0;
        for (int r = 0; r < n; ++r) s += wk[r] * Y[(int64_t)(1 + b) * n + r];
        out[n + b] = s;
    }
    // lambda = Phi_k' w_k: the discrete adjoint, one column, backward through the steps (k_tdb's recursion)
    double* W = TA;
    double* WN = TB;
    double* KB = ACC;
    double* UB = ACC + n;
    for (int e = tid; e < n; e += 256) W[e] = wk[e];
    __syncthreads();
    for (int step = a.T.substeps - 1; step >= 0; --step) {
        for (int e = tid; e < n; e += 256) WN[e] = W[e];
        for (int stage = 3; stage >= 0; --stage) {
            const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
            if (stage != 1) form_jets(tau, 1);   // stages 2 and 1 share their time (form_jets ends with a barrier)
            const double cw = (stage == 3 || stage == 0) ? h / 6.0 : h / 3.0;
            const double cu = stage == 3 ? 0.0 : (stage == 2 ? h : 0.5 * h);
            for (int e = tid; e < n; e += 256) KB[e] = cw * W[e] + (cu != 0.0 ? cu * UB[e] : 0.0);
            __syncthreads();
            for (int r = tid; r < n; r += 256) {   // ubar = M' kbar: column r of M . kbar
                double s = 0.0;
                const double* mc = MJ + (int64_t)r * n;
                for (int k = 0; k < n; ++k) s += mc[k] * KB[k];
                UB[r] = s;
                WN[r] += s;
            }
            __syncthreads();
        }
        for (int e = tid; e < n; e += 256) W[e] = WN[e];
        __syncthreads();
    }
    for (int i = tid; i < n; i += 256) out[i] = W[i];
}

// J' w: the staged per-interval results into y.  One thread per entry of the knots' part of y adds what the interval on its left
// (w_{k-1}, the u_{k+1} terms) and the interval on its right (-Phi_k' w_k, the u_k, t_k, dt_k terms) contribute, in that order
__global__ void __launch_bounds__(256) k_tdb_jtv_place(KProb P, KTdb T, const double* __restrict__ w, const double* __restrict__ stage,
                                                       double* __restrict__ y) {
    const int z = P.z, n = T.n, m = T.m, p = m + 2 + (T.order ? m : 0);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= P.N * z) return;
    const int64_t kn = e / z;
    const int c = (int)(e - kn * z), i = c - T.x_off;
    const bool in_x = i >= 0 && i < n;
    double acc = 0.0;
    if (kn >= 1) {
        if (in_x) acc += w[T.row_off + (kn - 1) * n + i];
        if (T.order) {
            const double* s = stage + (kn - 1) * (int64_t)(n + p) + n + m + 2;
            for (int j = 0; j < m; ++j)
                if (T.u_off + j == c) acc -= s[j];
        }
    }
    if (kn < P.K) {
        const double* s = stage + kn * (int64_t)(n + p);
        if (in_x) acc -= s[i];
        for (int b = 0; b < m + 2; ++b)
            if (tdb_param_entry(T, z, P.dt_idx, b) == c) acc -= s[n + b];
    }
    y[e] += acc;
}

}  // namespace

bool tdb_supported(const KTdb& T) {
    return T.n >= 1 && T.n <= 64 && T.nmod >= 0 && T.substeps >= 1 && tdb_table_fits(T.m, T.order, T.nmod);
}

size_t tdb_scratch_doubles(const KTdb& T, int need) {
    const int n = T.n, p = tdb_num_params(T.m, T.order);
    const size_t P2 = tdb_num_pairs(p);
    if (need >= 3) {   // product modes: x, d | x, x_b, one jet per column
        const size_t Cp = need == 3 ? 2 : 1 + p;
        return 4 * Cp * n + Cp * (size_t)n * n;
    }
    const size_t C = need == 0 ? 1 : (need == 1 ? 1 + n + p : (tdb_uses_adjoint(n) ? 1 + p + P2 : 1 + n + p + (size_t)n * p + P2));
    const size_t nM = need == 0 ? 1 : (need == 1 ? 1 + p : 1 + p + P2);
    return 4 * C * n + nM * (size_t)n * n;
}

hipError_t launch_tdb(hipStream_t st, const KProb& P, const KTdb& T, const double* dZ, const double* dmu, int need, int64_t i_lo,
                      int64_t count, double* vals, double* jac, double* hess, double* scratch, size_t scratch_stride) {
    if (count <= 0) return hipSuccess;
    TdbArgs a{};
    a.P = P; a.T = T; a.Z = dZ; a.mu = dmu; a.need = need; a.i_lo = i_lo;
    a.vals = vals; a.jac = jac; a.hess = hess; a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride;
    hipLaunchKernelGGL(k_tdb, dim3((unsigned)count), dim3(P.debug_bad_launch ? 4096 : 256), 0, st, a);
    return hipGetLastError();
}

// flops of one interval of a product call as executed: per stage the M and jet products of every column, per stage time the jets
double tdb_product_flops(const KTdb& T, int need) {
    const double n2 = (double)T.n * T.n, S = T.substeps;
    const int p = tdb_num_params(T.m, T.order), C = need == 3 ? 2 : 1 + p, Q = tdb_num_shared(T.m, T.nmod);
    double fl = 4.0 * 2.0 * n2 * (2 * C - 1) + 3.0 * 2.0 * Q * n2 * C;
    if (need == 4) fl += 4.0 * 2.0 * n2 + 3.0 * 2.0 * Q * n2;
    return S * fl;
}

hipError_t launch_tdb_product(hipStream_t st, const KProb& P, const KTdb& T, const double* dZ, const double* dw, int need, double* out,
                              double* scratch, size_t scratch_stride) {
    if (P.K <= 0) return hipSuccess;
    if ((need != 3 && need != 4) || tdb_scratch_doubles(T, need) > scratch_stride) return hipErrorInvalidValue;
    TdbProductArgs a{};
    a.P = P; a.T = T; a.Z = dZ; a.w = dw; a.need = need; a.out = out; a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride;
    hipLaunchKernelGGL(k_tdb_product, dim3((unsigned)P.K), dim3(P.debug_bad_launch ? 4096 : 256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tdb_jtv_place(hipStream_t st, const KProb& P, const KTdb& T, const double* dw, const double* stage, double* dy) {
    const int64_t entries = P.N * P.z;
    if (entries <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tdb_jtv_place, dim3((unsigned)((entries + 255) / 256)), dim3(P.debug_bad_launch ? 4096 : 256), 0, st, P, T, dw, stage, dy);
    return hipGetLastError();
}

}  // namespace dto
