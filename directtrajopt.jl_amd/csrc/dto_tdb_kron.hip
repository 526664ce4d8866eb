// dto_tdb_kron.hip -- TimeDependentBilinearIntegrator whose generator family is replicated blocks, G_j = I_r (x) B_j and
// H_cj = I_r (x) B_cj (DTO_FLAG_BLOCK_GENERATORS).
//
// The state is an operator in isomorphic coordinates, x = vec(X) with X of b x r, and the discrete flow of k_tdb / k_tdb_mfma
// (classical RK4, `substeps` fixed steps on tau in [0, 1], parameters theta = [u_k (m), t_k, dt_k, u_{k+1} (m, order 1)]) is
// I_r (x) Phi~ with Phi~ the same scheme on b x b.  So the kernel is k_tdb_mfma's mathematics on matrices:
//
//   * the Q = (m+1)(1+nmod) shared blocks B_q (zero-padded to bp x bp, bp a multiple of 16; blocks below 16 rows grouped to
//     I_g (x) B as on the bilinear structured path) are read through the caches; M0 = sum_q c_q B_q is formed once per stage time
//     into LDS (from the transposed blocks in the adjoint recursion), as k_kron keeps Gu;
//   * a derivative jet is applied as a scalar combination of U_q = B_q Y -- no matrix per parameter;
//   * every product is v_mfma_f64_16x16x4_f64 on 16-column tiles, one wavefront per tile and task.  A "column group" is the cp
//     columns (r rounded up to 16) that one vector of the dense kernels becomes:
//         defect    X
//         Jacobian  X, X_a (p groups) | Phi~ (bp columns, starts as I_b)
//         Hessian   X, X_a, X_ab (p (p+1) / 2 groups) forward; Lambda = Phi~' M_k, Lambda_a (p groups) backward through the same
//                   stages with M0' (the discrete adjoint of DESIGN 4.11 on matrices).  No Phi~.
//         J w       X | D (k_tdb_kron_product, the matrix-free products of DESIGN 4.24: no Phi~, no staged block)
//         J' w      X, X_b (p groups) forward; Lambda = Phi~' W_k, one group, backward
//   * a persistent grid of `resident` workgroups walks the intervals, one scratch slot each.
//
// Numerical rules: what a workgroup computes is a function of its interval's data alone, every sum has a fixed
// order, there is no floating-point atomic, every output entry has one writer.  The kernel ASSIGNS the entries it owns in the staged
// blocks vals [K][n], jac [K][2z][n], hess [K][2z][2z] -- the r diagonal b x b blocks of -(I_r (x) Phi~), the theta columns, the +I,
// the (x, theta) and (theta, theta) entries; state, controls, t and dt are disjoint components on this path, so no two of them
// share a position -- and leaves alone the constant zeros the engine wrote when it allocated the blocks.  Padded rows and columns
// are computed (they are zeros) and never written out.
#include <algorithm>

#include "dto_gemm.hip.h"
#include "dto_kernels.h"
#include "dto_tdb_coef.hip.h"

namespace dto {

namespace {

constexpr int TDBK_MAX_PAIRS = 160;   // p (p+1) / 2 <= 136 at 7 drives, order 1

inline __host__ __device__ int pad16(int v) { return (v + 15) / 16 * 16; }

// scratch of one resident workgroup (doubles): four column sets, the U_q groups, ubar of the adjoint, the coefficient table
struct TdbkLayout {
    int bp, cp, p, P2, Q, G, ctot, ucols, wcols, njet;
    size_t oY, oACC, oTA, oTB, oU, oUB, oCoef, total;
};
// need 0 .. 2, the value calls of k_tdb_kron.  (Kept apart from the product modes below: with their cases folded into this function
// k_tdb_kron<1> was allocated 160 registers instead of 161 -- DESIGN 4.21, last paragraph.)
inline __host__ __device__ TdbkLayout tdbk_layout(const KTdb& T, const KKron& K, int need) {
    TdbkLayout L;
    L.bp = K.bp;
    L.cp = pad16(K.rw);
    L.p = tdb_num_params(T.m, T.order);
    L.P2 = tdb_num_pairs(L.p);
    L.Q = tdb_num_shared(T.m, T.nmod);
    L.G = need == 0 ? 1 : (need == 1 ? 1 + L.p : 1 + L.p + L.P2);   // column groups of the forward pass
    L.ctot = L.G * L.cp + (need == 1 ? L.bp : 0);
    L.ucols = need == 0 ? 0 : (need == 1 ? L.cp : (1 + L.p) * L.cp);  // columns whose U_q enter this call's jets
    L.wcols = need == 2 ? (1 + L.p) * L.cp : 0;
    L.njet = L.G;
    const size_t cols = (size_t)L.bp * L.ctot;
    L.oY = 0; L.oACC = cols; L.oTA = 2 * cols; L.oTB = 3 * cols;
    L.oU = 4 * cols;
    L.oUB = L.oU + (size_t)L.Q * L.ucols * L.bp;
    L.oCoef = L.oUB + (size_t)L.wcols * L.bp;
    L.total = L.oCoef + (size_t)L.njet * L.Q;
    L.total = (L.total + 1) & ~(size_t)1;
    return L;
}
// need 3 (J w: groups X | D) and 4 (J' w: groups X, X_b forward, one adjoint group), the product modes of k_tdb_kron_product: no
// Phi~ columns, the U_q of the X group alone, a cp-column ubar for the adjoint; table rows 0 .. p, and in a J w call the
// directional row behind them.  The same order of the slot's parts.
inline __host__ __device__ TdbkLayout tdbk_product_layout(const KTdb& T, const KKron& K, int need) {
    TdbkLayout L;
    L.bp = K.bp;
    L.cp = pad16(K.rw);
    L.p = tdb_num_params(T.m, T.order);
    L.P2 = tdb_num_pairs(L.p);
    L.Q = tdb_num_shared(T.m, T.nmod);
    L.G = need == 3 ? 2 : 1 + L.p;
    L.ctot = L.G * L.cp;
    L.ucols = L.cp;
    L.wcols = need == 4 ? L.cp : 0;
    L.njet = need == 3 ? 2 + L.p : 1 + L.p;
    const size_t cols = (size_t)L.bp * L.ctot;
    L.oY = 0; L.oACC = cols; L.oTA = 2 * cols; L.oTB = 3 * cols;
    L.oU = 4 * cols;
    L.oUB = L.oU + (size_t)L.Q * L.ucols * L.bp;
    L.oCoef = L.oUB + (size_t)L.wcols * L.bp;
    L.total = L.oCoef + (size_t)L.njet * L.Q;
    L.total = (L.total + 1) & ~(size_t)1;
    return L;
}
inline TdbkLayout tdbk_layout_of(const KTdb& T, const KKron& K, int need) {
    return need >= 3 ? tdbk_product_layout(T, K, need) : tdbk_layout(T, K, need);
}

struct TdbkArgs {
    KProb P;
    KTdb T;
    KKron K;             // Bm / BmT: the Q working blocks B_q and their transposes, q = j (1 + nmod) + c (c = 0: G_j, c >= 1: H_{c-1, j})
    const double* Z;
    const double* mu;
    int need;
    int64_t i_lo, count;
    double* vals;        // [K][n]
    double* jac;         // [K][2z][n]
    double* hess;        // [K][2z][2z]
    double* scratch;
    int64_t scratch_stride;
};

// acc[ti] += Mat[16 ti + lr][k] * frag[k] over this lane's k range (lane l: lr = l & 15, kk = l >> 4, k = kk KS + s): the product is
// issued transposed (dto_gemm.hip.h), so acc[ti][reg] is row 16 ti + lr, column kk + 4 reg of the 16-column tile (k_kron's form).
template <int MT>
__device__ __forceinline__ void tile_mac(const double* __restrict__ mat, int ld, const double (&frag)[4 * MT], d4 (&acc)[MT]) {
    const int lr = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int s = 0; s < 4 * MT; ++s) {
        const double* col = mat + (size_t)(kk * 4 * MT + s) * ld + lr;
#pragma unroll
        for (int ti = 0; ti < MT; ++ti) acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(frag[s], col[16 * ti], acc[ti], 0, 0, 0);
    }
}

template <int MT>
__device__ __forceinline__ void load_frag(const double* __restrict__ slab, int col, double (&frag)[4 * MT]) {
    constexpr int BP = 16 * MT;
    const int lr = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4;
    const d2* p = reinterpret_cast<const d2*>(slab + (size_t)(col + lr) * BP + kk * 4 * MT);
#pragma unroll
    for (int s = 0; s < 2 * MT; ++s) { const d2 v = p[s]; frag[2 * s] = v.x; frag[2 * s + 1] = v.y; }
}

template <int MT>
__global__ void __launch_bounds__(256) k_tdb_kron(TdbkArgs a) {
    constexpr int BP = 16 * MT;
    constexpr int LD = (MT & 1) ? BP : BP + 16;   // as k_kron: LD mod 32 == 16
    const TdbkLayout L = tdbk_layout(a.T, a.K, a.need);
    const int n = a.T.n, z = a.P.z, need = a.need;
    const int bw = a.K.bw, rw = a.K.rw, bf = a.K.b;
    const int cp = L.cp, p = L.p, P2 = L.P2, Q = L.Q, G = L.G, ctot = L.ctot, ucols = L.ucols;
    const int cpt = cp / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, kk = lane >> 4;
    constexpr size_t bb = (size_t)BP * BP;
    __shared__ double sM0[BP * LD];
    __shared__ unsigned char pair_a[TDBK_MAX_PAIRS], pair_b[TDBK_MAX_PAIRS];
    for (int e = tid; e < P2; e += 256) {
        int aa, ab;
        tdb_pair_unrank(e, p, &aa, &ab);
        pair_a[e] = (unsigned char)aa; pair_b[e] = (unsigned char)ab;
    }
    double* S = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    double* Y = S + L.oY;
    double* ACC = S + L.oACC;
    double* TA = S + L.oTA;
    double* TB = S + L.oTB;
    double* U = S + L.oU;          // [Q][ucols][BP]
    double* UB = S + L.oUB;        // [wcols][BP]
    double* coefs = S + L.oCoef;   // [jets][Q]
    __syncthreads();

    for (int64_t it = blockIdx.x; it < a.count; it += gridDim.x) {
        const int64_t kn = a.i_lo + it;
        const double* zk = a.Z + kn * z;
        const double* zk1 = zk + z;
        const double tk = zk[a.T.t_off], dt = zk[a.P.dt_idx];

        // coefficients of `njet` jets at tau, then M0 = sum_q c_q B_q (B_q' in the adjoint) into LDS, in the fixed order q = 0, 1, ...
        auto form_m0 = [&](double tau, int njet, const double* __restrict__ B) {
            for (int e = tid; e < njet * Q; e += 256) coefs[e] = tdbm_coef(a.T, zk, zk1, tk, dt, tau, p, e / Q, e % Q);
            __syncthreads();
            for (int e = tid; e < BP * BP; e += 256) {
                double acc = 0.0;
                for (int q = 0; q < Q; ++q) acc += coefs[q] * B[q * bb + e];
                sM0[(e % BP) + (e / BP) * LD] = acc;
            }
            __syncthreads();
        };
        // U[q][c0 + ..] = B_q IN[c0 + ..] for `ntile` 16-column tiles of IN from column 0 on: one wavefront per (q, tile)
        auto u_pass = [&](const double* __restrict__ B, const double* __restrict__ IN, int ntile) {
            for (int task = wave; task < Q * ntile; task += 4) {
                const int q = task / ntile, t = task - q * ntile;
                d4 acc[MT];
                double frag[4 * MT];
#pragma unroll
                for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
                load_frag<MT>(IN, 16 * t, frag);
                tile_mac<MT>(B + q * bb, BP, frag, acc);
#pragma unroll
                for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) U[((size_t)q * ucols + 16 * t + kk + 4 * r) * BP + 16 * ti + lr] = acc[ti][r];
            }
            __syncthreads();
        };
        // sum_q cf[q] U_q[col][row]
        auto jet = [&](const double* cf, int col, int row) {
            double s = 0.0;
            for (int q = 0; q < Q; ++q) s += cf[q] * U[((size_t)q * ucols + col) * BP + row];
            return s;
        };
        // entry of state index e (row i of replica c of the working block: e = c bw + i) in column group g of a slab
        auto at_state = [&](const double* slab, int g, int e) { const int c = e / bw, i = e - c * bw; return slab[((size_t)g * cp + c) * BP + i]; };

        // initial values: X = reshape(x_k), Phi~ = I, everything else (padding included) 0
        for (int e = tid; e < BP * ctot; e += 256) {
            const int c = e / BP, i = e - c * BP;
            double v = 0.0;
            if (i < bw) {
                if (c < rw) v = zk[a.T.x_off + c * bw + i];
                else if (c >= G * cp) v = (c - G * cp == i) ? 1.0 : 0.0;
            }
            Y[e] = v;
        }
        __syncthreads();

        const double h = 1.0 / a.T.substeps;
        for (int step = 0; step < a.T.substeps; ++step) {
            for (int stage = 0; stage < 4; ++stage) {
                const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
                const double* IN = stage == 0 ? Y : (stage == 2 ? TB : TA);
                double* OUT = stage == 0 ? TA : (stage == 1 ? TB : (stage == 2 ? TA : Y));
                if (stage != 2) form_m0(tau, L.njet, a.K.Bm);   // stages 1 and 2 share their time
                // U_q = B_q IN for the groups whose jets enter this call: X (Jacobian), X and X_a (Hessian)
                if (need >= 1) u_pass(a.K.Bm, IN, ucols / 16);
                const double w_acc = (stage == 0 || stage == 3) ? h / 6.0 : h / 3.0;
                const double w_tmp = stage == 2 ? h : 0.5 * h;
                // K = M0 IN (+ the jets' terms), then the RK4 update of this stage: one wavefront per 16-column tile
                for (int task = wave; task < ctot / 16; task += 4) {
                    const int c0 = 16 * task, g = c0 / cp, cw0 = c0 - g * cp;   // g >= G: the Phi~ columns
                    d4 acc[MT];
                    double frag[4 * MT];
#pragma unroll
                    for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
                    load_frag<MT>(IN, c0, frag);
                    tile_mac<MT>(sM0, LD, frag, acc);
                    const int e2 = g - 1 - p;
                    const int aa = (g > p && g < G) ? pair_a[e2] : 0, ab = (g > p && g < G) ? pair_b[e2] : 0;
#pragma unroll
                    for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * ti + lr, cw = cw0 + kk + 4 * r;
                            double Kv = acc[ti][r];
                            if (g >= 1 && g <= p) Kv += jet(coefs + (size_t)g * Q, cw, row);   // jet 1 + b, b = g - 1
                            else if (g > p && g < G) {
                                const double *ca = coefs + (size_t)(1 + aa) * Q, *cb = coefs + (size_t)(1 + ab) * Q, *cab = coefs + (size_t)g * Q;
                                double s = 0.0;
                                for (int q = 0; q < Q; ++q) {
                                    const double* uq = U + ((size_t)q * ucols + cw) * BP + row;
                                    s += ca[q] * uq[(size_t)(1 + ab) * cp * BP] + cb[q] * uq[(size_t)(1 + aa) * cp * BP] + cab[q] * uq[0];
                                }
                                Kv += s;
                            }
                            const size_t e = (size_t)(c0 + kk + 4 * r) * BP + row;
                            const double y0 = Y[e];
                            if (stage == 0) { ACC[e] = y0 + w_acc * Kv; OUT[e] = y0 + w_tmp * Kv; }
                            else if (stage < 3) { ACC[e] += w_acc * Kv; OUT[e] = y0 + w_tmp * Kv; }
                            else OUT[e] = ACC[e] + w_acc * Kv;
                        }
                }
                __syncthreads();
            }
        }

        // ---- outputs: the owned entries of the staged blocks, each assigned by one thread
        for (int e = tid; e < n; e += 256) a.vals[kn * n + e] = zk1[a.T.x_off + e] - at_state(Y, 0, e);
        auto zz_of = [&](int b) { return tdb_param_entry(a.T, z, a.P.dt_idx, b); };
        if (need == 1) {
            double* J = a.jac + kn * (int64_t)n * 2 * z;
            // -(I_r (x) Phi~): the diagonal blocks of the finest size (what lies outside them is a constant zero)
            const double* PHI = Y + (size_t)G * cp * BP;
            for (int e = tid; e < n * bf; e += 256) {
                const int j = e / bf, i = e - j * bf;      // state column j, row i of its finest block
                const int blk = j / bf;
                const int jw = j % bw, iw = (blk * bf) % bw + i;   // position inside the working block
                J[(int64_t)(a.T.x_off + j) * n + blk * bf + i] = -PHI[(size_t)jw * BP + iw];
            }
            for (int e = tid; e < n; e += 256) J[(int64_t)(z + a.T.x_off + e) * n + e] = 1.0;
            for (int e = tid; e < n * p; e += 256) {
                const int b = e / n, s = e - b * n;
                J[(int64_t)zz_of(b) * n + s] = -at_state(Y, 1 + b, s);
            }
        } else if (need == 2) {
            // discrete adjoint Lambda = Phi~' M_k and its parameter sensitivities Lambda_a, backward through the steps (k_tdb_mfma's
            // recursion on column groups).  Groups 0 .. p of W: Lambda, Lambda_a; Y keeps X_ab for the (theta, theta) block.
            const double* muk = a.mu + a.T.row_off + kn * n;
            double* W = TA;
            double* WN = TB;
            double* KB = ACC;
            const int CA = 1 + p, nv = BP * CA * cp;
            for (int e = tid; e < nv; e += 256) {
                const int c = e / BP, i = e - c * BP;
                W[e] = (c < rw && i < bw) ? muk[c * bw + i] : 0.0;
                UB[e] = 0.0;
            }
            __syncthreads();
            for (int step = a.T.substeps - 1; step >= 0; --step) {
                for (int e = tid; e < nv; e += 256) WN[e] = W[e];
                for (int stage = 3; stage >= 0; --stage) {
                    const double tau = (step + (stage == 0 ? 0.0 : (stage == 3 ? 1.0 : 0.5))) * h;
                    if (stage != 1) form_m0(tau, CA, a.K.BmT);   // stages 2 and 1 share their time
                    const double cw_ = (stage == 3 || stage == 0) ? h / 6.0 : h / 3.0;
                    const double cu = stage == 3 ? 0.0 : (stage == 2 ? h : 0.5 * h);
                    for (int e = tid; e < nv; e += 256) KB[e] = cw_ * W[e] + (cu != 0.0 ? cu * UB[e] : 0.0);
                    __syncthreads();
                    u_pass(a.K.BmT, KB, cpt);   // U_q = B_q' kbar_0
                    // ubar_g = M0' kbar_g (+ M_a' kbar_0 for the sensitivity groups)
                    for (int task = wave; task < CA * cpt; task += 4) {
                        const int c0 = 16 * task, g = c0 / cp, cw0 = c0 - g * cp;
                        d4 acc[MT];
                        double frag[4 * MT];
#pragma unroll
                        for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
                        load_frag<MT>(KB, c0, frag);
                        tile_mac<MT>(sM0, LD, frag, acc);
#pragma unroll
                        for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = 16 * ti + lr;
                                double u = acc[ti][r];
                                if (g >= 1) u += jet(coefs + (size_t)g * Q, cw0 + kk + 4 * r, row);
                                const size_t e = (size_t)(c0 + kk + 4 * r) * BP + row;
                                UB[e] = u;
                                WN[e] += u;
                            }
                    }
                    __syncthreads();
                }
                for (int e = tid; e < nv; e += 256) W[e] = WN[e];
                __syncthreads();
            }

            const int ld = 2 * z;
            double* Hb = a.hess + kn * (int64_t)4 * z * z;
            // (x_i, theta_b) = -(Lambda_b)_i, both triangles
            for (int e = tid; e < n * p; e += 256) {
                const int b = e / n, s = e - b * n;
                const double v = -at_state(W, 1 + b, s);
                Hb[(a.T.x_off + s) + (int64_t)ld * zz_of(b)] = v;
                Hb[zz_of(b) + (int64_t)ld * (a.T.x_off + s)] = v;
            }
            // (theta_a, theta_b) = -<M_k, X_ab>: one wavefront per entry, lanes stride the state in order, then a butterfly
            for (int e = wave; e < P2; e += 4) {
                double s = 0.0;
                for (int st = lane; st < n; st += 64) s += muk[st] * at_state(Y, 1 + p + e, st);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (lane == 0) {
                    const int ra = zz_of(pair_a[e]), rb = zz_of(pair_b[e]);
                    Hb[ra + (int64_t)ld * rb] = -s;
                    if (ra != rb) Hb[rb + (int64_t)ld * ra] = -s;
                }
            }
        }
        __syncthreads();   // the slot is reused by this workgroup's next interval
    }
}

struct TdbkProductArgs {
    KProb P;
    KTdb T;
    KKron K;
    const double* Z;
    const double* w;
    int need;            // 3: J w, 4: J' w
    int64_t count;       // intervals 0 .. count - 1 (products need an unsharded handle)
    double* out;         // need 3: y (the integrator's rows are assigned); need 4: staging [K][n + p]
    double* scratch;
    int64_t scratch_stride;
};

// The product modes: k_tdb_mfma's product modes with a vector replaced by a column group.  A sibling of k_tdb_kron,
// not a mode of it: that kernel's register allocation stays what it is.
//   need 3  groups X | D, D(0) = reshape(w_x(k)); K_D = M0 D + sum_q c_wq U_q with U_q = B_q X and c_w the directional row
//           (tdbm_dir_coef, table row 1 + p); y rows = w_x(k+1) - D(1)
//   need 4  groups X, X_b forward (the Jacobian's pass without Phi~), g_kb = <w_k, X_b(1)>; then Lambda = Phi~' W_k for the one group
//           W_k = reshape(w_k) backward with M0' (no U_q, no jets); [lambda (n), g (p)] staged for launch_tdb_jtv_place
template <int MT>
__global__ void __launch_bounds__(256) k_tdb_kron_product(TdbkProductArgs a) {
    constexpr int BP = 16 * MT;
    constexpr int LD = (MT & 1) ? BP : BP + 16;
    const TdbkLayout L = tdbk_product_layout(a.T, a.K, a.need);
    const int n = a.T.n, z = a.P.z, need = a.need;
    const int bw = a.K.bw, rw = a.K.rw;
    const int cp = L.cp, p = L.p, Q = L.Q, ctot = L.ctot;
    const int cpt = cp / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, kk = lane >> 4;
    constexpr size_t bb = (size_t)BP * BP;
    __shared__ double sM0[BP * LD];
    __shared__ double w_theta[2 * MAX_DRIVES + 2];   // J w: the entries of w at the interval's parameters
    double* S = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    double* Y = S + L.oY;
    double* ACC = S + L.oACC;
    double* TA = S + L.oTA;
    double* TB = S + L.oTB;
    double* U = S + L.oU;          // [Q][cp][BP]: U_q of the X group
    double* UB = S + L.oUB;        // [cp][BP] (J' w)
    double* coefs = S + L.oCoef;   // [rows][Q]

    for (int64_t kn = blockIdx.x; kn < a.count; kn += gridDim.x) {
        const double* zk = a.Z + kn * z;
        const double* zk1 = zk + z;
        const double tk = zk[a.T.t_off], dt = zk[a.P.dt_idx];
        if (need == 3 && tid < p) w_theta[tid] = a.w[kn * z + tdb_param_entry(a.T, z, a.P.dt_idx, tid)];

        // rows 0 .. `rows` - 1 of the table at tau (with `dir` the directional row behind rows 0 .. p), then M0 = sum_q c_q B_q
        // (B_q' in the adjoint) into LDS, in the fixed order q = 0, 1, ...
        auto form_m0 = [&](double tau, int rows, bool dir, const double* __restrict__ B) {
            for (int e = tid; e < rows * Q; e += 256) coefs[e] = tdbm_coef(a.T, zk, zk1, tk, dt, tau, p, e / Q, e % Q);
            __syncthreads();
            if (dir)   // (read by the stage's epilogue, after the barrier below)
                for (int q = tid; q < Q; q += 256) coefs[(size_t)(1 + p) * Q + q] = tdbm_dir_coef(coefs, Q, p, q, w_theta);
            for (int e = tid; e < BP * BP; e += 256) {
                double acc = 0.0;
                for (int q = 0; q < Q; ++q) acc += coefs[q] * B[q * bb + e];
                sM0[(e % BP) + (e / BP) * LD] = acc;
            }
            __syncthreads();
        };
        auto at_state = [&](const double* slab, int g, int e) { const int c = e / bw, i = e - c * bw; return slab[((size_t)g * cp + c) * BP + i]; };

        // initial values: X = reshape(x_k), D = reshape(w_x(k)), everything else (padding included) 0
        for (int e = tid; e < BP * ctot; e += 256) {
            const int c = e / BP, i = e - c * BP;
            double v = 0.0;
            if (i < bw) {
                if (c < rw) v = zk[a.T.x_off + c * bw + i];
                else if (need == 3 && c >= cp && c - cp < rw) v = a.w[kn * z + a.T.x_off + (c - cp) * bw + i];
            }
            Y[e] = v;
        }
        __syncthreads();

        const double h = 1.0 / a.T.substeps;
        for (int step = 0; step < a.T.substeps; ++step) {
            for (int stage = 0; stage < 4; ++stage) {
                const TdbFwdStage sg = tdb_fwd_stage(step, stage, h);
                const double* IN = tdb_fwd_in(stage, Y, TA, TB);
                double* OUT = tdb_fwd_out(stage, Y, TA, TB);
                if (tdb_fwd_new_jets(stage)) form_m0(sg.tau, 1 + p, need == 3, a.K.Bm);
                // U_q = B_q IN for the X group: one wavefront per (q, tile)
                for (int task = wave; task < Q * cpt; task += 4) {
                    const int q = task / cpt, t = task - q * cpt;
                    d4 acc[MT];
                    double frag[4 * MT];
#pragma unroll
                    for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
                    load_frag<MT>(IN, 16 * t, frag);
                    tile_mac<MT>(a.K.Bm + q * bb, BP, frag, acc);
#pragma unroll
                    for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                        for (int r = 0; r < 4; ++r) U[((size_t)q * cp + 16 * t + kk + 4 * r) * BP + 16 * ti + lr] = acc[ti][r];
                }
                __syncthreads();
                // K = M0 IN (+ the group's jet on X), then the RK4 update of this stage: one wavefront per 16-column tile
                for (int task = wave; task < ctot / 16; task += 4) {
                    const int c0 = 16 * task, g = c0 / cp, cw0 = c0 - g * cp;
                    d4 acc[MT];
                    double frag[4 * MT];
#pragma unroll
                    for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
                    load_frag<MT>(IN, c0, frag);
                    tile_mac<MT>(sM0, LD, frag, acc);
                    const double* cf = coefs + (size_t)(need == 3 ? 1 + p : g) * Q;   // J w: M_w; J' w: M_b, b = g - 1
#pragma unroll
                    for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * ti + lr, cw = cw0 + kk + 4 * r;
                            double Kv = acc[ti][r];
                            if (g >= 1) {
                                double s = 0.0;
                                // (every q, zeros of a drive's row included: skipping them on `cf[q] != 0` serialises the loads
                                // and was measured slower)
                                for (int q = 0; q < Q; ++q) s += cf[q] * U[((size_t)q * cp + cw) * BP + row];
                                Kv += s;
                            }
                            const size_t e = (size_t)(c0 + kk + 4 * r) * BP + row;
                            tdb_fwd_update(stage, sg.w_acc, sg.w_tmp, Y[e], Kv, ACC[e], OUT[e]);
                        }
                }
                __syncthreads();
            }
        }

        if (need == 3) {
            // the integrator's rows of J w: w_x(k+1) - D(1), each assigned by one thread
            for (int e = tid; e < n; e += 256) a.out[a.T.row_off + kn * n + e] = a.w[(kn + 1) * z + a.T.x_off + e] - at_state(Y, 1, e);
        } else {
            const double* wk = a.w + a.T.row_off + kn * n;
            double* out = a.out + kn * (int64_t)(n + p);
            // g_kb = <w_k, X_b(1)>: one wavefront per b, lanes stride the state in order, then a butterfly
            for (int b = wave; b < p; b += 4) {
                double s = 0.0;
                for (int st = lane; st < n; st += 64) s += wk[st] * at_state(Y, 1 + b, st);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (lane == 0) out[n + b] = s;
            }
            // Lambda = Phi~' W_k: group 0 of the Hessian's adjoint recursion alone, backward through the steps with M0'
            double* W = TA;
            double* WN = TB;
            double* KB = ACC;
            const int nv = BP * cp;
            for (int e = tid; e < nv; e += 256) {
                const int c = e / BP, i = e - c * BP;
                W[e] = (c < rw && i < bw) ? wk[c * bw + i] : 0.0;
                UB[e] = 0.0;
            }
            __syncthreads();
            for (int step = a.T.substeps - 1; step >= 0; --step) {
                for (int e = tid; e < nv; e += 256) WN[e] = W[e];
                for (int stage = 3; stage >= 0; --stage) {
                    const TdbBwdStage sg = tdb_bwd_stage(step, stage, h);
                    if (tdb_bwd_new_jets(stage)) form_m0(sg.tau, 1, false, a.K.BmT);
                    for (int e = tid; e < nv; e += 256) KB[e] = tdb_bwd_kbar(sg.cw, sg.cu, W[e], UB[e]);
                    __syncthreads();
                    for (int task = wave; task < cpt; task += 4) {   // ubar = M0' kbar
                        const int c0 = 16 * task;
                        d4 acc[MT];
                        double frag[4 * MT];
#pragma unroll
                        for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
                        load_frag<MT>(KB, c0, frag);
                        tile_mac<MT>(sM0, LD, frag, acc);
#pragma unroll
                        for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const size_t e = (size_t)(c0 + kk + 4 * r) * BP + 16 * ti + lr;
                                UB[e] = acc[ti][r];
                                WN[e] += acc[ti][r];
                            }
                    }
                    __syncthreads();
                }
                for (int e = tid; e < nv; e += 256) W[e] = WN[e];
                __syncthreads();
            }
            for (int e = tid; e < n; e += 256) out[e] = at_state(W, 0, e);
        }
        __syncthreads();   // the slot (and w_theta) is reused by this workgroup's next interval
    }
}

}  // namespace

bool tdb_kron_supported(const KTdb& T, const KKron& K) {
    return K.r >= 2 && K.b <= 64 && T.n > 32 && T.n <= 512 && K.bw >= 1 && K.bw <= K.bp && K.bp >= 16 && K.bp <= 64 && K.bp % 16 == 0 &&
           K.rw >= 1 && K.bw * K.rw == T.n && T.substeps >= 1 && T.nmod >= 0 && tdb_table_fits(T.m, T.order, T.nmod) &&
           tdb_num_pairs(tdb_num_params(T.m, T.order)) <= TDBK_MAX_PAIRS;
}

size_t tdb_kron_scratch_doubles(const KTdb& T, const KKron& K, int need) { return tdbk_layout_of(T, K, need).total; }

// MFMA flops of one interval as executed (padding included): per stage the M0 product over all columns and the U_q products; per
// stage time the formation of M0
double tdb_kron_flops(const KTdb& T, const KKron& K, int need) {
    const TdbkLayout L = tdbk_layout_of(T, K, need);
    const double b2 = (double)L.bp * L.bp, S = T.substeps;
    const double form = 2.0 * L.Q * b2;
    const double fwd = 4.0 * 2.0 * b2 * (L.ctot + (double)L.Q * L.ucols) + 3.0 * form;
    double bwd = 0.0;
    if (need == 2) bwd = 4.0 * 2.0 * b2 * (L.wcols + (double)L.Q * L.cp) + 3.0 * form;
    if (need == 4) bwd = 4.0 * 2.0 * b2 * L.wcols + 3.0 * form;   // the one adjoint group: no U_q
    return S * (fwd + bwd);
}

hipError_t launch_tdb_kron(hipStream_t st, const KProb& P, const KTdb& T, const KKron& K, const double* dZ, const double* dmu, int need,
                           int64_t i_lo, int64_t count, double* vals, double* jac, double* hess, double* scratch, size_t scratch_stride,
                           int resident) {
    if (count <= 0) return hipSuccess;
    if (resident < 1 || !tdb_kron_supported(T, K) || tdbk_layout(T, K, need).total > scratch_stride) return hipErrorInvalidValue;
    TdbkArgs a{};
    a.P = P; a.T = T; a.K = K; a.Z = dZ; a.mu = dmu; a.need = need; a.i_lo = i_lo; a.count = count;
    a.vals = vals; a.jac = jac; a.hess = hess; a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride;
    const dim3 grid((unsigned)std::min<int64_t>(count, resident)), block(256);
    switch (K.bp / 16) {
        case 1: hipLaunchKernelGGL(k_tdb_kron<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_tdb_kron<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(k_tdb_kron<3>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(k_tdb_kron<4>, grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_tdb_kron_product(hipStream_t st, const KProb& P, const KTdb& T, const KKron& K, const double* dZ, const double* dw, int need,
                                   double* out, double* scratch, size_t scratch_stride, int resident) {
    if (P.K <= 0) return hipSuccess;
    if ((need != 3 && need != 4) || resident < 1 || !tdb_kron_supported(T, K) || tdbk_product_layout(T, K, need).total > scratch_stride)
        return hipErrorInvalidValue;
    TdbkProductArgs a{};
    a.P = P; a.T = T; a.K = K; a.Z = dZ; a.w = dw; a.need = need; a.count = P.K;
    a.out = out; a.scratch = scratch; a.scratch_stride = (int64_t)scratch_stride;
    const dim3 grid((unsigned)std::min<int64_t>(P.K, resident)), block(256);
    switch (K.bp / 16) {
        case 1: hipLaunchKernelGGL(k_tdb_kron_product<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_tdb_kron_product<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(k_tdb_kron_product<3>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(k_tdb_kron_product<4>, grid, block, 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dto
