// dto_kron.hip -- BilinearIntegrator whose generators are replicated blocks, G_j = I_r (x) B_j (DTO_FLAG_BLOCK_GENERATORS).
//
// The state of such an integrator is an operator in isomorphic coordinates stored column after column, x = vec(X) with X a
// b x r matrix, and exp(dt G(u)) x = vec(exp(A) X) with the b x b matrix A = dt (B_0 + sum_j u_j B_j).  One workgroup per interval
// runs ONE Taylor sweep over "column groups" of b rows each, all sharing the interval's scale dt / (q t):
//
//     p    (r columns, start X)      p_t    = s_t Gu p_{t-1}                              sum = exp(A) X
//     d^j  (r columns, start 0)      d^j_t  = s_t (Gu d^j_{t-1} + B_j p_{t-1})            sum = L(A, dt B_j) X
//     h^ij (r columns, start 0)      h^ij_t = s_t (Gu h^ij_{t-1} + B_i d^j_{t-1} + B_j d^i_{t-1})   (Hessian calls)
//     e    (b columns, start I_b)    e_t    = s_t Gu e_{t-1}                              sum = exp(A)       (Jacobian calls)
//     pa, da^j                       the p / d^j recurrences with Gu', B_j' on M = reshape(mu_k, b, r)      (Hessian calls)
//     pw   (r columns, start W)      the p recurrence on W = reshape(w_x(k), b, r)        sum = exp(A) W     (J w calls)
// (J' w calls run p, d^j and pa with M = reshape(w rows of interval k, b, r): DESIGN 4.19.)
//
// (Gu = B_0 + sum_j u_j B_j, s_t = dt / (q t); q rounds restart the recurrences from the sums: the groups together are the columns
// of the exponential of one block-triangular matrix.)  No n x n matrix is formed: the work per term is 2 b^2 per column and source,
// on v_mfma_f64_16x16x4_f64 with Gu and Gu' in LDS, the shared B_j read through the caches and the terms in a per-workgroup slab.
// Termination is Al-Mohy & Higham's test (two successive terms below 1.1e-16 of the sum, every group) from a step on that depends on
// the interval's own norm bound; budget and rounds come from that bound as in plan_sweep.  Everything a workgroup computes is a
// function of its interval's data alone, every reduction has a fixed order, and the only atomics are integer ones (norm maxima
// as bit patterns in LDS, the statistics words).
//
// Outputs go straight into the caller's vectors at the closed-form positions of the dense generic block (jac_pos / hess_pos): only
// the b x b diagonal blocks of -(I_r (x) E) are written, the share (r-1)/r of each x-block stays the zero the fill put there.
#include "dto_gemm.hip.h"
#include "dto_kernels.h"

namespace dto {

namespace {

constexpr int KRON_MAX_GROUPS = 48;
constexpr double KRON_TOL = 1.1e-16;

struct KronArgs {
    KProb P;
    KBil B;
    KKron K;
    const double* Z;
    const double* mu;
    int need;  // 0 defect, 1 Jacobian block, 2 Hessian block, 3 J w (mu = w, g = y), 4 J' w (mu = w, g = y)
    double* g;
    double* vals;
    double* H;
    double* scratch;
    int64_t stride;
};

struct Group {
    int32_t col0, cols;   // first column in the term slabs, real columns
    int32_t tr;           // 1: transposed matrices (adjoint groups)
    int32_t n_extra;
    int32_t gen[2], src[2];
    double mult[2];
};

__device__ __forceinline__ unsigned long long dbits(double v) { return (unsigned long long)__double_as_longlong(fabs(v)); }

// acc[ti] += Mat[16 ti + lr][k] * frag[k] over this lane's k range (lane l: lr = l & 15, kk = l >> 4, k = kk KS + s): the product is
// issued transposed (dto_gemm.hip.h), so acc[ti][reg] is row 16 ti + lr, column kk + 4 reg of the 16-column tile.
template <int MT>
__device__ __forceinline__ void tile_mac(const double* __restrict__ mat, int ld, const double (&frag)[4 * MT], double scale, d4 (&acc)[MT]) {
    const int lr = threadIdx.x & 15, kk = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int s = 0; s < 4 * MT; ++s) {
        const double bf = frag[s] * scale;
        const double* col = mat + (size_t)(kk * 4 * MT + s) * ld + lr;
#pragma unroll
        for (int ti = 0; ti < MT; ++ti) acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf, col[16 * ti], acc[ti], 0, 0, 0);
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
__global__ void __launch_bounds__(256) k_kron(KronArgs a) {
    constexpr int BP = 16 * MT;
    constexpr int LD = (MT & 1) ? BP : BP + 16;   // LD mod 32 == 16: the two k's of a 32-lane LDS read land on disjoint bank halves
    constexpr int KS = 4 * MT;
    extern __shared__ double kron_lds[];   // Gu, Gu' (BP x LD each; 80 KB at 64 rows: dynamic, opted into by kron_prepare)
    double* sGu = kron_lds;
    double* sGuT = kron_lds + BP * LD;
    __shared__ Group grp[KRON_MAX_GROUPS];
    __shared__ unsigned long long tn[2][KRON_MAX_GROUPS], sn[KRON_MAX_GROUPS];
    __shared__ double red[8];
    __shared__ int plan[4];   // q, d_ub, tc

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, kk = lane >> 4;
    const int m = a.B.m, n = a.B.n, z = a.P.z, need = a.need;
    const int bw = a.K.bw, rw = a.K.rw, bf_ = a.K.b;
    const int cp = (rw + 15) & ~15;
    const int64_t kl = blockIdx.x, kn = a.P.kn_lo + kl;
    const double* zk = a.Z + kn * z;
    const double dt = zk[a.P.dt_idx];
    const int P2 = m * (m + 1) / 2;
    const int G = need == 0 ? 1 : (need == 2 ? 2 + 2 * m + P2 : m + 2);
    // Jacobian calls: the e group (J w: pw in its place); Hessian and J' w calls: the first adjoint group
    const int g_e = m + 1, g_pa = need == 4 ? m + 1 : 1 + m + P2;
    const bool adj = need == 2 || need == 4;
    const int ctot = (G - 1) * cp + (need == 1 ? BP : cp);
    double* T0 = a.scratch + kl * a.stride;
    double* T1 = T0 + (size_t)ctot * BP;
    double* S = T1 + (size_t)ctot * BP;
    double* AUX = S + (size_t)ctot * BP;    // [(m + 3)][cp][BP]: products outside the sweep

    // ---- group table
    if (tid == 0) {
        for (int g = 0; g < G; ++g) grp[g] = Group{g * cp, rw, 0, 0, {0, 0}, {0, 0}, {0.0, 0.0}};
        if (need >= 1)
            for (int j = 1; j <= m; ++j) { grp[j].n_extra = 1; grp[j].gen[0] = j; grp[j].src[0] = 0; grp[j].mult[0] = 1.0; }
        if (need == 1) grp[g_e].cols = bw;
        if (adj) grp[g_pa].tr = 1;
        if (need == 2) {
            int g = 1 + m;
            for (int i = 1; i <= m; ++i)
                for (int j = i; j <= m; ++j, ++g) {
                    if (i == j) { grp[g].n_extra = 1; grp[g].gen[0] = i; grp[g].src[0] = i; grp[g].mult[0] = 2.0; }
                    else { grp[g].n_extra = 2; grp[g].gen[0] = i; grp[g].src[0] = j; grp[g].gen[1] = j; grp[g].src[1] = i; grp[g].mult[0] = grp[g].mult[1] = 1.0; }
                }
            for (int j = 1; j <= m; ++j) {
                Group& d = grp[g_pa + j];
                d.tr = 1; d.n_extra = 1; d.gen[0] = j; d.src[0] = g_pa; d.mult[0] = 1.0;
            }
        }
    }
    // ---- Gu and Gu' (padded rows and columns of the B_j are zero)
    for (int e = tid; e < BP * BP; e += 256) {
        const int i = e % BP, k = e / BP;
        double v = a.K.Bm[e];
        for (int j = 1; j <= m; ++j) v += zk[a.B.u_off + j - 1] * a.K.Bm[(size_t)j * BP * BP + e];
        sGu[i + k * LD] = v;
        sGuT[k + i * LD] = v;
    }
    // ---- start vectors: term 0 and sum
    const double* muk = adj ? a.mu + a.B.row_off + kn * n : nullptr;   // mu_k, or the rows of interval k of w (J' w)
    const double* wxk = need == 3 ? a.mu + kn * z + a.B.x_off : nullptr; // w_x(k) (J w)
    for (int e = tid; e < ctot * BP; e += 256) {
        const int c = e / BP, i = e - c * BP;
        const int g = min(c / cp, G - 1), cw = c - g * cp;
        double v = 0.0;
        if (i < bw) {
            if (g == 0 && cw < rw) v = zk[a.B.x_off + cw * bw + i];
            else if (need == 1 && g == g_e && cw < bw) v = cw == i ? 1.0 : 0.0;
            else if (adj && g == g_pa && cw < rw) v = muk[cw * bw + i];
            else if (need == 3 && g == g_e && cw < rw) v = wxk[cw * bw + i];
        }
        T0[e] = v;
        S[e] = v;
    }
    __syncthreads();
    // ---- step budget from the interval's own norm bound (plan_sweep's rule on max(||A||_1, ||A||_inf))
    {
        double cs = 0.0, rs = 0.0;
        if (tid < BP)
            for (int k = 0; k < BP; ++k) { cs += fabs(sGu[k + tid * LD]); rs += fabs(sGuT[k + tid * LD]); }
        double v = fmax(cs, rs);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
        if (lane == 0) red[wave] = v;
        __syncthreads();
        if (tid == 0) {
            const double beta = fabs(dt) * fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
            int q = 1, d_ub = 30, tc = 14;
            if (beta == beta && beta <= 1e6) {
                q = max(1, (int)ceil(beta / 9.0));
                const double br = beta / q;
                int t = 8;
                double term = 1.0;
                for (int i = 1; i <= t; ++i) term *= br / i;
                while (term > 1e-19 && t < 200) { ++t; term *= br / t; }
                d_ub = t + 6;
                tc = min(d_ub / 2 - 1, max(2, (int)ceil(br) + 4));
            }
            plan[0] = q; plan[1] = d_ub; plan[2] = tc;
        }
        __syncthreads();
    }
    const int q = plan[0], d_ub = plan[1], tc = plan[2];

    // out tile (group g, column tile tj) = scale * (Mat src + extras); Mat = Gu / Gu' from LDS, extras B_j / B_j' through the caches
    auto product = [&](const Group& gd, int tj, const double* src, d4 (&acc)[MT]) {
        double frag[KS];
#pragma unroll
        for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
        load_frag<MT>(src, gd.col0 + 16 * tj, frag);
        tile_mac<MT>(gd.tr ? sGuT : sGu, LD, frag, 1.0, acc);
        for (int x = 0; x < gd.n_extra; ++x) {
            load_frag<MT>(src, grp[gd.src[x]].col0 + 16 * tj, frag);
            tile_mac<MT>((gd.tr ? a.K.BmT : a.K.Bm) + (size_t)gd.gen[x] * BP * BP, BP, frag, gd.mult[x], acc);
        }
    };
    // number of wave tasks: one per (group, column tile)
    const int tiles_main = cp / 16, tiles_e = BP / 16;
    const int n_tasks = (G - 1) * tiles_main + (need == 1 ? tiles_e : tiles_main);
    auto task_of = [&](int task, int& g, int& tj) { g = min(task / tiles_main, G - 1); tj = task - g * tiles_main; };

    // ---- products on the start vectors (Hessian calls): AUX[0] = Gu' M, AUX[j] = B_j' M
    if (need == 2) {
        for (int task = wave; task < (1 + m) * tiles_main; task += 4) {
            const int j = task / tiles_main, tj = task - j * tiles_main;
            d4 acc[MT];
            double frag[KS];
#pragma unroll
            for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
            load_frag<MT>(T0, grp[g_pa].col0 + 16 * tj, frag);
            if (j == 0) tile_mac<MT>(sGuT, LD, frag, 1.0, acc);
            else tile_mac<MT>(a.K.BmT + (size_t)j * BP * BP, BP, frag, 1.0, acc);
#pragma unroll
            for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) AUX[((size_t)j * cp + 16 * tj + kk + 4 * r) * BP + 16 * ti + lr] = acc[ti][r];
        }
    }

    // ---- the sweep
    double* cur = T0;
    double* nxt = T1;
    int failed = 0, used = 0;
    for (int round = 0; round < q; ++round) {
        bool done = false;
        int t = 1;
        for (; t <= d_ub && !done; ++t) {
            const int pb = t & 1;
            if (tid < G) { tn[pb][tid] = 0ull; sn[tid] = 0ull; }
            __syncthreads();
            const double scale = dt / ((double)q * (double)t);
            for (int task = wave; task < n_tasks; task += 4) {
                int g, tj;
                task_of(task, g, tj);
                const Group& gd = grp[g];   // (read in place: a private copy indexed by the extra's number would live in scratch)
                d4 acc[MT];
                product(gd, tj, cur, acc);
                double tmax = 0.0, smax = 0.0;
#pragma unroll
                for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const size_t at = (size_t)(gd.col0 + 16 * tj + kk + 4 * r) * BP + 16 * ti + lr;
                        const double v = scale * acc[ti][r];
                        const double s = S[at] + v;
                        nxt[at] = v;
                        S[at] = s;
                        tmax = fmax(tmax, fabs(v));
                        smax = fmax(smax, fabs(s));
                        if (v != v) tmax = INFINITY;   // a NaN term never passes the test
                    }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { tmax = fmax(tmax, __shfl_xor(tmax, o, 64)); smax = fmax(smax, __shfl_xor(smax, o, 64)); }
                if (lane == 0) { atomicMax(&tn[pb][g], dbits(tmax)); atomicMax(&sn[g], dbits(smax)); }
            }
            __syncthreads();
            if (t >= tc) {
                done = true;
                for (int g = 0; g < G; ++g) {
                    const double t1 = __longlong_as_double((long long)tn[pb][g]), t0 = __longlong_as_double((long long)tn[pb ^ 1][g]);
                    const double s = __longlong_as_double((long long)sn[g]);
                    if (!(t1 + t0 <= KRON_TOL * s)) done = false;
                }
            }
            double* sw = cur; cur = nxt; nxt = sw;
            __syncthreads();
        }
        used = max(used, t - 1);
        if (!done) failed = 1;
        if (round + 1 < q) {   // the next round starts from the sums
            for (int e = tid; e < ctot * BP; e += 256) cur[e] = S[e];
            __syncthreads();
        }
    }
    if (tid == 0) {
        if (failed) atomicAdd(&a.K.stats[0], 1);
        atomicMax(&a.K.stats[1], used + 1);
    }

    // ---- products on the sums: Gu exp(A) X (Jacobian and Hessian calls), Gu' exp(A') M (Hessian calls)
    const int aux_gy = need == 2 ? m + 1 : 0, aux_xdt = m + 2;
    if (need >= 1) {
        const int n_post = (need == 2 ? 2 : 1) * tiles_main;
        for (int task = wave; task < n_post; task += 4) {
            const int which = task / tiles_main, tj = task - which * tiles_main;
            d4 acc[MT];
            double frag[KS];
#pragma unroll
            for (int ti = 0; ti < MT; ++ti) acc[ti] = d4{0.0, 0.0, 0.0, 0.0};
            load_frag<MT>(S, (which ? grp[g_pa].col0 : 0) + 16 * tj, frag);
            tile_mac<MT>(which ? sGuT : sGu, LD, frag, 1.0, acc);
            const int ag = which ? aux_xdt : aux_gy;
#pragma unroll
            for (int ti = 0; ti < MT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) AUX[((size_t)ag * cp + 16 * tj + kk + 4 * r) * BP + 16 * ti + lr] = acc[ti][r];
        }
        __syncthreads();
    }

    // ---- outputs.  State index of (row i, replica c) of the working block: c bw + i
    auto at_state = [&](const double* slab, int col0, int e) { const int c = e / bw, i = e - c * bw; return slab[(size_t)(col0 + c) * BP + i]; };
    if (need == 0) {
        for (int e = tid; e < n; e += 256) a.g[a.B.lrow_off + kl * n + e] = zk[z + a.B.x_off + e] - at_state(S, 0, e);
        return;
    }
    if (need == 1) {
        // -(I_r (x) E): the diagonal b x b blocks only (finest block size: what lies outside them is a structural zero)
        const double* E = S + (size_t)grp[g_e].col0 * BP;
        for (int e = tid; e < n * bf_; e += 256) {
            const int j = e / bf_, i = e - j * bf_;        // state column j, row i of its finest block
            const int blk = j / bf_;
            const int jw = j % bw, iw = (blk * bf_) % bw + i;  // position inside the working block
            a.vals[jac_pos(a.P, a.P.colptr, kn, a.B.x_off + j, a.B.pre, n, 1, blk * bf_ + i)] = -E[(size_t)jw * BP + iw];
        }
        for (int j = 1; j <= m; ++j) {
            const int64_t base = jac_pos(a.P, a.P.colptr, kn, a.B.u_off + j - 1, a.B.pre, n, 1, 0);
            for (int e = tid; e < n; e += 256) a.vals[base + e] = -at_state(S, grp[j].col0, e);
        }
        const int64_t base = jac_pos(a.P, a.P.colptr, kn, a.P.dt_idx, a.B.pre, n, 1, 0);
        for (int e = tid; e < n; e += 256) a.vals[base + e] = -at_state(AUX, aux_gy * cp, e);
        return;
    }
    if (need == 3) {
        // rows of interval kn of J w: w_x(k+1) - exp(A) W - sum_j w_uj d^j - w_dt Gu exp(A) X, one writer per row
        const double* wk = a.mu + kn * z;
        const double wdt = wk[a.P.dt_idx];
        for (int e = tid; e < n; e += 256) {
            double v = wk[z + a.B.x_off + e] - at_state(S, grp[g_e].col0, e) - wdt * at_state(AUX, aux_gy * cp, e);
            for (int j = 1; j <= m; ++j) v -= wk[a.B.u_off + j - 1] * at_state(S, grp[j].col0, e);
            a.g[a.B.row_off + kn * n + e] = v;
        }
        return;
    }
    if (need == 4) {
        // entries of knot kn of J' w (y is zero-filled, launches follow each other on the stream: one writer per entry and launch).
        // The +w_{k-1} of the last knot, which owns no interval, is k_kron_jtv_tail's.
        double* yk = a.g + kn * z;
        for (int e = tid; e < n; e += 256)
            yk[a.B.x_off + e] += (kn >= 1 ? a.mu[a.B.row_off + (kn - 1) * n + e] : 0.0) - at_state(S, grp[g_pa].col0, e);
        for (int sc = wave; sc <= m; sc += 4) {   // u_j = -<W, d^j>, dt = -<W, Gu exp(A) X>: as the Hessian's scalar blocks
            double s = 0.0;
            if (sc < m) for (int e = lane; e < n; e += 64) s += muk[e] * at_state(S, grp[1 + sc].col0, e);
            else for (int e = lane; e < n; e += 64) s += muk[e] * at_state(AUX, aux_gy * cp, e);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) yk[sc < m ? a.B.u_off + sc : a.P.dt_idx] -= s;
        }
        return;
    }
    // Hessian of mu_k' delta_k (per replica, summed over the replicas in state order).  Every entry has one writer.
    auto hadd = [&](int c1, int c2, double v) { a.H[hess_pos(a.P, kn, c1 < c2 ? c1 : c2, c1 < c2 ? c2 : c1)] += v; };
    for (int e = tid; e < n; e += 256) {
        for (int j = 1; j <= m; ++j) hadd(a.B.x_off + e, a.B.u_off + j - 1, -at_state(S, grp[g_pa + j].col0, e));
        hadd(a.B.x_off + e, a.P.dt_idx, -at_state(AUX, aux_xdt * cp, e));
    }
    // scalar blocks: one wavefront per entry, lanes stride the state in order, then a butterfly
    const int n_scal = P2 + m + 1;
    for (int sc = wave; sc < n_scal; sc += 4) {
        double s = 0.0;
        int c1, c2;
        if (sc < P2) {          // (u_i, u_j) = -<M, h^ij>
            int rem = sc, i = 0;
            while (rem >= m - i) { rem -= m - i; ++i; }
            c1 = a.B.u_off + i; c2 = a.B.u_off + i + rem;
            for (int e = lane; e < n; e += 64) s += muk[e] * at_state(S, grp[1 + m + sc].col0, e);
        } else if (sc < P2 + m) {   // (u_j, dt) = -(<B_j' M, exp(A) X> + <Gu' M, d^j>)
            const int j = sc - P2 + 1;
            c1 = a.B.u_off + j - 1; c2 = a.P.dt_idx;
            for (int e = lane; e < n; e += 64) s += at_state(AUX, j * cp, e) * at_state(S, 0, e) + at_state(AUX, 0, e) * at_state(S, grp[j].col0, e);
        } else {                    // (dt, dt) = -<Gu' M, Gu exp(A) X>
            c1 = c2 = a.P.dt_idx;
            for (int e = lane; e < n; e += 64) s += at_state(AUX, 0, e) * at_state(AUX, aux_gy * cp, e);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) hadd(c1, c2, -s);
    }
}

// identity of the z_{k+1} half (rows of interval kn - 1 in the state columns of knot kn)
__global__ void k_kron_identity(KProb P, KBil B, double* __restrict__ vals) {
    const int64_t kn = P.kn_lo + blockIdx.x;
    if (kn < 1) return;
    for (int r = threadIdx.x; r < B.n; r += blockDim.x) vals[jac_pos(P, P.colptr, kn, B.x_off + r, B.pre, B.n, 0, r)] = 1.0;
}

// J' w: +w_{k-1} into the state entries of the first owned knot past the owned intervals (the last knot of an unsharded handle)
__global__ void k_kron_jtv_tail(KProb P, KBil B, const double* __restrict__ w, double* __restrict__ y) {
    const int64_t kn = P.kn_lo + P.n_int;
    if (kn < 1 || kn >= P.N || kn >= P.kn_lo + P.n_knots) return;
    for (int r = threadIdx.x; r < B.n; r += blockDim.x) y[kn * P.z + B.x_off + r] += w[B.row_off + (kn - 1) * B.n + r];
}

}  // namespace

hipError_t kron_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_kron<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 64 * 80 * 8);
}

int kron_groups(int m, int need) { return need == 0 ? 1 : (need == 2 ? 2 + 2 * m + m * (m + 1) / 2 : m + 2); }

bool kron_supported(const KKron& K, int m, bool hessian) {
    return K.bw >= 1 && K.bp >= 16 && K.bp <= 64 && K.bp % 16 == 0 && K.bw <= K.bp && kron_groups(m, hessian ? 2 : 1) <= KRON_MAX_GROUPS;
}

size_t kron_scratch_doubles(const KKron& K, int m, int need) {
    const size_t cp = ((size_t)K.rw + 15) & ~(size_t)15;
    const size_t G = (size_t)kron_groups(m, need);
    const size_t ctot = (G - 1) * cp + (need == 1 ? (size_t)K.bp : cp);
    return (3 * ctot + ((size_t)m + 3) * cp) * (size_t)K.bp;
}

hipError_t launch_kron(hipStream_t st, const KProb& P, const KBil& B, const KKron& K, const double* dZ, const double* dmu, int need,
                       double* g, double* vals, double* H, double* scratch, size_t stride) {
    if (need == 1 && P.n_knots > 0) hipLaunchKernelGGL(k_kron_identity, dim3((unsigned)P.n_knots), dim3(P.debug_bad_launch ? 4096 : 256), 0, st, P, B, vals);
    if (need == 4 && P.n_knots > 0) hipLaunchKernelGGL(k_kron_jtv_tail, dim3(1), dim3(P.debug_bad_launch ? 4096 : 256), 0, st, P, B, dmu, g);
    if (P.n_int <= 0) return hipGetLastError();
    KronArgs a{};
    a.P = P; a.B = B; a.K = K; a.Z = dZ; a.mu = dmu; a.need = need; a.g = g; a.vals = vals; a.H = H;
    a.scratch = scratch; a.stride = (int64_t)stride;
    const dim3 grid((unsigned)P.n_int), block(P.debug_bad_launch ? 4096 : 256);
    auto lds = [](int mt) { const int bp = 16 * mt; return (size_t)2 * bp * ((mt & 1) ? bp : bp + 16) * sizeof(double); };
    switch (K.bp / 16) {
        case 1: hipLaunchKernelGGL(k_kron<1>, grid, block, lds(1), st, a); break;
        case 2: hipLaunchKernelGGL(k_kron<2>, grid, block, lds(2), st, a); break;
        case 3: hipLaunchKernelGGL(k_kron<3>, grid, block, lds(3), st, a); break;
        case 4: hipLaunchKernelGGL(k_kron<4>, grid, block, lds(4), st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dto
