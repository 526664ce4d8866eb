// dto_precond.hip -- kernels of the L-BFGS-preconditioned truncated-Newton step (dto_preconditioned_newton_step, dto_newton_precondition
// and their _dev forms; the pair store, the preparation, the application and the loop: dto_precond_plan.h; include/dto_engine.h,
// "Preconditioned truncated-Newton step").  The shape is dto_newton_box.hip's: the entry states and the curvature pass ARE that file's
// launches (k_newton_box_start, k_newton_box_curv, which read no scalar), and what is here are the passes that know the pairs.
//
//   k_precond_states  the entry states of dto_newton_precondition: free where the entry is independent and the mask leaves it
//   k_precond_gram    the masked Gram pass: per chunk the partial sums of SY_ij, YY_ij (i <= j) and SS_ii over F0; a wavefront keeps
//                     its four entries of s_j, y_j in registers and walks the pairs i <= j, whose lines come from L2
//   k_precond_prep    one workgroup: stage 2 of the Gram entries, then one thread runs precond_prepare (admission, gamma, R, M)
//   k_precond_dots    the multi-dot pass on its own (behind the start, and for dto_newton_precondition): r once, every s_k, y_k once
//   k_precond_comb    every workgroup: stage 2 of the 2 cnt dots, the two triangular solves by one thread (precond_coeffs, the prepared
//                     system staged in LDS), then z on its chunks and the partial sums of r . z
//   k_precond_step    k_newton_box_step with rz in rr's place in the decision, the harvest copy of (d, w) into the other bank, and the
//                     multi-dot pass on the r it has just updated (so an application is this launch's tail and k_precond_comb)
//   k_precond_dir     k_newton_box_dir with rz in beta, d = beta * d - z, the fallback, the running counts, `info` [16] and the
//                     trace's last columns
// A wavefront owns a chunk of NEWTON_CHUNK entries (lane-to-entry map i = 256 b + l + 64 t), a workgroup sixteen chunks in a row; every
// vector read is 512 contiguous bytes per wavefront and t.  Stage 2 of every reduction is done by every workgroup itself from L2.  What
// a launch reads of the scalars is never written in that launch.  No atomics; wavefront shuffles; plain 8-byte loads and stores.
#include <algorithm>

#include "dto_kernels.h"
#include "dto_precond_plan.h"
#include "dto_reduced_plan.h"

namespace dto {

namespace {

constexpr int PRECOND_WAVES = 16;
constexpr int PRECOND_THREADS = PRECOND_WAVES * NEWTON_LANES;   // 1024
constexpr int PER_LANE = NEWTON_CHUNK / NEWTON_LANES;           // 4

__device__ __forceinline__ double pc_tree64(double a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = newton_add(a, __shfl_down(a, off, 64));
    return a;
}
__device__ __forceinline__ double pc_mintree64(double a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = newton_box_min(a, __shfl_down(a, off, 64));
    return a;
}

// the lane's part of a chunk dot of two register quadruples, then the tree; lane 0 holds the chunk sum
__device__ __forceinline__ double pc_dot4(const double (&x)[PER_LANE], const double (&y)[PER_LANE], int live) {
    double a = 0.0;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t)
        if (t < live) a = newton_add(a, newton_mul(x[t], y[t]));
    return pc_tree64(a);
}

// the lane's entries of a chunk: `live` of them, i = base + 64 t
struct Chunk {
    int lane;
    int64_t b, base;
    int live;
};
__device__ __forceinline__ Chunk pc_chunk(const KNewtonBox& A) {
    Chunk c;
    c.lane = threadIdx.x % NEWTON_LANES;
    c.b = (int64_t)blockIdx.x * PRECOND_WAVES + threadIdx.x / NEWTON_LANES;
    c.base = c.b * NEWTON_CHUNK + c.lane;
    const int64_t end = c.b < A.nb ? min((c.b + 1) * NEWTON_CHUNK, A.n) : 0;
    const int64_t left = end - c.base;
    c.live = left <= 0 ? 0 : (int)min((int64_t)PER_LANE, (left + NEWTON_LANES - 1) / NEWTON_LANES);
    return c;
}

__device__ __forceinline__ void pc_load_masked(const double* x, const Chunk& c, unsigned fm, double (&o)[PER_LANE]) {
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) o[t] = (fm >> t & 1u) ? x[c.base + NEWTON_LANES * t] : 0.0;
}

__device__ __forceinline__ const double* pc_pair(const double* bank, const KPrecond& A, int k) {
    return bank + (size_t)precond_slot(A.head, k, A.m) * (size_t)A.B.n;
}

// the multi-dot pass of one chunk: rf the lane's entries of r on F (0 elsewhere), fm the lane's free bits
__device__ __forceinline__ void pc_dots_chunk(const KPrecond& A, const Chunk& c, unsigned fm, const double (&rf)[PER_LANE]) {
    for (int k = 0; k < A.cnt; ++k) {
        double s[PER_LANE], y[PER_LANE];
        pc_load_masked(pc_pair(A.S, A, k), c, fm, s);
        pc_load_masked(pc_pair(A.Y, A, k), c, fm, y);
        const double u = pc_dot4(s, rf, c.live), v = pc_dot4(y, rf, c.live);
        if (c.lane == 0) {
            A.uv[(size_t)k * A.B.nb + c.b] = u;
            A.uv[(size_t)(A.cnt + k) * A.B.nb + c.b] = v;
        }
    }
}

// stage 2 of the listed slots of `part` by the first `count` wavefronts of the workgroup; NBX_TMIN is a minimum
__device__ __forceinline__ void pc_combine(const KNewtonBox& A, const int* slots, int count, double* out) {
    const int wave = threadIdx.x / NEWTON_LANES, lane = threadIdx.x % NEWTON_LANES;
    if (wave < count) {
        const int slot = slots[wave];
        const double* P = A.part + (size_t)slot * A.nb;
        double t;
        if (slot == NBX_TMIN) {
            double m = newton_box_inf();
            for (int64_t b = lane; b < A.nb; b += NEWTON_LANES) m = newton_box_min(m, P[b]);
            t = pc_mintree64(m);
        } else {
            t = pc_tree64(newton_lane_sum(P, A.nb, lane));
        }
        if (lane == 0) out[wave] = t;
    }
    __syncthreads();
}

__device__ __forceinline__ double pc_lo(const KNewtonBox& A, int64_t i) { return A.lo ? A.lo[i] : -newton_box_inf(); }
__device__ __forceinline__ double pc_hi(const KNewtonBox& A, int64_t i) { return A.hi ? A.hi[i] : newton_box_inf(); }

__global__ void __launch_bounds__(PRECOND_THREADS) k_precond_states(KReduced R, KNewtonBox A) {
    const Chunk c = pc_chunk(A);
    for (int t = 0; t < c.live; ++t) {
        const int64_t i = c.base + NEWTON_LANES * t;
        A.es[i] = (unsigned char)(!reduced_is_dependent(R, i) && (!A.mask || A.mask[i] != 0.0) ? NBOX_FREE : NBOX_FIXED);
    }
}

__global__ void __launch_bounds__(PRECOND_THREADS) k_precond_gram(KPrecond A) {
    const Chunk c = pc_chunk(A.B);
    if (c.b >= A.B.nb) return;   // (uniform in a wavefront)
    unsigned fm = 0;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t)
        if (t < c.live && A.B.es[c.base + NEWTON_LANES * t] == NBOX_FREE) fm |= 1u << t;
    const int T = A.cnt * (A.cnt + 1) / 2;
    const size_t nb = (size_t)A.B.nb;
    for (int j = 0; j < A.cnt; ++j) {
        double sj[PER_LANE], yj[PER_LANE];
        pc_load_masked(pc_pair(A.S, A, j), c, fm, sj);
        pc_load_masked(pc_pair(A.Y, A, j), c, fm, yj);
        for (int i = 0; i <= j; ++i) {
            double si[PER_LANE], yi[PER_LANE];
            pc_load_masked(pc_pair(A.S, A, i), c, fm, si);
            pc_load_masked(pc_pair(A.Y, A, i), c, fm, yi);
            const double sy = pc_dot4(si, yj, c.live), yy = pc_dot4(yi, yj, c.live);
            if (c.lane == 0) {
                A.gram[(size_t)precond_tri(i, j) * nb + c.b] = sy;
                A.gram[(size_t)(T + precond_tri(i, j)) * nb + c.b] = yy;
            }
        }
        const double ss = pc_dot4(sj, sj, c.live);
        if (c.lane == 0) A.gram[(size_t)(2 * T + j) * nb + c.b] = ss;
    }
}

__global__ void __launch_bounds__(PRECOND_THREADS) k_precond_prep(KPrecond A) {
    __shared__ double G[PRECOND_GRAM_MAX];
    const int wave = threadIdx.x / NEWTON_LANES, lane = threadIdx.x % NEWTON_LANES;
    const int count = precond_gram_count(A.cnt);
    for (int q = wave; q < count; q += PRECOND_WAVES) {
        const double t = pc_tree64(newton_lane_sum(A.gram + (size_t)q * A.B.nb, A.B.nb, lane));
        if (lane == 0) G[q] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) precond_prepare(A.cnt, G, A.pc);
}

// whether the preconditioner is on for the application behind iteration j (j = 0: behind the start)
__device__ __forceinline__ bool pc_on(const KPrecond& A, int j) {
    if (A.cnt == 0) return false;
    return j == 0 ? A.pc[PPC_NADM] > 0.0 : A.B.state[NPS_ACTIVE + (j - 1) % 2] != 0.0;
}

__global__ void __launch_bounds__(PRECOND_THREADS) k_precond_dots(KPrecond A, const double* r) {
    const Chunk c = pc_chunk(A.B);
    if (c.b >= A.B.nb) return;
    unsigned fm = 0;
    double rf[PER_LANE];
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const bool f = t < c.live && A.B.es[c.base + NEWTON_LANES * t] == NBOX_FREE;
        fm |= (f ? 1u : 0u) << t;
        rf[t] = f ? r[c.base + NEWTON_LANES * t] : 0.0;
    }
    pc_dots_chunk(A, c, fm, rf);
}

// z from r; j selects the `on` flag (see pc_on).  r and z: the step's own, or a column of dto_newton_precondition.
__global__ void __launch_bounds__(PRECOND_THREADS) k_precond_comb(KPrecond A, const double* r, double* z, int j) {
    __shared__ double pc[PRECOND_PC];
    __shared__ double uv[2 * PRECOND_MAX_PAIRS], cc[2 * PRECOND_MAX_PAIRS];
    const bool on = pc_on(A, j);
    int q = 0;
    if (on) {
        const int wave = threadIdx.x / NEWTON_LANES, lane = threadIdx.x % NEWTON_LANES;
        for (int e = threadIdx.x; e < PRECOND_PC; e += PRECOND_THREADS) pc[e] = A.pc[e];
        for (int k = wave; k < 2 * A.cnt; k += PRECOND_WAVES) {
            const double t = pc_tree64(newton_lane_sum(A.uv + (size_t)k * A.B.nb, A.B.nb, lane));
            if (lane == 0) uv[k] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) precond_coeffs(pc, uv, uv + A.cnt, cc, cc + PRECOND_MAX_PAIRS);
        __syncthreads();
        q = (int)pc[PPC_NADM];
    }
    const Chunk c = pc_chunk(A.B);
    if (c.b >= A.B.nb) return;
    unsigned fm = 0;
    double rf[PER_LANE], zz[PER_LANE];
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const bool f = t < c.live && A.B.es[c.base + NEWTON_LANES * t] == NBOX_FREE;
        fm |= (f ? 1u : 0u) << t;
        rf[t] = f ? r[c.base + NEWTON_LANES * t] : 0.0;
        zz[t] = rf[t];
    }
    if (q > 0) {
        const double gamma = pc[PPC_GAMMA];
        double a1[PER_LANE] = {0.0, 0.0, 0.0, 0.0}, a2[PER_LANE] = {0.0, 0.0, 0.0, 0.0};
        for (int e = 0; e < q; ++e) {
            const int k = (int)pc[PPC_IDX + e];
            double s[PER_LANE], y[PER_LANE];
            pc_load_masked(pc_pair(A.S, A, k), c, fm, s);
            pc_load_masked(pc_pair(A.Y, A, k), c, fm, y);
            const double c1 = cc[e], c2 = cc[PRECOND_MAX_PAIRS + e];
#pragma unroll
            for (int t = 0; t < PER_LANE; ++t) {
                a1[t] = precond_acc(a1[t], c1, s[t]);
                a2[t] = precond_acc(a2[t], c2, y[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < PER_LANE; ++t) zz[t] = (fm >> t & 1u) ? precond_entry(gamma, rf[t], a1[t], a2[t]) : 0.0;
    }
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t)
        if (t < c.live) z[c.base + NEWTON_LANES * t] = zz[t];
    const double rz = pc_dot4(rf, zz, c.live);
    if (c.lane == 0) A.B.part[(size_t)NPX_RZ * A.B.nb + c.b] = rz;
}

__global__ void __launch_bounds__(PRECOND_THREADS) k_precond_step(KPrecond K, int j) {
    const KNewtonBox& A = K.B;
    __shared__ double dots[5];   // kappa, d . d, p . d, p . p, tau_box
    const int slots[5] = {NBX_KAPPA, NBX_DD, NBX_PD, NBX_PP, NBX_TMIN};
    pc_combine(A, slots, 5, dots);
    const double kappa = dots[0], dd = dots[1], tau_box = dots[4];
    const NewtonDecision D = newton_box_decide(kappa, dd, dots[2], dots[3], A.state[NPS_RZ + (j - 1) % 2], A.radius, tau_box, j);
    const bool took = K.harvest && precond_takes(kappa);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.state[NPS_DECISION] = (double)D.status;
        A.state[NPS_S] = D.s;
        A.state[NPS_KAPPA] = kappa;
        A.state[NPS_DD] = dd;
        A.state[NPS_TOOK] = took ? 1.0 : 0.0;
        if (A.trace) {
            double* row = A.trace + PRECOND_TRACE * (size_t)(j - 1);
            row[0] = kappa; row[1] = dd; row[2] = D.s; row[4] = tau_box;
        }
    }
    const Chunk c = pc_chunk(A);
    if (c.b >= A.nb) return;
    double *hs = nullptr, *hy = nullptr;
    if (took) {
        const size_t slot = (size_t)((int64_t)A.state[NPS_TAKEN + (j - 1) % 2] % K.m);
        hs = K.HS + slot * (size_t)A.n;
        hy = K.HY + slot * (size_t)A.n;
    }
    const bool move = D.status != NEWTON_NOT_FINITE;
    double rr = 0.0, pg = 0.0, pr = 0.0, pp = 0.0, nhit = 0.0, nfree = 0.0;
    unsigned fm = 0;
    double rf[PER_LANE] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        if (t >= c.live) continue;
        const int64_t i = c.base + NEWTON_LANES * t;
        int s = A.es[i];
        double p = A.p[i], r = A.r[i];
        const bool in_f = s == NBOX_FREE;
        const double z = in_f || A.zp ? A.Z[i] : 0.0, lo = in_f || A.zp ? pc_lo(A, i) : 0.0, hi = in_f || A.zp ? pc_hi(A, i) : 0.0;
        if (move || took) {
            const double d = A.d[i], w = A.w[i];
            if (took) {
                hs[i] = d;
                hy[i] = w;
            }
            if (move) {
                const double tb = in_f ? newton_box_breakpoint(z, p, d, lo, hi) : newton_box_inf();
                const int ns = newton_box_update(s, z, lo, hi, d, w, D.s, tb, &p, &r);
                A.p[i] = p;
                A.r[i] = r;
                if (ns != s) {
                    A.es[i] = (unsigned char)ns;
                    nhit = newton_add(nhit, 1.0);
                    s = ns;
                }
            }
        }
        if (A.zp) A.zp[i] = newton_box_point(s, z, p, lo, hi);
        if (A.es_out) A.es_out[i] = (double)s;
        const double g = newton_box_in_f0(s) ? A.g[i] : 0.0;
        const bool f = s == NBOX_FREE;
        rr = newton_add(rr, f ? newton_mul(r, r) : 0.0);
        pg = newton_add(pg, newton_mul(p, g));
        pr = newton_add(pr, newton_mul(p, r));
        pp = newton_add(pp, newton_mul(p, p));
        nfree = newton_add(nfree, f ? 1.0 : 0.0);
        fm |= (f ? 1u : 0u) << t;
        rf[t] = f ? r : 0.0;
    }
    rr = pc_tree64(rr); pg = pc_tree64(pg); pr = pc_tree64(pr); pp = pc_tree64(pp); nhit = pc_tree64(nhit); nfree = pc_tree64(nfree);
    if (c.lane == 0) {
        A.part[(size_t)NBX_RR * A.nb + c.b] = rr;
        A.part[(size_t)NBX_NHIT * A.nb + c.b] = nhit;
        A.part[(size_t)NBX_PG * A.nb + c.b] = pg;
        A.part[(size_t)NBX_PR * A.nb + c.b] = pr;
        A.part[(size_t)NBX_PP_NEW * A.nb + c.b] = pp;
        A.part[(size_t)NBX_NFREE * A.nb + c.b] = nfree;
    }
    if (pc_on(K, j)) pc_dots_chunk(K, c, fm, rf);
}

// j = 0: behind the start's application; j >= 1: behind k_precond_comb of iteration j
__global__ void __launch_bounds__(PRECOND_THREADS) k_precond_dir(KPrecond K, int j, int max_iter) {
    const KNewtonBox& A = K.B;
    // [0] r . r over F, [1] n_hit, [2] r . z; workgroup 0 also [3 .. 7] = p . g, p . r, p . p, |F|, held
    __shared__ double dots[8];
    const int slots[8] = {NBX_RR, NBX_NHIT, NPX_RZ, NBX_PG, NBX_PR, NBX_PP_NEW, NBX_NFREE, NBX_HELD};
    pc_combine(A, slots, blockIdx.x == 0 ? 8 : 3, dots);
    const double rr_new = dots[0], n_hit = j >= 1 ? dots[1] : 0.0, rz_new = dots[2];
    const double rr0 = j == 0 ? rr_new : A.state[NPS_RR0];
    int status;
    if (j == 0) status = rr_new == 0.0 ? NEWTON_CONVERGED : NEWTON_CONTINUE;
    else {
        status = (int)A.state[NPS_DECISION];
        if (status == NEWTON_CONTINUE && newton_converged(rr_new, rr0, A.rtol, A.atol)) status = NEWTON_CONVERGED;
    }
    const bool go_on = status == NEWTON_CONTINUE;
    const bool was_on = pc_on(K, j);
    const bool fallback = go_on && was_on && precond_rz_bad(rz_new);
    const bool on = was_on && !fallback;
    const bool restart = j >= 1 && go_on && n_hit > 0.0;
    const double rz_use = fallback ? rr_new : rz_new;
    if (go_on && j >= 1 && j == max_iter) status = NEWTON_MAX_ITER;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double held = j == 0 ? dots[7] : A.state[NPS_HELD];
        const double hits = j == 0 ? 0.0 : newton_add(A.state[NPS_HITS + (j - 1) % 2], n_hit);
        const double restarts = j == 0 ? 0.0 : newton_add(A.state[NPS_RESTARTS + (j - 1) % 2], restart ? 1.0 : 0.0);
        const double fallbacks = newton_add(j == 0 ? 0.0 : A.state[NPS_FALLBACKS + (j - 1) % 2], fallback ? 1.0 : 0.0);
        const double taken = j == 0 ? 0.0 : newton_add(A.state[NPS_TAKEN + (j - 1) % 2], A.state[NPS_TOOK]);
        const double rz0 = j == 0 ? rz_use : A.state[NPS_RZ0];
        A.state[NPS_STATUS] = (double)status;
        A.state[NPS_ITER] = (double)j;
        A.state[NPS_TAKEN_OUT] = taken;
        if (j == 0) {
            A.state[NPS_RR0] = rr_new;
            A.state[NPS_HELD] = held;
            A.state[NPS_RZ0] = rz0;
        }
        A.state[NPS_RZ + j % 2] = rz_use;
        A.state[NPS_HITS + j % 2] = hits;
        A.state[NPS_RESTARTS + j % 2] = restarts;
        A.state[NPS_ACTIVE + j % 2] = on ? 1.0 : 0.0;
        A.state[NPS_TAKEN + j % 2] = taken;
        A.state[NPS_FALLBACKS + j % 2] = fallbacks;
        if (j >= 1 && A.trace) {
            double* row = A.trace + PRECOND_TRACE * (size_t)(j - 1);
            row[3] = rr_new; row[5] = n_hit; row[6] = rz_new; row[7] = on ? 1.0 : 0.0;
        }
        if (status != NEWTON_CONTINUE) {
            const double pg = dots[3], pr = dots[4], pp = dots[5];   // (zeros at j = 0)
            A.info[0] = (double)status;
            A.info[1] = (double)j;
            A.info[2] = sqrt(rr0);
            A.info[3] = sqrt(rr_new);
            A.info[4] = sqrt(pp);
            A.info[5] = pg;
            A.info[6] = newton_mul(-0.5, newton_add(pg, pr));
            A.info[7] = j >= 1 ? newton_div(A.state[NPS_KAPPA], A.state[NPS_DD]) : 0.0;
            A.info[8] = held;
            A.info[9] = hits;
            A.info[10] = restarts;
            A.info[11] = dots[6];
            A.info[12] = K.cnt > 0 ? K.pc[PPC_NADM] : 0.0;
            A.info[13] = taken;
            A.info[14] = fallbacks;
            A.info[15] = sqrt(rz0);
        }
    }
    if (!go_on) return;
    const int mode = j == 0 ? PRECOND_DIR_START : (restart || fallback ? PRECOND_DIR_RESTART : PRECOND_DIR_BETA);
    const double beta = mode == PRECOND_DIR_BETA ? newton_div(rz_use, A.state[NPS_RZ + (j - 1) % 2]) : 0.0;
    const double* x = fallback ? A.r : K.z;
    const Chunk c = pc_chunk(A);
    for (int t = 0; t < c.live; ++t) {
        const int64_t i = c.base + NEWTON_LANES * t;
        A.d[i] = precond_direction(A.es[i], mode, beta, mode == PRECOND_DIR_BETA ? A.d[i] : 0.0, x[i]);
    }
}

// dst = src, n doubles (a pushed pair on the device)
__global__ void __launch_bounds__(256) k_precond_copy(int64_t n, const double* src, double* dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

unsigned precond_grid(const KNewtonBox& A) { return (unsigned)std::max<int64_t>(1, (A.nb + PRECOND_WAVES - 1) / PRECOND_WAVES); }

}  // namespace

void launch_precond_states(hipStream_t st, const KReduced& R, const KNewtonBox& A) {
    hipLaunchKernelGGL(k_precond_states, dim3(precond_grid(A)), dim3(PRECOND_THREADS), 0, st, R, A);
}
void launch_precond_gram(hipStream_t st, const KPrecond& A) {
    hipLaunchKernelGGL(k_precond_gram, dim3(precond_grid(A.B)), dim3(PRECOND_THREADS), 0, st, A);
}
void launch_precond_prep(hipStream_t st, const KPrecond& A) { hipLaunchKernelGGL(k_precond_prep, dim3(1), dim3(PRECOND_THREADS), 0, st, A); }
void launch_precond_dots(hipStream_t st, const KPrecond& A, const double* r) {
    hipLaunchKernelGGL(k_precond_dots, dim3(precond_grid(A.B)), dim3(PRECOND_THREADS), 0, st, A, r);
}
void launch_precond_comb(hipStream_t st, const KPrecond& A, const double* r, double* z, int j) {
    hipLaunchKernelGGL(k_precond_comb, dim3(precond_grid(A.B)), dim3(PRECOND_THREADS), 0, st, A, r, z, j);
}
void launch_precond_step(hipStream_t st, const KPrecond& A, int j) {
    hipLaunchKernelGGL(k_precond_step, dim3(precond_grid(A.B)), dim3(PRECOND_THREADS), 0, st, A, j);
}
void launch_precond_dir(hipStream_t st, const KPrecond& A, int j, int max_iter) {
    hipLaunchKernelGGL(k_precond_dir, dim3(precond_grid(A.B)), dim3(PRECOND_THREADS), 0, st, A, j, max_iter);
}
void launch_precond_copy(hipStream_t st, int64_t n, const double* src, double* dst) {
    if (n > 0) hipLaunchKernelGGL(k_precond_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, src, dst);
}

}  // namespace dto
