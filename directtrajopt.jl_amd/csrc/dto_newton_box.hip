// dto_newton_box.hip -- kernels of the bound-constrained truncated-Newton step (dto_projected_newton_step_box and its _dev form; the
// entry rules, the decision and the loop: dto_newton_box_plan.h; include/dto_engine.h, "Bound-constrained truncated-Newton step").
// The shape is dto_newton.hip's: the product T'HT d is the engine's own, and what is here are the vector updates with their clamps,
// the dots in their fixed order, the smallest breakpoint and the decisions, all on the device.
//
//   k_newton_box_start  the entry states (one byte each), r = g on F0, p = 0, d = -r, the partial sums of r . r and the counts of free
//                       and held entries; Zp = Z + p and the states as doubles where asked for
//   k_newton_box_curv   w = y + shift * d on F0 written in place of y, the partial sums of kappa = d . w, d . d, p . d, p . p and the
//                       chunk's smallest breakpoint (a shuffle tree of minima) in one pass
//   k_newton_box_step   combines those five, decides (newton_box_decide), p = p + s * d, r = r + s * w, clamps the free entries that
//                       reached a bound and writes their states, Zp and the states as doubles where asked for, the partial sums of
//                       r . r over the new F, p . g, p . r, p . p and the counts of hit and free entries
//   k_newton_box_dir    combines r . r and the hit count; behind a CG step the convergence test, then the restart d = -r on F or
//                       d = beta * d - r; workgroup 0 writes the status, the iteration count, the running counts, the rest of the
//                       trace row and, when the step ends, `info`.  With j = 0 it closes the start.
// A wavefront owns a chunk of NEWTON_CHUNK entries (lane-to-entry map i = 256 b + l + 64 t), a workgroup NEWTON_BOX_WAVES chunks in a
// row.  Stage 2 of every reduction is done by EVERY workgroup itself, one wavefront per slot, from L2: the same operations in the same
// order everywhere.  What a launch reads of the scalars is never written in that launch (rr and the running counts alternate between
// two slots).  Plain 8-byte loads and stores, one byte per entry for the state, wavefront shuffles, seven doubles of LDS, no atomics.
#include <algorithm>

#include "dto_kernels.h"
#include "dto_newton_box_plan.h"
#include "dto_reduced_plan.h"

namespace dto {

namespace {

constexpr int NEWTON_BOX_WAVES = 16;                                    // chunks per workgroup
constexpr int NEWTON_BOX_THREADS = NEWTON_BOX_WAVES * NEWTON_LANES;     // 1024

__device__ __forceinline__ double box_tree64(double a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = newton_add(a, __shfl_down(a, off, 64));
    return a;   // lane 0 holds a_0 of the halving tree
}
__device__ __forceinline__ double box_mintree64(double a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = newton_box_min(a, __shfl_down(a, off, 64));
    return a;
}

// stage 2 of the slots slot0 .. slot0 + count - 1 by the first `count` wavefronts of the workgroup; slot NBX_TMIN is a minimum
__device__ __forceinline__ void box_combine(const KNewtonBox& A, int slot0, int count, double* out) {
    const int wave = threadIdx.x / NEWTON_LANES, lane = threadIdx.x % NEWTON_LANES;
    if (wave < count) {
        const double* P = A.part + (size_t)(slot0 + wave) * A.nb;
        double t;
        if (slot0 + wave == NBX_TMIN) {
            double m = newton_box_inf();
            for (int64_t b = lane; b < A.nb; b += NEWTON_LANES) m = newton_box_min(m, P[b]);
            t = box_mintree64(m);
        } else {
            t = box_tree64(newton_lane_sum(P, A.nb, lane));
        }
        if (lane == 0) out[wave] = t;
    }
    __syncthreads();
}

#define NEWTON_BOX_CHUNK_LOOP(b, i, lane)                                                          \
    const int lane = threadIdx.x % NEWTON_LANES;                                                   \
    const int64_t b = (int64_t)blockIdx.x * NEWTON_BOX_WAVES + threadIdx.x / NEWTON_LANES;         \
    const int64_t i##_end = b < A.nb ? min((b + 1) * NEWTON_CHUNK, A.n) : 0;                       \
    for (int64_t i = b * NEWTON_CHUNK + lane; i < i##_end; i += NEWTON_LANES)

__device__ __forceinline__ double box_lo(const KNewtonBox& A, int64_t i) { return A.lo ? A.lo[i] : -newton_box_inf(); }
__device__ __forceinline__ double box_hi(const KNewtonBox& A, int64_t i) { return A.hi ? A.hi[i] : newton_box_inf(); }

__global__ void __launch_bounds__(NEWTON_BOX_THREADS) k_newton_box_start(KReduced R, KNewtonBox A) {
    double rr = 0.0, nfree = 0.0, held = 0.0;
    NEWTON_BOX_CHUNK_LOOP(b, i, lane) {
        int s = NBOX_FIXED;
        double r = 0.0;
        if (!reduced_is_dependent(R, i) && (!A.mask || A.mask[i] != 0.0)) {
            const double g = A.g[i];
            s = newton_box_classify(A.Z[i], box_lo(A, i), box_hi(A, i), g);
            if (s == NBOX_FREE) r = g;
        }
        A.es[i] = (unsigned char)s;
        A.r[i] = r;
        A.p[i] = 0.0;
        A.d[i] = -r;
        if (A.zp) A.zp[i] = newton_add(A.Z[i], 0.0);
        if (A.es_out) A.es_out[i] = (double)s;
        rr = newton_add(rr, newton_mul(r, r));
        nfree = newton_add(nfree, s == NBOX_FREE ? 1.0 : 0.0);
        held = newton_add(held, s == NBOX_HELD_LO || s == NBOX_HELD_HI ? 1.0 : 0.0);
    }
    if (b >= A.nb) return;   // (uniform in a wavefront)
    rr = box_tree64(rr); nfree = box_tree64(nfree); held = box_tree64(held);
    if (lane == 0) {
        A.part[(size_t)NBX_RR * A.nb + b] = rr;
        A.part[(size_t)NBX_NHIT * A.nb + b] = 0.0;
        A.part[(size_t)NBX_PG * A.nb + b] = 0.0;
        A.part[(size_t)NBX_PR * A.nb + b] = 0.0;
        A.part[(size_t)NBX_PP_NEW * A.nb + b] = 0.0;
        A.part[(size_t)NBX_NFREE * A.nb + b] = nfree;
        A.part[(size_t)NBX_HELD * A.nb + b] = held;
    }
}

__global__ void __launch_bounds__(NEWTON_BOX_THREADS) k_newton_box_curv(KNewtonBox A) {
    double kappa = 0.0, dd = 0.0, pd = 0.0, pp = 0.0, tmin = newton_box_inf();
    NEWTON_BOX_CHUNK_LOOP(b, i, lane) {
        const int s = A.es[i];
        const double d = A.d[i], p = A.p[i];
        const double w = newton_box_in_f0(s) ? newton_add(A.w[i], newton_mul(A.shift, d)) : 0.0;
        A.w[i] = w;
        if (s == NBOX_FREE) tmin = newton_box_min(tmin, newton_box_breakpoint(A.Z[i], p, d, box_lo(A, i), box_hi(A, i)));
        kappa = newton_add(kappa, newton_mul(d, w));
        dd = newton_add(dd, newton_mul(d, d));
        pd = newton_add(pd, newton_mul(p, d));
        pp = newton_add(pp, newton_mul(p, p));
    }
    if (b >= A.nb) return;
    kappa = box_tree64(kappa); dd = box_tree64(dd); pd = box_tree64(pd); pp = box_tree64(pp); tmin = box_mintree64(tmin);
    if (lane == 0) {
        A.part[(size_t)NBX_KAPPA * A.nb + b] = kappa;
        A.part[(size_t)NBX_DD * A.nb + b] = dd;
        A.part[(size_t)NBX_PD * A.nb + b] = pd;
        A.part[(size_t)NBX_PP * A.nb + b] = pp;
        A.part[(size_t)NBX_TMIN * A.nb + b] = tmin;
    }
}

__global__ void __launch_bounds__(NEWTON_BOX_THREADS) k_newton_box_step(KNewtonBox A, int j) {
    __shared__ double dots[5];   // kappa, d . d, p . d, p . p, tau_box
    box_combine(A, NBX_KAPPA, 5, dots);
    const double kappa = dots[0], dd = dots[1], tau_box = dots[4];
    const NewtonDecision D = newton_box_decide(kappa, dd, dots[2], dots[3], A.state[NBS_RR + (j - 1) % 2], A.radius, tau_box, j);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.state[NBS_DECISION] = (double)D.status;
        A.state[NBS_S] = D.s;
        A.state[NBS_KAPPA] = kappa;
        A.state[NBS_DD] = dd;
        if (A.trace) {
            double* row = A.trace + NEWTON_BOX_TRACE * (size_t)(j - 1);
            row[0] = kappa; row[1] = dd; row[2] = D.s; row[4] = tau_box;
        }
    }
    const bool move = D.status != NEWTON_NOT_FINITE;
    double rr = 0.0, pg = 0.0, pr = 0.0, pp = 0.0, nhit = 0.0, nfree = 0.0;
    NEWTON_BOX_CHUNK_LOOP(b, i, lane) {
        int s = A.es[i];
        double p = A.p[i], r = A.r[i];
        const bool in_f = s == NBOX_FREE;
        const double z = in_f || A.zp ? A.Z[i] : 0.0, lo = in_f || A.zp ? box_lo(A, i) : 0.0, hi = in_f || A.zp ? box_hi(A, i) : 0.0;
        if (move) {
            const double d = A.d[i];
            const double t = in_f ? newton_box_breakpoint(z, p, d, lo, hi) : newton_box_inf();
            const int ns = newton_box_update(s, z, lo, hi, d, A.w[i], D.s, t, &p, &r);
            A.p[i] = p;
            A.r[i] = r;
            if (ns != s) {
                A.es[i] = (unsigned char)ns;
                nhit = newton_add(nhit, 1.0);
                s = ns;
            }
        }
        if (A.zp) A.zp[i] = newton_box_point(s, z, p, lo, hi);
        if (A.es_out) A.es_out[i] = (double)s;
        const double g = newton_box_in_f0(s) ? A.g[i] : 0.0;
        rr = newton_add(rr, s == NBOX_FREE ? newton_mul(r, r) : 0.0);
        pg = newton_add(pg, newton_mul(p, g));
        pr = newton_add(pr, newton_mul(p, r));
        pp = newton_add(pp, newton_mul(p, p));
        nfree = newton_add(nfree, s == NBOX_FREE ? 1.0 : 0.0);
    }
    if (b >= A.nb) return;
    rr = box_tree64(rr); pg = box_tree64(pg); pr = box_tree64(pr); pp = box_tree64(pp); nhit = box_tree64(nhit); nfree = box_tree64(nfree);
    if (lane == 0) {
        A.part[(size_t)NBX_RR * A.nb + b] = rr;
        A.part[(size_t)NBX_NHIT * A.nb + b] = nhit;
        A.part[(size_t)NBX_PG * A.nb + b] = pg;
        A.part[(size_t)NBX_PR * A.nb + b] = pr;
        A.part[(size_t)NBX_PP_NEW * A.nb + b] = pp;
        A.part[(size_t)NBX_NFREE * A.nb + b] = nfree;
    }
}

// j = 0: behind k_newton_box_start; j >= 1: behind k_newton_box_step of iteration j
__global__ void __launch_bounds__(NEWTON_BOX_THREADS) k_newton_box_dir(KNewtonBox A, int j, int max_iter) {
    // [0] r . r over F, [1] n_hit; workgroup 0 also [2 .. 6] = p . g, p . r, p . p, |F|, held (slots NBX_RR .. NBX_HELD)
    __shared__ double dots[7];
    box_combine(A, NBX_RR, blockIdx.x == 0 ? 7 : 2, dots);
    const double rr_new = dots[0], n_hit = j >= 1 ? dots[1] : 0.0;
    const double rr0 = j == 0 ? rr_new : A.state[NBS_RR0];
    int status;
    if (j == 0) status = rr_new == 0.0 ? NEWTON_CONVERGED : NEWTON_CONTINUE;
    else {
        status = (int)A.state[NBS_DECISION];
        if (status == NEWTON_CONTINUE && newton_converged(rr_new, rr0, A.rtol, A.atol)) status = NEWTON_CONVERGED;
    }
    const bool cg_step = j >= 1 && (int)A.state[NBS_DECISION] == NEWTON_CONTINUE && status == NEWTON_CONTINUE;
    const bool restart = cg_step && n_hit > 0.0;
    if (cg_step && j == max_iter) status = NEWTON_MAX_ITER;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double held = j == 0 ? dots[6] : A.state[NBS_HELD];
        const double hits = j == 0 ? 0.0 : newton_add(A.state[NBS_HITS + (j - 1) % 2], n_hit);
        const double restarts = j == 0 ? 0.0 : newton_add(A.state[NBS_RESTARTS + (j - 1) % 2], restart ? 1.0 : 0.0);
        A.state[NBS_STATUS] = (double)status;
        A.state[NBS_ITER] = (double)j;
        if (j == 0) {
            A.state[NBS_RR0] = rr_new;
            A.state[NBS_HELD] = held;
        }
        A.state[NBS_RR + j % 2] = rr_new;
        A.state[NBS_HITS + j % 2] = hits;
        A.state[NBS_RESTARTS + j % 2] = restarts;
        if (j >= 1 && A.trace) {
            double* row = A.trace + NEWTON_BOX_TRACE * (size_t)(j - 1);
            row[3] = rr_new; row[5] = n_hit;
        }
        if (status != NEWTON_CONTINUE) {
            const double pg = dots[2], pr = dots[3], pp = dots[4];   // (zeros at j = 0)
            A.info[0] = (double)status;
            A.info[1] = (double)j;
            A.info[2] = sqrt(rr0);
            A.info[3] = sqrt(rr_new);
            A.info[4] = sqrt(pp);
            A.info[5] = pg;
            A.info[6] = newton_mul(-0.5, newton_add(pg, pr));
            A.info[7] = j >= 1 ? newton_div(A.state[NBS_KAPPA], A.state[NBS_DD]) : 0.0;
            A.info[8] = held;
            A.info[9] = hits;
            A.info[10] = restarts;
            A.info[11] = dots[5];
        }
    }
    if (!cg_step) return;
    const double beta = restart ? 0.0 : newton_div(rr_new, A.state[NBS_RR + (j - 1) % 2]);
    NEWTON_BOX_CHUNK_LOOP(b, i, lane) A.d[i] = newton_box_direction(A.es[i], restart, beta, A.d[i], A.r[i]);
}

unsigned newton_box_grid(const KNewtonBox& A) { return (unsigned)std::max<int64_t>(1, (A.nb + NEWTON_BOX_WAVES - 1) / NEWTON_BOX_WAVES); }

}  // namespace

void launch_newton_box_start(hipStream_t st, const KReduced& R, const KNewtonBox& A) {
    hipLaunchKernelGGL(k_newton_box_start, dim3(newton_box_grid(A)), dim3(NEWTON_BOX_THREADS), 0, st, R, A);
}
void launch_newton_box_curv(hipStream_t st, const KNewtonBox& A) {
    hipLaunchKernelGGL(k_newton_box_curv, dim3(newton_box_grid(A)), dim3(NEWTON_BOX_THREADS), 0, st, A);
}
void launch_newton_box_step(hipStream_t st, const KNewtonBox& A, int j) {
    hipLaunchKernelGGL(k_newton_box_step, dim3(newton_box_grid(A)), dim3(NEWTON_BOX_THREADS), 0, st, A, j);
}
void launch_newton_box_dir(hipStream_t st, const KNewtonBox& A, int j, int max_iter) {
    hipLaunchKernelGGL(k_newton_box_dir, dim3(newton_box_grid(A)), dim3(NEWTON_BOX_THREADS), 0, st, A, j, max_iter);
}

}  // namespace dto
