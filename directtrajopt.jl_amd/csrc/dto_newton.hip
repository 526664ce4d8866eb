// dto_newton.hip -- kernels of the truncated-Newton step (dto_projected_newton_step and its _dev form; the dot order and the scalar
// decision: dto_newton_plan.h; include/dto_engine.h, "Truncated-Newton step").  The step is Steihaug-Toint CG on
// A = M (T'HT) M + shift M; the product T'HT d is the engine's own (the one-column chunk of the block products), and what is here are
// the vector updates, the dots in their fixed order and the decisions, all on the device.
//
//   k_newton_start  r = M g, p = 0, d = -r, and the partial sums of r . r
//   k_newton_curv   w = M (y + shift * d) written in place of y, and the partial sums of kappa = d . w, d . d, p . d, p . p in one pass
//   k_newton_step   combines those four, decides (newton_decide), p = p + s * d, r = r + s * w (not after NOT_FINITE), the partial sums of
//                   r . r, p . g, p . r and p . p behind the update; workgroup 0 writes the decision, s, kappa, d . d and the trace row
//   k_newton_dir    combines r . r; behind a CG step the convergence test, then beta = rr' / rr, d = beta * d - r; workgroup 0 writes the
//                   status, the iteration count, rr' and, when the step ends, `info`.  With j = 0 it closes k_newton_start: rr0, and
//                   CONVERGED with no iteration when rr0 == 0.
// M zeroes the dependent entries (the states of knots 2 .. N) and the entries whose mask is 0.0; the mask of a dependent entry is not read.
//
// A wavefront owns a chunk of NEWTON_CHUNK entries, a workgroup NEWTON_WAVES chunks in a row.  Stage 2 of a dot -- the sum of the
// chunks' partial sums -- is done redundantly by EVERY workgroup at the start of k_newton_step / k_newton_dir, one wavefront per dot,
// from L2: the same operations in the same order everywhere, so every workgroup holds the same bits and no workgroup waits for another
// inside a launch.  (The other form, a one-workgroup launch of its own before each of the two, k_newton_combine, is kept for A/B runs of
// TUNING builds, DTO_NEWTON_COMBINE=1: two launches and 0.01 ms of device time more per iteration)
// What a launch reads of the scalars is never written in that launch (rr alternates between two slots).
// Plain 8-byte loads and stores -- the lane-to-entry map of the dot order is i = 256 b + l + 64 t -- wavefront shuffles, four doubles of
// LDS, no atomics.
#include <algorithm>

#include "dto_kernels.h"
#include "dto_newton_plan.h"
#include "dto_reduced_plan.h"

namespace dto {

namespace {

constexpr int NEWTON_WAVES = 16;                               // chunks per workgroup
constexpr int NEWTON_THREADS = NEWTON_WAVES * NEWTON_LANES;    // 1024

__device__ __forceinline__ double tree64(double a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = newton_add(a, __shfl_down(a, off, 64));
    return a;   // lane 0 holds a_0 of the halving tree
}

__device__ __forceinline__ bool is_free(const KReduced& R, const double* __restrict__ mask, int64_t i) {
    if (reduced_is_dependent(R, i)) return false;
    return !mask || mask[i] != 0.0;
}

// stage 2 of `count` dots by the first `count` wavefronts of the workgroup: out[w] = the dot of slot slot0 + w.  (A.combined: the
// dots a launch_newton_combine before this launch left in the state -- the same operations in the same order, so the same bits.)
__device__ __forceinline__ void combine(const KNewton& A, int slot0, int count, double* out) {
    const int wave = threadIdx.x / NEWTON_LANES, lane = threadIdx.x % NEWTON_LANES;
    if (A.combined) {
        if ((int)threadIdx.x < count) out[threadIdx.x] = A.state[NWS_DOTS + threadIdx.x];
    } else if (wave < count) {
        const double t = tree64(newton_lane_sum(A.part + (size_t)(slot0 + wave) * A.nb, A.nb, lane));
        if (lane == 0) out[wave] = t;
    }
    __syncthreads();
}

#define NEWTON_CHUNK_LOOP(b, i, lane)                                                              \
    const int lane = threadIdx.x % NEWTON_LANES;                                                   \
    const int64_t b = (int64_t)blockIdx.x * NEWTON_WAVES + threadIdx.x / NEWTON_LANES;             \
    const int64_t i##_end = b < A.nb ? min((b + 1) * NEWTON_CHUNK, A.n) : 0;                       \
    for (int64_t i = b * NEWTON_CHUNK + lane; i < i##_end; i += NEWTON_LANES)

__global__ void __launch_bounds__(NEWTON_THREADS) k_newton_start(KReduced R, KNewton A) {
    double rr = 0.0;
    NEWTON_CHUNK_LOOP(b, i, lane) {
        const double r = is_free(R, A.mask, i) ? A.g[i] : 0.0;
        A.r[i] = r;
        A.p[i] = 0.0;
        A.d[i] = -r;
        rr = newton_add(rr, newton_mul(r, r));
    }
    if (b >= A.nb) return;   // (uniform in a wavefront)
    rr = tree64(rr);
    if (lane == 0) A.part[(size_t)NWT_RR * A.nb + b] = rr;
}

__global__ void __launch_bounds__(NEWTON_THREADS) k_newton_curv(KReduced R, KNewton A) {
    double kappa = 0.0, dd = 0.0, pd = 0.0, pp = 0.0;
    NEWTON_CHUNK_LOOP(b, i, lane) {
        const double d = A.d[i], p = A.p[i];
        const double w = is_free(R, A.mask, i) ? newton_add(A.w[i], newton_mul(A.shift, d)) : 0.0;
        A.w[i] = w;
        kappa = newton_add(kappa, newton_mul(d, w));
        dd = newton_add(dd, newton_mul(d, d));
        pd = newton_add(pd, newton_mul(p, d));
        pp = newton_add(pp, newton_mul(p, p));
    }
    if (b >= A.nb) return;
    kappa = tree64(kappa); dd = tree64(dd); pd = tree64(pd); pp = tree64(pp);
    if (lane == 0) {
        A.part[(size_t)NWT_KAPPA * A.nb + b] = kappa;
        A.part[(size_t)NWT_DD * A.nb + b] = dd;
        A.part[(size_t)NWT_PD * A.nb + b] = pd;
        A.part[(size_t)NWT_PP * A.nb + b] = pp;
    }
}

__global__ void __launch_bounds__(NEWTON_THREADS) k_newton_step(KReduced R, KNewton A, int j) {
    __shared__ double dots[4];   // kappa, d . d, p . d, p . p
    combine(A, NWT_KAPPA, 4, dots);
    const double kappa = dots[0], dd = dots[1];
    const NewtonDecision D = newton_decide(kappa, dd, dots[2], dots[3], A.state[NWS_RR + (j - 1) % 2], A.radius, j);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.state[NWS_DECISION] = (double)D.status;
        A.state[NWS_S] = D.s;
        A.state[NWS_KAPPA] = kappa;
        A.state[NWS_DD] = dd;
        if (A.trace) {
            double* row = A.trace + 4 * (size_t)(j - 1);
            row[0] = kappa; row[1] = dd; row[2] = D.s;
        }
    }
    const bool move = D.status != NEWTON_NOT_FINITE;
    double rr = 0.0, pg = 0.0, pr = 0.0, pp = 0.0;
    NEWTON_CHUNK_LOOP(b, i, lane) {
        double p = A.p[i], r = A.r[i];
        if (move) {
            p = newton_add(p, newton_mul(D.s, A.d[i]));
            r = newton_add(r, newton_mul(D.s, A.w[i]));
            A.p[i] = p;
            A.r[i] = r;
        }
        const double g = is_free(R, A.mask, i) ? A.g[i] : 0.0;
        rr = newton_add(rr, newton_mul(r, r));
        pg = newton_add(pg, newton_mul(p, g));
        pr = newton_add(pr, newton_mul(p, r));
        pp = newton_add(pp, newton_mul(p, p));
    }
    if (b >= A.nb) return;
    rr = tree64(rr); pg = tree64(pg); pr = tree64(pr); pp = tree64(pp);
    if (lane == 0) {
        A.part[(size_t)NWT_RR * A.nb + b] = rr;
        A.part[(size_t)NWT_PG * A.nb + b] = pg;
        A.part[(size_t)NWT_PR * A.nb + b] = pr;
        A.part[(size_t)NWT_PP_NEW * A.nb + b] = pp;
    }
}

// j = 0: behind k_newton_start; j >= 1: behind k_newton_step of iteration j
__global__ void __launch_bounds__(NEWTON_THREADS) k_newton_dir(KNewton A, int j, int max_iter) {
    __shared__ double dots[4];   // [0] r . r; workgroup 0 at j >= 1 also [1 .. 3] = p . g, p . r, p . p (slots NWT_RR .. NWT_PP_NEW)
    combine(A, NWT_RR, j >= 1 && blockIdx.x == 0 ? 4 : 1, dots);
    const double rr_new = dots[0];
    const double rr0 = j == 0 ? rr_new : A.state[NWS_RR0];
    int status;
    if (j == 0) status = rr_new == 0.0 ? NEWTON_CONVERGED : NEWTON_CONTINUE;
    else {
        status = (int)A.state[NWS_DECISION];
        if (status == NEWTON_CONTINUE && newton_converged(rr_new, rr0, A.rtol, A.atol)) status = NEWTON_CONVERGED;
    }
    const bool cg_step = j >= 1 && (int)A.state[NWS_DECISION] == NEWTON_CONTINUE && status == NEWTON_CONTINUE;
    if (cg_step && j == max_iter) status = NEWTON_MAX_ITER;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        A.state[NWS_STATUS] = (double)status;
        A.state[NWS_ITER] = (double)j;
        if (j == 0) A.state[NWS_RR0] = rr_new;
        A.state[NWS_RR + j % 2] = rr_new;
        if (j >= 1 && A.trace) A.trace[4 * (size_t)(j - 1) + 3] = rr_new;
        if (status != NEWTON_CONTINUE) {
            const double pg = j >= 1 ? dots[1] : 0.0, pr = j >= 1 ? dots[2] : 0.0, pp = j >= 1 ? dots[3] : 0.0;
            A.info[0] = (double)status;
            A.info[1] = (double)j;
            A.info[2] = sqrt(rr0);
            A.info[3] = sqrt(rr_new);
            A.info[4] = sqrt(pp);
            A.info[5] = pg;
            A.info[6] = newton_mul(-0.5, newton_add(pg, pr));
            A.info[7] = j >= 1 ? newton_div(A.state[NWS_KAPPA], A.state[NWS_DD]) : 0.0;
        }
    }
    if (!cg_step) return;
    const double beta = newton_div(rr_new, A.state[NWS_RR + (j - 1) % 2]);
    NEWTON_CHUNK_LOOP(b, i, lane) A.d[i] = newton_sub(newton_mul(beta, A.d[i]), A.r[i]);
}

__global__ void __launch_bounds__(4 * NEWTON_LANES) k_newton_combine(KNewton A, int slot0, int count) {
    const int wave = threadIdx.x / NEWTON_LANES, lane = threadIdx.x % NEWTON_LANES;
    if (wave >= count) return;
    const double t = tree64(newton_lane_sum(A.part + (size_t)(slot0 + wave) * A.nb, A.nb, lane));
    if (lane == 0) A.state[NWS_DOTS + wave] = t;
}

unsigned newton_grid(const KNewton& A) { return (unsigned)std::max<int64_t>(1, (A.nb + NEWTON_WAVES - 1) / NEWTON_WAVES); }

}  // namespace

void launch_newton_start(hipStream_t st, const KReduced& R, const KNewton& A) {
    hipLaunchKernelGGL(k_newton_start, dim3(newton_grid(A)), dim3(NEWTON_THREADS), 0, st, R, A);
}
void launch_newton_curv(hipStream_t st, const KReduced& R, const KNewton& A) {
    hipLaunchKernelGGL(k_newton_curv, dim3(newton_grid(A)), dim3(NEWTON_THREADS), 0, st, R, A);
}
void launch_newton_step(hipStream_t st, const KReduced& R, const KNewton& A, int j) {
    hipLaunchKernelGGL(k_newton_step, dim3(newton_grid(A)), dim3(NEWTON_THREADS), 0, st, R, A, j);
}
void launch_newton_dir(hipStream_t st, const KNewton& A, int j, int max_iter) {
    hipLaunchKernelGGL(k_newton_dir, dim3(newton_grid(A)), dim3(NEWTON_THREADS), 0, st, A, j, max_iter);
}

void launch_newton_combine(hipStream_t st, const KNewton& A, int slot0, int count) {
    hipLaunchKernelGGL(k_newton_combine, dim3(1), dim3(4 * NEWTON_LANES), 0, st, A, slot0, count);
}

}  // namespace dto
