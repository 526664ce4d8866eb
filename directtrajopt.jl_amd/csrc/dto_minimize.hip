// dto_minimize.hip -- kernels of the reduced-space minimize call (dto_projected_minimize and its _dev form; the rules, the scalars and the
// loop: dto_minimize_plan.h; include/dto_engine.h, "Reduced-space minimize").  Two small launches, one behind every trial and one behind
// every outer iteration; everything else the call enqueues is the step's, the merit's and the row pass's own.
//
//   k_minimize_trial  every workgroup reads the trial's scalars (phi and delta from the bank the launch reads, phi_t, the step's status,
//                     ||g|| and predicted decrease), calls minimize_trial_decide itself and, where the trial is accepted, copies its
//                     chunks of Zt into Z.  Thread 0 of workgroup 0 runs minimize_trial_update: the other bank, the history row, the
//                     mailbox and info.
//   k_minimize_outer  the same shape over the rows: every workgroup reads the row pass's max viol and the old one, calls
//                     minimize_outer_decide itself and writes mu <- mu_eff and the new rho on its non-dynamics rows (the dynamics rows
//                     are not touched).  Thread 0 of workgroup 0 runs minimize_outer_update.
// A wavefront owns a chunk of NEWTON_CHUNK entries (lane-to-entry map i = 256 b + l + 64 t), a workgroup sixteen chunks in a row, as in
// dto_precond.hip; every vector access is 512 contiguous bytes per wavefront and t.  No launch reads a scalar it writes: launch number q
// reads bank q % 2 and writes the other.  No atomics, no LDS; plain 8-byte loads and stores.
#include <algorithm>

#include "dto_kernels.h"
#include "dto_minimize_plan.h"

namespace dto {

namespace {

constexpr int MINIMIZE_WAVES = 16;
constexpr int MINIMIZE_THREADS = MINIMIZE_WAVES * NEWTON_LANES;   // 1024
constexpr int PER_LANE = NEWTON_CHUNK / NEWTON_LANES;             // 4

inline unsigned minimize_grid(int64_t entries) {
    return (unsigned)std::max<int64_t>(1, (newton_chunks(entries) + MINIMIZE_WAVES - 1) / MINIMIZE_WAVES);
}

__global__ void __launch_bounds__(MINIMIZE_THREADS) k_minimize_trial(KMinimize A) {
    const MinimizeTrialFlags& F = A.F;
    const double* opt = A.opt.v;
    if (!F.gradient) {
        const double phi = A.bank_in[MNS_PHI], delta = F.first_trial ? opt[MIN_OPT_RADIUS0] : A.bank_in[MNS_DELTA];
        const MinimizeTrial D = minimize_trial_decide(phi, A.phi_t[0], A.sinfo[6], (int)A.sinfo[0], delta, opt);
        if (D.accepted) {
            const int lane = threadIdx.x % NEWTON_LANES;
            const int64_t b = (int64_t)blockIdx.x * MINIMIZE_WAVES + threadIdx.x / NEWTON_LANES;
            const int64_t base = b * NEWTON_CHUNK + lane;
#pragma unroll
            for (int t = 0; t < PER_LANE; ++t) {
                const int64_t i = base + NEWTON_LANES * t;
                if (i < A.n) A.Z[i] = A.Zt[i];
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        minimize_trial_update(A.bank_in, A.bank_out, A.sinfo, F.gradient ? 0.0 : A.phi_t[0], F, opt, A.row, A.mail);
        minimize_info_store(A.bank_out, A.info);
    }
}

__global__ void __launch_bounds__(MINIMIZE_THREADS) k_minimize_outer(KMinimize A) {
    const double* opt = A.opt.v;
    const double viol = A.first_outer ? A.rinfo0[AL_MAX_VIOL] : A.bank_in[MNS_VIOL];
    const MinimizeOuter D = minimize_outer_decide(viol, A.rinfo[AL_MAX_VIOL], opt);
    const int lane = threadIdx.x % NEWTON_LANES;
    const int64_t b = (int64_t)blockIdx.x * MINIMIZE_WAVES + threadIdx.x / NEWTON_LANES;
    const int64_t base = A.n_dyn + b * NEWTON_CHUNK + lane;
#pragma unroll
    for (int t = 0; t < PER_LANE; ++t) {
        const int64_t r = base + NEWTON_LANES * t;
        if (r < A.n_cons) {
            A.mu[r] = A.mu_eff[r];
            A.rho[r] = minimize_rho_next(A.rho[r], D.grew, opt);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        minimize_outer_update(A.bank_in, A.bank_out, A.rinfo, A.rinfo0[AL_MAX_VIOL], A.first_outer, A.last_outer, opt, A.row, A.mail);
        minimize_info_store(A.bank_out, A.info);
    }
}

}  // namespace

void launch_minimize_trial(hipStream_t st, const KMinimize& A) {
    hipLaunchKernelGGL(k_minimize_trial, dim3(minimize_grid(A.n)), dim3(MINIMIZE_THREADS), 0, st, A);
}
void launch_minimize_outer(hipStream_t st, const KMinimize& A) {
    hipLaunchKernelGGL(k_minimize_outer, dim3(minimize_grid(A.n_cons - A.n_dyn)), dim3(MINIMIZE_THREADS), 0, st, A);
}

}  // namespace dto
