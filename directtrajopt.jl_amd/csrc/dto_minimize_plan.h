// dto_minimize_plan.h -- the reduced-space minimize call (dto_projected_minimize and its _dev form, dto_minimize.hip; include/dto_engine.h,
// "Reduced-space minimize") in plain C++ (no HIP header, no engine header): the trust-region rules of a trial, the multiplier / penalty
// rules of an outer iteration, the scalars both carry from launch to launch, and the whole loop.  The rounded operators are those of
// dto_newton_plan.h; every difference, product and quotient below is rounded on its own, in the operand order written.  The same text
// serves the kernels, the host routine and a g++-built test (tests/test_minimize_plan_header.py).
//
// A trial (minimize_trial_decide), from phi at Z, phi_t at the trial point, the step's predicted decrease and status, and delta:
//   ratio = (phi - phi_t) / predicted
//   the step's status is NOT_FINITE, or ratio is not finite       stop = NOT_FINITE, rejected, delta stays
//   accepted = ratio > eta_accept
//   ratio < eta_shrink                                            delta_next = delta / shrink_div
//   else ratio > eta_grow and the step's status != CONVERGED      delta_next = min(delta * grow_mul, radius_max)
//   else                                                          delta_next = delta
//   delta_next < radius_min                                       stop = RADIUS
// With the defaults (0.1, 0.25, 0.75, 4, 2, +inf, 0) these are the comparisons and the bits of the README's trust-region loop.
// An outer iteration (minimize_outer_decide), from max viol before and behind the inner loop:
//   grew = !(new_viol <= viol / viol_div)         (a NaN grows the penalty)
//   a row's penalty becomes rho_r * rho_mul where grew and rho_r != 0, and stays elsewhere (minimize_rho_next)
//   feasible = new_viol <= ctol
// The loop (minimize_solve below is this text as a program):
//   with rho: the row pass at the caller's Z gives the first max viol
//   outer iteration o = 0 .. outer - 1  (without rho: exactly one, no row pass, no outer decision)
//     phi, Z <- merit(Z): Z becomes its feasible trajectory;  delta = radius0
//     trial t = 0 .. trials - 1
//       (info, Zp) = step(Z, delta)
//       info[2] <= gtol: the inner loop ends with GRADIENT before any merit; the step is discarded, the trial logged as rejected
//       else (phi_t, Zt) = merit(Zp), the decision; accepted: Z = Zt, phi = phi_t;  stop != 0 ends the inner loop;  the last trial ends
//       it with MAX_TRIALS
//     NOT_FINITE ends the call.  Without rho the inner loop's end is the call's: GRADIENT -> CONVERGED, RADIUS, MAX_TRIALS.
//     with rho: (mu_eff, max viol, ..) = rows(Z);  mu <- mu_eff on the non-dynamics rows, the outer decision, rho, viol;
//       GRADIENT and feasible: CONVERGED;  else the last outer iteration: MAX_OUTER
// With gtol = ctol = radius_min = 0 the loop runs outer x trials trials (unless a gradient norm is exactly 0).
//
// The scalars (MINIMIZE_STATE doubles, two banks on the device: launch number q reads bank q % 2 and writes the other, so no launch reads
// a scalar it writes) are `info` as it stands, with the inner loop's stop in [14]:
//   [0] status  [1] outer iterations  [2] trials  [3] accepted trials  [4] phi first  [5] phi  [6] delta  [7] the last step's ||g||
//   [8] max viol first  [9] max viol  [10] penalty increases  [11] sum of the steps' CG iterations  [12] pairs harvested  [13] fallbacks
#pragma once

#include <cstdint>
#include <vector>

#include "dto_auglag_plan.h"
#include "dto_newton_plan.h"

namespace dto {

// exit status of the call (DTO_MINIMIZE_* in include/dto_engine.h); MINIMIZE_RUNNING: the loop goes on
enum { MINIMIZE_RUNNING = -1, MINIMIZE_CONVERGED = 0, MINIMIZE_MAX_OUTER = 1, MINIMIZE_MAX_TRIALS = 2, MINIMIZE_RADIUS = 3, MINIMIZE_NOT_FINITE = 4 };
// how an inner loop ended
enum { MIN_STOP_NONE = 0, MIN_STOP_GRADIENT = 1, MIN_STOP_RADIUS = 2, MIN_STOP_NOT_FINITE = 3, MIN_STOP_MAX_TRIALS = 4 };
// options (DTO_MIN_OPT_*)
enum { MIN_OPT_RADIUS0 = 0, MIN_OPT_ETA_ACCEPT = 1, MIN_OPT_ETA_SHRINK = 2, MIN_OPT_ETA_GROW = 3, MIN_OPT_SHRINK_DIV = 4, MIN_OPT_GROW_MUL = 5,
       MIN_OPT_RADIUS_MAX = 6, MIN_OPT_RADIUS_MIN = 7, MIN_OPT_GTOL = 8, MIN_OPT_CTOL = 9, MIN_OPT_VIOL_DIV = 10, MIN_OPT_RHO_MUL = 11,
       MIN_OPT_SHIFT = 12, MIN_OPT_RTOL = 13, MIN_OPT_ATOL = 14, MIN_OPT_MAX_ITER = 15, MINIMIZE_OPTIONS = 16 };
// info / the scalars
enum { MNS_STATUS = 0, MNS_OUTER = 1, MNS_TRIALS = 2, MNS_ACCEPTED = 3, MNS_PHI_FIRST = 4, MNS_PHI = 5, MNS_DELTA = 6, MNS_GNORM = 7,
       MNS_VIOL_FIRST = 8, MNS_VIOL = 9, MNS_GREW = 10, MNS_CG = 11, MNS_HARVESTED = 12, MNS_FALLBACKS = 13, MNS_INNER_STOP = 14,
       MINIMIZE_STATE = 16, MINIMIZE_INFO = 16 };
constexpr int MINIMIZE_HISTORY = 8, MINIMIZE_OUTER_HISTORY = 4, MINIMIZE_MAIL = 4, MINIMIZE_STEP_INFO = 16;
// the mailbox a launch leaves for the host: what it accepted (a trial) or whether rho grew (an outer iteration), delta for the next
// step, whether the loop it belongs to ends, phi
enum { MNM_ACCEPTED = 0, MNM_DELTA = 1, MNM_STOP = 2, MNM_PHI = 3 };

struct MinimizeOptions { double v[MINIMIZE_OPTIONS]; };

NWT_HD inline MinimizeOptions minimize_default_options() {
    MinimizeOptions o{};
    o.v[MIN_OPT_RADIUS0] = 1.0; o.v[MIN_OPT_ETA_ACCEPT] = 0.1; o.v[MIN_OPT_ETA_SHRINK] = 0.25; o.v[MIN_OPT_ETA_GROW] = 0.75;
    o.v[MIN_OPT_SHRINK_DIV] = 4.0; o.v[MIN_OPT_GROW_MUL] = 2.0; o.v[MIN_OPT_RADIUS_MAX] = __builtin_huge_val(); o.v[MIN_OPT_RADIUS_MIN] = 0.0;
    o.v[MIN_OPT_GTOL] = 0.0; o.v[MIN_OPT_CTOL] = 0.0; o.v[MIN_OPT_VIOL_DIV] = 4.0; o.v[MIN_OPT_RHO_MUL] = 10.0;
    o.v[MIN_OPT_SHIFT] = 0.0; o.v[MIN_OPT_RTOL] = 1e-6; o.v[MIN_OPT_ATOL] = 0.0; o.v[MIN_OPT_MAX_ITER] = 50.0;
    return o;
}

struct MinimizeTrial {
    double ratio;
    int accepted;
    double delta_next;
    int stop;   // MIN_STOP_NONE, MIN_STOP_RADIUS or MIN_STOP_NOT_FINITE
};

NWT_HD inline MinimizeTrial minimize_trial_decide(double phi, double phi_t, double predicted, int step_status, double delta, const double* opt) {
    const double ratio = newton_div(newton_sub(phi, phi_t), predicted);
    if (step_status == NEWTON_NOT_FINITE || !newton_finite(ratio)) return MinimizeTrial{ratio, 0, delta, MIN_STOP_NOT_FINITE};
    MinimizeTrial D{ratio, ratio > opt[MIN_OPT_ETA_ACCEPT] ? 1 : 0, delta, MIN_STOP_NONE};
    if (ratio < opt[MIN_OPT_ETA_SHRINK]) {
        D.delta_next = newton_div(delta, opt[MIN_OPT_SHRINK_DIV]);
    } else if (ratio > opt[MIN_OPT_ETA_GROW] && step_status != NEWTON_CONVERGED) {
        const double grown = newton_mul(delta, opt[MIN_OPT_GROW_MUL]);
        D.delta_next = opt[MIN_OPT_RADIUS_MAX] < grown ? opt[MIN_OPT_RADIUS_MAX] : grown;
    }
    if (D.delta_next < opt[MIN_OPT_RADIUS_MIN]) D.stop = MIN_STOP_RADIUS;
    return D;
}

struct MinimizeOuter {
    int grew;
    int stop;   // 1: max viol <= ctol
};

NWT_HD inline MinimizeOuter minimize_outer_decide(double viol, double new_viol, const double* opt) {
    return MinimizeOuter{!(new_viol <= newton_div(viol, opt[MIN_OPT_VIOL_DIV])) ? 1 : 0, new_viol <= opt[MIN_OPT_CTOL] ? 1 : 0};
}
NWT_HD inline double minimize_rho_next(double rho, int grew, const double* opt) {
    return (grew && rho != 0.0) ? newton_mul(rho, opt[MIN_OPT_RHO_MUL]) : rho;
}

// what a trial's launch is told (the host knows these when it enqueues) and what it reads from the device
struct MinimizeTrialFlags {
    int first_call;    // the first trial of the call: phi first is recorded
    int first_trial;   // the first trial of an outer iteration: delta = radius0, one more outer iteration
    int last_trial;    // the inner loop ends here with MAX_TRIALS unless it ends otherwise
    int gradient;      // the step's ||g|| <= gtol: no merit was made
    int has_rho;
    int step_info;     // 16: the preconditioned step's info (harvested, fallbacks in [13], [14]); 12: the box step's
};

// the scalars behind a trial: `in` the bank the launch reads, `out` the bank it writes; sinfo the step's info, phi_t the trial's merit
// value (not read for a gradient trial); row [8] the history row, mail [4].  Returns the decision.
NWT_HD inline MinimizeTrial minimize_trial_update(const double* in, double* out, const double* sinfo, double phi_t, const MinimizeTrialFlags& F,
                                                  const double* opt, double* row, double* mail) {
    const double phi = in[MNS_PHI], delta = F.first_trial ? opt[MIN_OPT_RADIUS0] : in[MNS_DELTA];
    const int step_status = (int)sinfo[0];
    MinimizeTrial D{0.0, 0, delta, MIN_STOP_GRADIENT};
    if (F.gradient) phi_t = phi;
    else D = minimize_trial_decide(phi, phi_t, sinfo[6], step_status, delta, opt);
    int stop = D.stop;
    if (stop == MIN_STOP_NONE && F.last_trial) stop = MIN_STOP_MAX_TRIALS;
    for (int i = 0; i < MINIMIZE_STATE; ++i) out[i] = in[i];
    if (F.first_call) out[MNS_PHI_FIRST] = phi;
    if (F.first_trial) out[MNS_OUTER] = newton_add(in[MNS_OUTER], 1.0);
    out[MNS_TRIALS] = newton_add(in[MNS_TRIALS], 1.0);
    out[MNS_ACCEPTED] = newton_add(in[MNS_ACCEPTED], D.accepted ? 1.0 : 0.0);
    out[MNS_PHI] = D.accepted ? phi_t : phi;
    out[MNS_DELTA] = D.delta_next;
    out[MNS_GNORM] = sinfo[2];
    out[MNS_CG] = newton_add(in[MNS_CG], sinfo[1]);
    if (F.step_info >= 16) {
        out[MNS_HARVESTED] = newton_add(in[MNS_HARVESTED], sinfo[13]);
        out[MNS_FALLBACKS] = newton_add(in[MNS_FALLBACKS], sinfo[14]);
    }
    out[MNS_INNER_STOP] = (double)stop;
    int status = MINIMIZE_RUNNING;
    if (stop == MIN_STOP_NOT_FINITE) status = MINIMIZE_NOT_FINITE;
    else if (!F.has_rho && stop != MIN_STOP_NONE)
        status = stop == MIN_STOP_GRADIENT ? MINIMIZE_CONVERGED : stop == MIN_STOP_RADIUS ? MINIMIZE_RADIUS : MINIMIZE_MAX_TRIALS;
    out[MNS_STATUS] = (double)status;
    if (row) {
        row[0] = D.ratio; row[1] = D.accepted ? 1.0 : 0.0; row[2] = delta; row[3] = phi_t;
        row[4] = sinfo[6]; row[5] = sinfo[0]; row[6] = sinfo[1]; row[7] = sinfo[2];
    }
    mail[MNM_ACCEPTED] = D.accepted ? 1.0 : 0.0; mail[MNM_DELTA] = D.delta_next; mail[MNM_STOP] = (double)stop; mail[MNM_PHI] = out[MNS_PHI];
    return D;
}

// the scalars behind an outer iteration: rinfo the row pass's eight scalars behind the inner loop, viol0 the first max viol (read in
// the first outer iteration only); row [4], mail [4].  Returns the decision.
NWT_HD inline MinimizeOuter minimize_outer_update(const double* in, double* out, const double* rinfo, double viol0, int first_outer, int last_outer,
                                                  const double* opt, double* row, double* mail) {
    const double viol = first_outer ? viol0 : in[MNS_VIOL], new_viol = rinfo[AL_MAX_VIOL];
    const MinimizeOuter D = minimize_outer_decide(viol, new_viol, opt);
    for (int i = 0; i < MINIMIZE_STATE; ++i) out[i] = in[i];
    if (first_outer) out[MNS_VIOL_FIRST] = viol0;
    out[MNS_VIOL] = new_viol;
    out[MNS_GREW] = newton_add(in[MNS_GREW], D.grew ? 1.0 : 0.0);
    int status = MINIMIZE_RUNNING;
    if ((int)in[MNS_INNER_STOP] == MIN_STOP_GRADIENT && D.stop) status = MINIMIZE_CONVERGED;
    else if (last_outer) status = MINIMIZE_MAX_OUTER;
    out[MNS_STATUS] = (double)status;
    if (row) { row[0] = new_viol; row[1] = D.grew ? 1.0 : 0.0; row[2] = rinfo[AL_ACTIVE]; row[3] = rinfo[AL_P]; }
    mail[MNM_ACCEPTED] = D.grew ? 1.0 : 0.0; mail[MNM_DELTA] = in[MNS_DELTA]; mail[MNM_STOP] = status != MINIMIZE_RUNNING ? 1.0 : 0.0;
    mail[MNM_PHI] = in[MNS_PHI];
    return D;
}

// info from the scalars: the inner loop's stop is not part of it
NWT_HD inline void minimize_info_store(const double* state, double* info) {
    for (int i = 0; i < MINIMIZE_INFO; ++i) info[i] = i < MNS_INNER_STOP ? state[i] : 0.0;
}

// ---- the whole loop on host arrays (the statement of the algorithm; the device routine is these steps as launches) --------------------
// Z [n] in / out; mu, rho [n_cons] in / out or null (rho null: one outer iteration, mu is not written); the rows r < n_dyn of mu and rho
// are left as they are.  opt [16].
//   step(Z, delta, Zp, sinfo)   the trial point Zp [n] and the step's info (12 or step_info = 16 doubles) at Z with radius delta
//   merit(Zin, Zout) -> phi     Zout [n] = the feasible trajectory of Zin (Zout == Zin allowed) and the merit value there
//   rows(Z, mu_eff, rinfo)      mu_eff [n_cons] and the row pass's AL_INFO scalars at Z            (called with rho only)
// step, merit and rows read mu and rho as they stand.  info [16]; history [outer * trials][8] and outer_history [outer][4] may be
// null; rows past the last trial / outer iteration are left as they are.
template <class Step, class Merit, class Rows>
inline void minimize_solve(int64_t n, int64_t n_cons, int64_t n_dyn, double* Z, double* mu, double* rho, const double* opt, int outer, int trials,
                           int step_info, Step&& step, Merit&& merit, Rows&& rows, double* info, double* history, double* outer_history) {
    std::vector<double> Zp((size_t)n), Zt((size_t)n), mu_eff((size_t)(n_cons > 0 ? n_cons : 1));
    double bank[2][MINIMIZE_STATE] = {}, sinfo[MINIMIZE_STEP_INFO] = {}, rinfo0[AL_INFO] = {}, rinfo[AL_INFO] = {}, mail[MINIMIZE_MAIL] = {};
    int q = 0;   // launches so far: bank q % 2 is current
    if (!rho) outer = 1;
    if (rho) rows(Z, mu_eff.data(), rinfo0);
    int64_t trial = 0;
    for (int o = 0; o < outer; ++o) {
        bank[q % 2][MNS_PHI] = merit(Z, Z);
        double delta = opt[MIN_OPT_RADIUS0];
        int stop = MIN_STOP_NONE;
        for (int t = 0; t < trials && stop == MIN_STOP_NONE; ++t, ++trial) {
            step(Z, delta, Zp.data(), sinfo);
            MinimizeTrialFlags F{q == 0, t == 0, t == trials - 1, sinfo[2] <= opt[MIN_OPT_GTOL], rho != nullptr, step_info};
            const double phi_t = F.gradient ? 0.0 : merit(Zp.data(), Zt.data());
            const MinimizeTrial D = minimize_trial_update(bank[q % 2], bank[(q + 1) % 2], sinfo, phi_t, F, opt,
                                                          history ? history + MINIMIZE_HISTORY * trial : nullptr, mail);
            if (D.accepted)
                for (int64_t i = 0; i < n; ++i) Z[i] = Zt[(size_t)i];
            ++q;
            delta = mail[MNM_DELTA];
            stop = (int)mail[MNM_STOP];
        }
        if (stop == MIN_STOP_NOT_FINITE || !rho) break;
        rows(Z, mu_eff.data(), rinfo);
        const MinimizeOuter D = minimize_outer_update(bank[q % 2], bank[(q + 1) % 2], rinfo, rinfo0[AL_MAX_VIOL], o == 0, o == outer - 1, opt,
                                                      outer_history ? outer_history + MINIMIZE_OUTER_HISTORY * o : nullptr, mail);
        for (int64_t r = n_dyn; r < n_cons; ++r) {
            mu[r] = mu_eff[(size_t)r];
            rho[r] = minimize_rho_next(rho[r], D.grew, opt);
        }
        ++q;
        if (mail[MNM_STOP] != 0.0) break;
    }
    minimize_info_store(bank[q % 2], info);
}

}  // namespace dto
