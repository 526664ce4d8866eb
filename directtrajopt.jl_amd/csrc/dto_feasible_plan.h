// dto_feasible_plan.h -- schedule of the feasible-trajectory rollout (dto_feasible_trajectory / dto_feasible_merit and their _dev forms,
// dto_feasible.hip): in which order the integrators' states of knots 2 .. N are rebuilt from the states of knot 1, and where the
// Jacobian is evaluated on the way.  Plain C++ (no HIP header, no engine header), like dto_elim_plan.h and dto_reduced_plan.h: the
// same function serves the host routine (dto_engine.cpp) and a g++-built test (tests/test_feasible_plan_header.py).
//
// Input: per integrator (list order) its dependency level (dto_elim_plan.h: 0 without dependencies, else 1 + the highest level among
// the integrators whose states it reads) and whether it has a propagator (bilinear, time-dependent) or is a DerivativeIntegrator.
// Levels run ascending.  Inside a level:
//   1. DERIV(i) for every DerivativeIntegrator of the level, in list order: x_{k+1} = x_k + dt_k xdot_k, serial in the knots;
//   2. ONE JACOBIAN when the level holds an integrator with a propagator: the Jacobian at the trajectory built so far, which then
//      holds -E_k of every such integrator of the level (E_k reads no state of its own level);
//   3. ROLL(i) for every integrator with a propagator, in list order: its product tree from that Jacobian, the descent from its
//      knot-1 state, the scatter into the trajectory.
// Every integrator appears in exactly one step; a JACOBIAN step names its level and no integrator.
#pragma once

#include <vector>

namespace dto {

enum { FEAS_DERIV = 0, FEAS_JACOBIAN = 1, FEAS_ROLL = 2 };

struct FeasibleStep {
    int kind;         // FEAS_*
    int integrator;   // list position (DERIV, ROLL), -1 (JACOBIAN)
    int level;
};

struct FeasiblePlan {
    std::vector<FeasibleStep> steps;
    int n_jacobians = 0;   // JACOBIAN steps: the levels that hold a propagator
    int n_deriv = 0, n_roll = 0;
};

// level [I], has_propagator [I] (0: a DerivativeIntegrator)
inline FeasiblePlan feasible_plan(const std::vector<int>& level, const std::vector<int>& has_propagator) {
    FeasiblePlan p;
    const int I = (int)level.size();
    int n_levels = 0;
    for (int i = 0; i < I; ++i) n_levels = level[i] + 1 > n_levels ? level[i] + 1 : n_levels;
    for (int l = 0; l < n_levels; ++l) {
        bool propagates = false;
        for (int i = 0; i < I; ++i) {
            if (level[i] != l) continue;
            if (has_propagator[i]) { propagates = true; continue; }
            p.steps.push_back(FeasibleStep{FEAS_DERIV, i, l});
            ++p.n_deriv;
        }
        if (!propagates) continue;
        p.steps.push_back(FeasibleStep{FEAS_JACOBIAN, -1, l});
        ++p.n_jacobians;
        for (int i = 0; i < I; ++i)
            if (level[i] == l && has_propagator[i]) {
                p.steps.push_back(FeasibleStep{FEAS_ROLL, i, l});
                ++p.n_roll;
            }
    }
    return p;
}

}  // namespace dto
