// dto_elim_plan.h -- plan of the whole-dynamics solves (dto_dynamics_solve_all / dto_dynamics_solve_all_dev, dto_elim.hip): which
// integrator's states feed which integrator's rows, the order in which the block elimination visits the integrators, and where each
// integrator's coupling blocks sit in the compact store.  Plain C++ (no HIP header, no engine header), like dto_rollout_plan.h: the
// same functions serve the host routine (dto_engine.cpp), the kernels (dto_elim.hip) and a g++-built test
// (tests/test_elim_plan_header.py).
//
// Integrator a has the state components S_a = [x_off, x_off + x_dim) and reads, besides them, its INPUTS:
//   bilinear        [in_off, in_off + in_dim) (the controls) and dt_idx
//   time-dependent  the same and t_off
//   derivative      [in_off, in_off + x_dim) (the derivative's components) and dt_idx
// a DEPENDS on b != a when S_b meets a's inputs.  level(a) = 0 without dependencies, else 1 + max level(deps).  The forward solve
// visits the integrators by (level, list position) ascending, the adjoint solve in the reverse of that order.
//
// Coupling store.  C_a holds, per interval k = 0 .. K - 1, a's rows of that interval in the columns of its dependencies' states at
// knot k (half 0) and at knot k + 1 (half 1):  C_a [K][2][W_a][x_dim_a], rows contiguous, W_a the sum of x_dim_b over deps(a) in list
// order (column dep_col(a, b) + j is component j of S_b).  The stores of all integrators lie one behind the other in list order.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define ELP_HD __host__ __device__
#else
#define ELP_HD
#endif

namespace dto {

enum { ELIM_BILINEAR = 0, ELIM_DERIVATIVE = 1, ELIM_TIME_DEPENDENT = 2 };

struct ElimIntegrator {
    int kind;              // ELIM_*
    int x_off, x_dim;      // states
    int in_off, in_dim;    // controls (bilinear, time-dependent) or the derivative's components (derivative: in_dim = x_dim)
    int t_off;             // time component (time-dependent), -1 otherwise
};

struct ElimDep {
    int b;       // the integrator depended on (list position)
    int col;     // first column of S_b inside the W_a columns of a's coupling blocks
};

struct ElimPlan {
    std::string refusal;                       // empty: the plan holds
    int n_states = 0, n_levels = 0;            // D, and 1 + the highest level
    std::vector<int> pre;                      // [I] states of the integrators before i in list order
    std::vector<int> level;                    // [I]
    std::vector<int> order;                    // [I] forward processing order (list positions)
    std::vector<std::vector<ElimDep>> deps;    // [I] dependencies in list order
    std::vector<std::vector<int>> dependents;  // [I] who depends on i, in list order
    std::vector<int> width;                    // [I] W_a
    std::vector<int64_t> store_off;            // [I + 1] first double of C_a in the coupling store (K intervals)
};

inline bool elim_meets(int lo, int len, int lo2, int len2) { return len > 0 && len2 > 0 && lo < lo2 + len2 && lo2 < lo + len; }

// does S (x_off, x_dim) meet the inputs of `a`?
inline bool elim_reads(const ElimIntegrator& a, int dt_idx, int x_off, int x_dim) {
    if (elim_meets(a.in_off, a.in_dim, x_off, x_dim)) return true;
    if (elim_meets(dt_idx, 1, x_off, x_dim)) return true;
    return a.kind == ELIM_TIME_DEPENDENT && elim_meets(a.t_off, 1, x_off, x_dim);
}

// doubles of one interval of C_a
ELP_HD inline int64_t elim_interval_doubles(int width, int x_dim) { return (int64_t)2 * width * x_dim; }
// position inside C_a of (interval k, half, column j, row 0)
ELP_HD inline int64_t elim_block_pos(int width, int x_dim, int64_t k, int half, int j) {
    return (k * 2 + half) * (int64_t)width * x_dim + (int64_t)j * x_dim;
}

inline ElimPlan elim_plan(const std::vector<ElimIntegrator>& its, int dt_idx, int64_t K) {
    ElimPlan p;
    const int I = (int)its.size();
    p.pre.assign(I, 0);
    for (int i = 0; i < I; ++i) {
        p.pre[i] = p.n_states;
        p.n_states += its[i].x_dim;
    }
    for (int a = 0; a < I; ++a)
        for (int b = a + 1; b < I; ++b)
            if (elim_meets(its[a].x_off, its[a].x_dim, its[b].x_off, its[b].x_dim)) {
                p.refusal = "the states of integrators " + std::to_string(a) + " and " + std::to_string(b) + " overlap";
                return p;
            }
    for (int a = 0; a < I; ++a)
        if (elim_reads(its[a], dt_idx, its[a].x_off, its[a].x_dim)) {
            p.refusal = "the inputs of integrator " + std::to_string(a) + " meet its own states";
            return p;
        }
    p.deps.assign(I, {});
    p.dependents.assign(I, {});
    p.width.assign(I, 0);
    for (int a = 0; a < I; ++a)
        for (int b = 0; b < I; ++b)
            if (b != a && elim_reads(its[a], dt_idx, its[b].x_off, its[b].x_dim)) {
                p.deps[a].push_back(ElimDep{b, p.width[a]});
                p.width[a] += its[b].x_dim;
                p.dependents[b].push_back(a);
            }
    // levels: longest path; more than I rounds of relaxation mean a cycle
    p.level.assign(I, 0);
    for (int round = 0;; ++round) {
        bool changed = false;
        for (int a = 0; a < I; ++a)
            for (const ElimDep& d : p.deps[a])
                if (p.level[a] < p.level[d.b] + 1) { p.level[a] = p.level[d.b] + 1; changed = true; }
        if (!changed) break;
        if (round >= I) {
            p.refusal = "the integrators depend on each other in a cycle";
            return p;
        }
    }
    for (int a = 0; a < I; ++a) p.n_levels = p.level[a] + 1 > p.n_levels ? p.level[a] + 1 : p.n_levels;
    for (int l = 0; l < p.n_levels; ++l)
        for (int a = 0; a < I; ++a)
            if (p.level[a] == l) p.order.push_back(a);
    p.store_off.assign(I + 1, 0);
    for (int a = 0; a < I; ++a) p.store_off[a + 1] = p.store_off[a] + (K > 0 ? K : 0) * elim_interval_doubles(p.width[a], its[a].x_dim);
    return p;
}

}  // namespace dto
