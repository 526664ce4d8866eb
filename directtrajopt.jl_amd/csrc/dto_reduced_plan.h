// dto_reduced_plan.h -- index plan of the reduced-space operators (dto_reduced_gradient / dto_reduced_hessian_product and their _dev
// forms, dto_reduced.hip): which entries of a Z-layout vector are integrator states, where they sit in the [N][1][D] layout of the
// whole-dynamics solves, and which constraint row belongs to (interval, state).  Plain C++ (no HIP header, no engine header), like
// dto_elim_plan.h and dto_rollout_plan.h: the same functions serve the host routine (dto_engine.cpp), the kernels (dto_reduced.hip) and
// a g++-built test (tests/test_reduced_plan_header.py).
//
// A Z-layout vector has n_vars = N z + gd entries: z components per knot, then gd globals.  Integrator i (list order) owns the state
// components [x_off, x_off + x_dim) of every knot, the D-axis positions [pre, pre + x_dim) (pre: the dimensions before it in list order,
// D their sum) and the constraint rows row0 + k x_dim + r for interval k (0-based) and component r.  An entry of Z is
//   a STATE of knot k   when its component lies in some integrator's [x_off, x_off + x_dim);
//   DEPENDENT           when it is a state of a knot k >= 1 (the set S the dynamics determine);
//   FREE                otherwise (controls, timesteps, times, the states of knot 0, globals).
// The tables below answer each question with one load: comp_pos [z] (component -> D position, -1: no state), pos_comp [D] (D position
// -> component), pos_dim [D] (x_dim of the owner) and pos_row [D] (row0 of the owner + r).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define RDP_HD __host__ __device__
#else
#define RDP_HD
#endif

namespace dto {

struct ReducedIntegrator {
    int x_off, x_dim;   // states
    int pre;            // first position on the D axis
    int64_t row0;       // first constraint row
};

// what the index functions read: the four tables (host pointers in a CPU build, device pointers in a kernel) and the sizes
struct KReduced {
    const int32_t* comp_pos;   // [z]
    const int32_t* pos_comp;   // [D]
    const int32_t* pos_dim;    // [D]
    const int64_t* pos_row;    // [D]
    int32_t z, D;
    int64_t N, n_vars, n_cons, n_dyn;
};

struct ReducedPlan {
    std::vector<int32_t> comp_pos, pos_comp, pos_dim;
    std::vector<int64_t> pos_row;
    int D = 0;
};

// (states that overlap are refused by dto_elim_plan.h before this plan is asked for)
inline ReducedPlan reduced_plan(const std::vector<ReducedIntegrator>& its, int z) {
    ReducedPlan p;
    for (const ReducedIntegrator& it : its) p.D = it.pre + it.x_dim > p.D ? it.pre + it.x_dim : p.D;
    p.comp_pos.assign((size_t)(z > 0 ? z : 0), -1);
    p.pos_comp.assign((size_t)p.D, -1);
    p.pos_dim.assign((size_t)p.D, 0);
    p.pos_row.assign((size_t)p.D, -1);
    for (const ReducedIntegrator& it : its)
        for (int r = 0; r < it.x_dim; ++r) {
            p.comp_pos[(size_t)(it.x_off + r)] = it.pre + r;
            p.pos_comp[(size_t)(it.pre + r)] = it.x_off + r;
            p.pos_dim[(size_t)(it.pre + r)] = it.x_dim;
            p.pos_row[(size_t)(it.pre + r)] = it.row0 + r;
        }
    return p;
}

inline KReduced reduced_view(const ReducedPlan& p, int z, int64_t N, int64_t n_vars, int64_t n_cons, int64_t n_dyn) {
    return KReduced{p.comp_pos.data(), p.pos_comp.data(), p.pos_dim.data(), p.pos_row.data(), z, p.D, N, n_vars, n_cons, n_dyn};
}

// knot of Z entry c (N: a global)
RDP_HD inline int64_t reduced_knot(const KReduced& R, int64_t c) { return c < R.N * R.z ? c / R.z : R.N; }
// D position of Z entry c when it is a state of its knot, else -1
RDP_HD inline int reduced_state_pos(const KReduced& R, int64_t c) { return c < R.N * R.z ? R.comp_pos[c % R.z] : -1; }
// "entry c is a state of knot k"
RDP_HD inline bool reduced_is_state_of(const KReduced& R, int64_t c, int64_t k) { return reduced_knot(R, c) == k && reduced_state_pos(R, c) >= 0; }
// "entry c is dependent": a state of a knot past the first
RDP_HD inline bool reduced_is_dependent(const KReduced& R, int64_t c) { return reduced_state_pos(R, c) >= 0 && c >= R.z; }
// pack: the Z entry that position (k, d) of [N][1][D] gathers
RDP_HD inline int64_t reduced_pack_index(const KReduced& R, int64_t k, int d) { return k * R.z + R.pos_comp[d]; }
// unpack: the [N][1][D] position that the state entry c of Z takes (reduced_state_pos(c) >= 0)
RDP_HD inline int64_t reduced_unpack_index(const KReduced& R, int64_t c) { return (c / R.z) * R.D + R.comp_pos[c % R.z]; }
// the constraint row of interval k (0-based: knots k, k + 1) at D position d
RDP_HD inline int64_t reduced_dyn_row(const KReduced& R, int64_t k, int d) { return R.pos_row[d] + k * R.pos_dim[d]; }

}  // namespace dto
