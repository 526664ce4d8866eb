// dto_input_plan.h -- plan of the reduced-space operators' input-block store (option "reduced_input_store"; kernels: dto_reduced.hip):
// which knot components are FREE INPUTS of which integrator, where each integrator's input blocks sit in the compact store, and which
// (integrator, column) terms read a knot component.  Plain C++ (no HIP header, no engine header), like dto_elim_plan.h, whose
// ElimIntegrator and position function it uses: the same functions serve the host routine (dto_engine.cpp), the kernels and a
// g++-built test (tests/test_input_plan_header.py).
//
// The inputs of integrator a are those dto_elim_plan.h names: [in_off, in_off + in_dim), dt_idx and, for the time-dependent kind,
// t_off.  A FREE input is an input component that is no integrator's state; fin_a lists them by ascending component index (each once)
// and Wf_a is their number (0 is legal: no store, no terms).
//
// Input store.  F_a holds, per interval k = 0 .. K - 1, a's rows of that interval in the columns of its free inputs at knot k (half 0)
// and at knot k + 1 (half 1):  F_a [K][2][Wf_a][x_dim_a], rows contiguous, positions by elim_block_pos(Wf_a, x_dim_a, k, half, j).
// Both halves are always stored.  The stores of all integrators lie one behind the other in list order.
//
// A knot component is a STATE (of some integrator), READ (a free input of at least one integrator: its terms (a, j), j the column
// inside F_a, in list order of a) or UNREAD (neither).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "dto_elim_plan.h"

namespace dto {

enum { INPUT_STATE = 0, INPUT_READ = 1, INPUT_UNREAD = 2 };

struct InputTerm {
    int a;   // the integrator that reads the component (list position)
    int j;   // its column inside the Wf_a columns of F_a
};

struct InputPlan {
    std::vector<std::vector<int>> fin;          // [I] free inputs, ascending component index
    std::vector<int> width;                     // [I] Wf_a
    std::vector<int64_t> store_off;             // [I + 1] first double of F_a in the input store (K intervals)
    std::vector<int> kind;                      // [z] INPUT_*
    std::vector<std::vector<InputTerm>> terms;  // [z] who reads the component, in list order
};

// is component c a state of some integrator?
inline bool input_is_state(const std::vector<ElimIntegrator>& its, int c) {
    for (const ElimIntegrator& b : its)
        if (elim_meets(b.x_off, b.x_dim, c, 1)) return true;
    return false;
}

// is component c an input of `a`?
inline bool input_reads(const ElimIntegrator& a, int dt_idx, int c) { return elim_reads(a, dt_idx, c, 1); }

inline InputPlan input_plan(const std::vector<ElimIntegrator>& its, int dt_idx, int z, int64_t K) {
    InputPlan p;
    const int I = (int)its.size();
    p.fin.assign(I, {});
    p.width.assign(I, 0);
    p.kind.assign((size_t)(z > 0 ? z : 0), INPUT_UNREAD);
    p.terms.assign((size_t)(z > 0 ? z : 0), {});
    for (int c = 0; c < z; ++c) {
        if (input_is_state(its, c)) {
            p.kind[c] = INPUT_STATE;
            continue;
        }
        for (int a = 0; a < I; ++a)
            if (input_reads(its[a], dt_idx, c)) {
                p.terms[c].push_back(InputTerm{a, p.width[a]});
                p.fin[a].push_back(c);
                ++p.width[a];
                p.kind[c] = INPUT_READ;
            }
    }
    p.store_off.assign(I + 1, 0);
    for (int a = 0; a < I; ++a) p.store_off[a + 1] = p.store_off[a] + (K > 0 ? K : 0) * elim_interval_doubles(p.width[a], its[a].x_dim);
    return p;
}

}  // namespace dto
