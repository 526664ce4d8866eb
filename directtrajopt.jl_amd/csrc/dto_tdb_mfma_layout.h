// dto_tdb_mfma_layout.h -- the scratch slot of one resident workgroup of k_tdb_mfma (dto_tdb_mfma.hip) and the column layout of
// its calls.  Plain C++ (no HIP header, no engine header), in the manner of dto_tdb_scheme.h: the kernel, its launchers, the host's
// sizing (dto_create.cpp through tdb_mfma_scratch_doubles) and a g++-built test (tests/test_tdb_mfma_layout.py) read one text.
#pragma once

#include <cstddef>

#include "dto_tdb_scheme.h"

namespace dto {

constexpr int TDBM_VEC = 32;   // column tile of the vector block

TDB_HD inline int tdbm_pad32(int v) { return (v + 31) / 32 * 32; }

// Columns of one call (np rows each) and the slot in doubles: four column sets, M0, the U_q vectors, ubar of the adjoint, the
// coefficient table.  `members` integrators of one system side by side (1: a lone integrator; need 3 / 4, the product modes, exist
// at one member only).  need 0 / 1 / 2: defect, Jacobian, Hessian; 3: J w (x, d); 4: J' w (x, x_b).
struct TdbmLayout {
    int np, p, P2, Q, C1, cstride, Cv, Ctot, ustep, ucols;
    size_t oY, oACC, oTA, oTB, oM0, oU, oUB, oCoef, total;
};
TDB_HD inline TdbmLayout tdbm_layout(int n, int m, int order, int nmod, int need, int members) {
    TdbmLayout L;
    L.np = tdbm_pad32(n);
    L.p = tdb_num_params(m, order);
    L.P2 = tdb_num_pairs(L.p);
    L.Q = tdb_num_shared(m, nmod);
    // meaningful columns of one member
    L.C1 = need == 0 ? 1 : (need == 3 ? 2 : (need == 1 || need == 4 ? 1 + L.p : 1 + L.p + L.P2));
    L.cstride = need == 2 ? tdbm_pad32(L.C1) : L.C1;   // columns from one member to the next
    L.Cv = tdbm_pad32(members * L.cstride);
    L.Ctot = L.Cv + (need == 1 ? L.np : 0);            // the Phi block, one for the group
    L.ustep = need == 2 ? TDBM_VEC : 1;                // U columns of one member and q
    L.ucols = members * L.ustep;
    const size_t cols = (size_t)L.np * L.Ctot;
    L.oY = 0; L.oACC = cols; L.oTA = 2 * cols; L.oTB = 3 * cols;
    L.oM0 = 4 * cols;
    L.oU = L.oM0 + (size_t)L.np * L.np;
    L.oUB = L.oU + (size_t)L.Q * L.ucols * L.np;
    // ubar: a 32-column tile per member in a Hessian call; a lone integrator keeps one tile in every call (need 4 uses a column)
    L.oCoef = L.oUB + (members == 1 || need == 2 ? (size_t)L.np * TDBM_VEC * members : 0);
    L.total = L.oCoef + (size_t)(1 + L.p + L.P2) * L.Q;
    L.total = (L.total + 1) & ~(size_t)1;
    return L;
}

}  // namespace dto
