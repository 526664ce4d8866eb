// dto_slab_layout.h -- the layout of the two value vectors, stated once: where an integrator's rows sit inside a Jacobian column and
// where the column's constraint entries begin; where a knot's Hessian block, a column of it and the tail of global-variable columns
// start.  Plain C++ (no HIP header, no engine header, no handle): the same functions run in the kernels (jac_pos and hess_pos of
// dto_kernels.h forward here; hess_pos_off spells hess_inner_col_pos out), in the host's structure, shard, plan and
// index builders (dto_create.cpp, dto_engine.cpp) and in a g++-built test (tests/test_slab_layout_header.py), which also holds
// the three device functions to it.  Positions are 0-based and global; a shard subtracts the start of its slab.
// The functions are templates over the type that carries N, K, z, D: SlabDims below on the host, the kernels' own KProb on the
// device (a copy into a SlabDims first moved scalar loads in thirty kernels).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define SLAB_HD __host__ __device__
#else
#define SLAB_HD
#endif

namespace dto {

struct SlabDims {
    int64_t N, K;   // knots, intervals (K = N - 1)
    int32_t z, D;   // components per knot, integrator rows per interval (the sum of the integrators' dimensions)
};

// ---- Jacobian, CSC.  A column of knot kn holds, per integrator in list order, its rows of interval kn-1 (part 0) and then its rows
// of interval kn (part 1), each part only where the interval exists; the constraint entries of the column follow in ascending row
// order.  Columns of global variables (kn >= N) hold constraint entries only.
template <class Dims> SLAB_HD inline bool jac_has_part(const Dims& L, int64_t kn, int part) { return part == 0 ? (kn >= 1 && kn < L.N) : kn < L.K; }
// adjacent intervals of a knot column (kn < N) ...
template <class Dims> SLAB_HD inline int jac_knot_cnt(const Dims& L, int64_t kn) { return (kn >= 1) + (kn < L.K); }
// ... and of any column: none for a global variable
template <class Dims> SLAB_HD inline int jac_col_cnt(const Dims& L, int64_t kn) { return kn >= L.N ? 0 : jac_knot_cnt(L, kn); }
// offset inside a knot column of row 0 of the integrator with `pre` rows of earlier integrators per interval and d rows of its own:
// from the column's count of adjacent intervals (a kernel has it at hand), or from the dimensions
SLAB_HD inline int64_t jac_part_off_cnt(int cnt, int64_t kn, int pre, int d, int part) {
    return (int64_t)pre * cnt + ((part == 1 && kn >= 1) ? d : 0);
}
template <class Dims> SLAB_HD inline int64_t jac_part_off(const Dims& L, int64_t kn, int pre, int d, int part) {
    return jac_part_off_cnt(jac_knot_cnt(L, kn), kn, pre, d, part);
}
// offset at which the column's constraint entries begin: the column's fixed length
template <class Dims> SLAB_HD inline int64_t jac_con_off(const Dims& L, int64_t kn) { return (int64_t)L.D * jac_col_cnt(L, kn); }

// ---- Hessian, upper triangle, CSC.  Block kn holds the columns of knot kn: column b lists the z rows of knot kn-1 (its off-diagonal
// part, kn >= 1) and then rows 0 .. b of knot kn (its diagonal part).  The blocks of all N knots are followed by the tail of
// global-variable columns.
// entries of the upper triangle of an n x n block (n of either integer width, the product in 64 bits)
template <class T> SLAB_HD inline int64_t hess_tri(T n) { return (int64_t)n * (n + 1) / 2; }
// rows of the off-diagonal part of a column
template <class Dims> SLAB_HD inline int64_t hess_off_width(const Dims& L, int64_t kn) { return kn == 0 ? 0 : L.z; }
// position of the first entry of column b of block kn >= 1: a full first block, kn - 1 blocks with both parts, b columns
template <class Dims> SLAB_HD inline int64_t hess_inner_col_pos(const Dims& L, int64_t kn, int b) {
    const int64_t z = L.z, tri = hess_tri(z);
    return tri + (kn - 1) * (z * z + tri) + (int64_t)b * z + hess_tri(b);
}
// column b of any block: position of its diagonal part, and of its first entry
template <class Dims> SLAB_HD inline int64_t hess_diag_pos(const Dims& L, int64_t kn, int b) {
    return kn == 0 ? hess_tri(b) : hess_inner_col_pos(L, kn, b) + hess_off_width(L, kn);
}
template <class Dims> SLAB_HD inline int64_t hess_col_pos(const Dims& L, int64_t kn, int b) { return hess_diag_pos(L, kn, b) - hess_off_width(L, kn); }
// start of block kn; at kn = N the number of entries in all blocks, where the tail begins
template <class Dims> SLAB_HD inline int64_t hess_block_start(const Dims& L, int64_t kn) { return hess_col_pos(L, kn, 0); }
template <class Dims> SLAB_HD inline int64_t hess_block_len(const Dims& L, int64_t kn) { return hess_block_start(L, kn + 1) - hess_block_start(L, kn); }
template <class Dims> SLAB_HD inline int64_t hess_block_of(const Dims& L, int64_t pos) {
    return pos < hess_block_len(L, 0) ? 0 : 1 + (pos - hess_block_len(L, 0)) / hess_block_len(L, 1);
}
// column b inside block kn: where it starts and how many entries it has
template <class Dims> SLAB_HD inline int64_t hess_col_start(const Dims& L, int64_t kn, int b) { return hess_col_pos(L, kn, b) - hess_block_start(L, kn); }
template <class Dims> SLAB_HD inline int64_t hess_col_len(const Dims& L, int64_t kn, int b) { return hess_off_width(L, kn) + b + 1; }

// Walks the block part in slab order and names the (row, col) of each position, 0-based.  Past the last block kn == N.
struct HessBlockCursor {
    SlabDims L;
    int64_t kn = 0;   // block
    int b = 0;        // column inside it
    int64_t r = 0;    // entry inside that column
    SLAB_HD explicit HessBlockCursor(const SlabDims& L_) : L(L_) {}
    SLAB_HD bool in_blocks() const { return kn < L.N; }
    SLAB_HD void seek(int64_t pos) {
        kn = hess_block_of(L, pos);
        const int64_t local = pos - hess_block_start(L, kn);
        int lo = 0, hi = L.z - 1;  // the last column whose entries start at or before `local`
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (hess_col_start(L, kn, mid) <= local) lo = mid; else hi = mid - 1;
        }
        b = lo;
        r = local - hess_col_start(L, kn, b);
    }
    SLAB_HD void next() {
        if (++r < hess_col_len(L, kn, b)) return;
        r = 0;
        if (++b < L.z) return;
        b = 0;
        ++kn;
    }
    SLAB_HD int64_t col() const { return kn * L.z + b; }
    SLAB_HD int64_t row() const {
        const int64_t w = hess_off_width(L, kn);
        return r < w ? (kn - 1) * L.z + r : kn * L.z + (r - w);
    }
};

}  // namespace dto
