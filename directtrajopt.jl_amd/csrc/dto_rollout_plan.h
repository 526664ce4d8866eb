// dto_rollout_plan.h -- index plan of the open-loop rollout (dto_rollout / dto_rollout_dev): a balanced binary tree of propagator
// products over the K = N - 1 intervals and the descent that turns its nodes into the states of every knot.  Plain C++ (no HIP
// header, no engine header): the same functions serve the host routine (dto_engine.cpp), the kernels (dto_rollout.hip) and a
// g++-built test (tests/test_rollout_plan_header.py).
//
// Tree.  L = levels(K) is the smallest L with 2^L >= K.  Level 0 holds 2^L leaves, leaf i = E_i for i < K and the identity for the
// rest; node j of level l is the product E_{(j+1) 2^l - 1} ... E_{j 2^l} of the 2^l leaves it covers.  Every level is stored in
// BIT-REVERSED order: node j of level l sits in slot rev(L - l, j) of that level.  The left children (even nodes) of a level are then
// its first half and the right children its second half, both in the slot order of their parents, so the next level is the
// contiguous batch  level[l+1][s] = level[l][half + s] * level[l][s],  s = 0 .. half - 1,  half = 2^(L-l-1).
// Levels lie one behind the other in one buffer of 2^(L+1) - 1 matrices.
//
// Descent.  S[0] = X0.  Item (l, i), l = L .. 1, i = 0 .. 2^(L-l) - 1, belongs to node i of level l, which covers the knots
// start = i 2^l .. start + 2^l: it forms S[mid] = (left child) * S[start], mid = start + 2^(l-1), and is LIVE when mid <= K.  The
// left child is node 2 i of level l - 1: slot rev(L - l, i) of that level's first half.  S[start] is a multiple of 2^l and was
// written at a higher level (or is S[0]), so one launch per level, top down, suffices.  The knot K = 2^L is nobody's midpoint: it
// comes from the root, written here as the item (L + 1, 0) whose "left child" is slot 0 of level L.  Every knot 1 .. K is the
// midpoint of exactly one live item.
#pragma once

#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RLP_HD __host__ __device__
#else
#define RLP_HD
#endif

namespace dto {

// smallest L with 2^L >= K (K >= 1)
RLP_HD inline int rollout_levels(int64_t K) {
    int L = 0;
    while (((int64_t)1 << L) < K) ++L;
    return L;
}

// the low `bits` bits of i in reverse order
RLP_HD inline int64_t rollout_rev(int bits, int64_t i) {
    int64_t r = 0;
    for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}

// slot of leaf i (interval i, 0-based) in level 0
RLP_HD inline int64_t rollout_leaf_slot(int L, int64_t i) { return rollout_rev(L, i); }

// nodes of level l and the position of its first node in the tree buffer, in matrices
RLP_HD inline int64_t rollout_level_len(int L, int l) { return (int64_t)1 << (L - l); }
RLP_HD inline int64_t rollout_level_off(int L, int l) { return ((int64_t)2 << L) - ((int64_t)2 << (L - l)); }
RLP_HD inline int64_t rollout_tree_matrices(int L) { return ((int64_t)2 << L) - 1; }

struct RolloutItem {
    int64_t node;    // position of the left factor in the tree buffer, in matrices
    int64_t start;   // knot whose state is multiplied (0-based: knot 0 holds X0)
    int64_t mid;     // knot whose state is written
    bool live;       // mid <= K
};
// item (l, i): l = 1 .. L with i < 2^(L-l), or the root's item (L + 1, 0)
RLP_HD inline RolloutItem rollout_item(int L, int64_t K, int l, int64_t i) {
    RolloutItem it;
    if (l == L + 1) {
        it.node = rollout_level_off(L, L);
        it.start = 0;
        it.mid = (int64_t)1 << L;
    } else {
        it.node = rollout_level_off(L, l - 1) + rollout_rev(L - l, i);
        it.start = i << l;
        it.mid = it.start + ((int64_t)1 << (l - 1));
    }
    it.live = it.mid <= K;
    return it;
}
// items of level l (the root's level L + 1 has one)
RLP_HD inline int64_t rollout_items(int L, int l) { return l == L + 1 ? 1 : (int64_t)1 << (L - l); }

// The item that writes knot t (1 <= t <= K), as (level, index): t = 2^(l-1) (2 i + 1), or the root's item for t = 2^L.  Following
// `start` from knot K down to 0 lists the at most L + 1 items the final state alone needs (mode DTO_ROLLOUT_FINAL).
RLP_HD inline void rollout_writer(int L, int64_t t, int& l, int64_t& i) {
    if (t == ((int64_t)1 << L)) { l = L + 1; i = 0; return; }
    l = 1;
    while (!((t >> (l - 1)) & 1)) ++l;
    i = t >> l;
}

// columns of the padded trajectory: whole 16-column tiles, whole 64-column tiles from 49 columns on (the descent's two column tiles)
RLP_HD inline int rollout_col_pad(int n_cols) { return n_cols <= 48 ? (n_cols + 15) / 16 * 16 : (n_cols + 63) / 64 * 64; }
RLP_HD inline int rollout_col_tile(int n_cols) { return n_cols <= 48 ? 16 : 64; }

// workspace of one rollout beside the private Jacobian slab, in bytes: the tree and the padded trajectory [K + 1][col_pad][npad]
RLP_HD inline size_t rollout_tree_bytes(int npad, int64_t K) {
    return (size_t)rollout_tree_matrices(rollout_levels(K)) * (size_t)npad * (size_t)npad * sizeof(double);
}
RLP_HD inline size_t rollout_traj_bytes(int npad, int64_t K, int n_cols) {
    return (size_t)(K + 1) * (size_t)rollout_col_pad(n_cols) * (size_t)npad * sizeof(double);
}
RLP_HD inline size_t rollout_workspace_bytes(int npad, int64_t K, int n_cols) {
    return rollout_tree_bytes(npad, K) + rollout_traj_bytes(npad, K, n_cols);
}

}  // namespace dto
