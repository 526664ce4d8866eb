// dto_rollout_plan.h -- index plan of the open-loop rollout (dto_rollout / dto_rollout_dev): a balanced binary tree of propagator
// products over the K = N - 1 intervals and the descent that turns its nodes into the states of every knot.  Plain C++ (no HIP
// header, no engine header): the same functions serve the host routine (dto_engine.cpp), the kernels (dto_rollout.hip) and a
// g++-built test (tests/test_rollout_plan_header.py).  The solves with the dynamics block (dto_dynamics_solve, dto_dynsolve.hip) scan
// the same tree: their index functions are at the end of this file (tests/test_dynamics_solve_plan_header.py).
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
// Those items in the order they are launched, highest level first: the first starts at knot 0, the last writes knot K.  Fills
// lv[c], ix[c] and returns their count, at most L + 1 (arrays of ROLLOUT_MAX_PATH hold any K).
constexpr int ROLLOUT_MAX_PATH = 64;
RLP_HD inline int rollout_final_path(int L, int64_t K, int* lv, int64_t* ix) {
    int cnt = 0;
    for (int64_t t = K; t > 0; t = rollout_item(L, K, lv[cnt - 1], ix[cnt - 1]).start) { rollout_writer(L, t, lv[cnt], ix[cnt]); ++cnt; }
    for (int a = 0, b = cnt - 1; a < b; ++a, --b) {
        const int l = lv[a]; lv[a] = lv[b]; lv[b] = l;
        const int64_t i = ix[a]; ix[a] = ix[b]; ix[b] = i;
    }
    return cnt;
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

// ---- solves with the dynamics block (dto_dynamics_solve / dto_dynamics_solve_dev): affine scans over the same tree.
//
// Every node of the tree gets an OFFSET block [col_pad][npad] beside its matrix, at the node's position in a second buffer of
// 2^(L+1) - 1 blocks.  A node (T, F) of the forward scan stands for  S[end] = T S[start] + F,  a node (T, D) of the adjoint scan for
// Lam[start] = T' Lam[end] + D;  both read the ONE matrix tree, the adjoint through a transposed left operand.
//   forward   leaf i carries B_{i+1} for i < K and zero otherwise;  S[0] = B_0
//             up-sweep   F[l+1][s] = T[l][half+s] F[l][s] + F[l][half+s]
//             descent    item (l, i) of rollout_item:  S[mid] = T[node] S[start] + F[node]
//   adjoint   leaf i carries B_i for i <= K and zero beyond (leaf K is an identity leaf when K < 2^L);  Lam[t] = 0 for t > K, and
//             Lam[2^L] = B_K when K = 2^L
//             up-sweep   D[l+1][s] = T[l][s]' D[l][half+s] + D[l][s]
//             descent    the root's item (L + 1, 0):  Lam[0] = T[root]' Lam[2^L] + D[root];  item (l, i), l = L .. 1, belongs to the
//                        RIGHT child of node i of level l:  Lam[mid] = T[node]' Lam[end] + D[node],  end = start + 2^l, live when
//                        mid <= K.  An end beyond K is zero and is not read (src_zero).
// Forward, every knot 1 .. K is written by exactly one live item; adjoint, every knot 0 .. K - 1, and knot K too when K < 2^L (when
// K = 2^L the loader places B_K there).  Levels run top down: what an item reads is a multiple of 2^l, written at a higher level, by
// the loader, or zero.

// up-sweep of level l into level l + 1, s = 0 .. 2^(L-l-1) - 1:  out = op(a) x + add;  `a` a position in the matrix tree, x / add /
// out positions in the offset tree
struct DynsolveUp {
    int64_t a, x, add, out;
};
RLP_HD inline DynsolveUp dynsolve_up(int L, int adjoint, int l, int64_t s) {
    const int64_t lo = rollout_level_off(L, l), half = rollout_level_len(L, l + 1);
    DynsolveUp u;
    u.a = adjoint ? lo + s : lo + half + s;
    u.x = adjoint ? lo + half + s : lo + s;
    u.add = u.a;
    u.out = rollout_level_off(L, l + 1) + s;
    return u;
}

// descent item (l, i), l = 1 .. L with i < 2^(L-l), or the root's item (L + 1, 0):  knot[dst] = op(T[node]) knot[src] + offset[node]
struct DynsolveItem {
    int64_t node;    // position of the matrix and of the offset block in their trees
    int64_t src;     // knot read
    int64_t dst;     // knot written
    bool live;
    bool src_zero;   // the knot read lies beyond K: zero, never read from memory
};
RLP_HD inline DynsolveItem dynsolve_item(int L, int64_t K, int adjoint, int l, int64_t i) {
    DynsolveItem d;
    if (!adjoint) {
        const RolloutItem it = rollout_item(L, K, l, i);
        d.node = it.node; d.src = it.start; d.dst = it.mid; d.live = it.live; d.src_zero = false;
        return d;
    }
    const int64_t P = (int64_t)1 << L;
    if (l == L + 1) {
        d.node = rollout_level_off(L, L);
        d.src = P;
        d.dst = 0;
        d.live = true;
    } else {
        d.node = rollout_level_off(L, l - 1) + ((int64_t)1 << (L - l)) + rollout_rev(L - l, i);
        d.dst = (i << l) + ((int64_t)1 << (l - 1));
        d.src = (i + 1) << l;
        d.live = d.dst <= K;
    }
    d.src_zero = d.src > K;
    return d;
}
// live items of level l of a descent, and those among them that multiply (the others copy their offset): for counting flops
RLP_HD inline int64_t dynsolve_live_items(int L, int64_t K, int adjoint, int l) {
    if (l == L + 1) return adjoint || K == ((int64_t)1 << L) ? 1 : 0;
    return ((K >> (l - 1)) + 1) >> 1;
}
RLP_HD inline int64_t dynsolve_product_items(int L, int64_t K, int adjoint, int l) {
    if (!adjoint) return dynsolve_live_items(L, K, 0, l);
    return l == L + 1 ? (K == ((int64_t)1 << L) ? 1 : 0) : K >> l;
}

// the loader: what leaf i's offset block holds, as a knot of B (-1: zero), and the one knot of the trajectory it fills besides
RLP_HD inline int64_t dynsolve_leaf_knot(int64_t K, int adjoint, int64_t i) { return adjoint ? (i <= K ? i : -1) : (i < K ? i + 1 : -1); }
struct DynsolveStart {
    int64_t knot;    // knot of the trajectory the loader writes (-1: none)
    int64_t from;    // knot of B it holds
};
RLP_HD inline DynsolveStart dynsolve_start(int L, int64_t K, int adjoint) {
    DynsolveStart s;
    if (!adjoint) { s.knot = 0; s.from = 0; }
    else if (K == ((int64_t)1 << L)) { s.knot = K; s.from = K; }
    else { s.knot = -1; s.from = -1; }
    return s;
}

// the offset tree, in bytes
RLP_HD inline size_t dynsolve_offset_bytes(int npad, int64_t K, int n_cols) {
    return (size_t)rollout_tree_matrices(rollout_levels(K)) * (size_t)rollout_col_pad(n_cols) * (size_t)npad * sizeof(double);
}

}  // namespace dto
