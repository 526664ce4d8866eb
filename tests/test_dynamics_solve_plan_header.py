"""CPU: the index plan of the solves with the dynamics block (dto_dynamics_solve, csrc/dto_rollout_plan.h) from plain C++.  A
stand-alone program is compiled with g++ (address and undefined-behaviour sanitizers on) against the header alone and prints, for
K = 1 .. 70 and both directions, the loader's leaves and start knot, the up-sweep's triples and the descent's items.  Both affine
scans are then carried out in NumPy with those indices and nothing else, on random orthogonal 3 x 3 E_k, and compared with the direct
recurrences  Y_{k+1} = E_k Y_k + B_{k+1}  and  Lam_k = E_k' Lam_{k+1} + B_k."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
KS = list(range(1, 71))

PROGRAM = r"""
#include <cstdio>
#include "dto_rollout_plan.h"
using namespace dto;

int main() {
    for (long K = 1; K <= 70; ++K) {
        const int L = rollout_levels(K);
        for (int adj = 0; adj < 2; ++adj) {
            printf("head %ld %d %d %ld\n", K, adj, L, (long)rollout_tree_matrices(L));
            printf("leaf %ld %d", K, adj);
            for (long i = 0; i < (1L << L); ++i) printf(" %ld:%ld", (long)(rollout_level_off(L, 0) + rollout_leaf_slot(L, i)), (long)dynsolve_leaf_knot(K, adj, i));
            printf("\n");
            const DynsolveStart st = dynsolve_start(L, K, adj);
            printf("start %ld %d %ld %ld\n", K, adj, (long)st.knot, (long)st.from);
            for (int l = 0; l < L; ++l)
                for (long s = 0; s < (long)rollout_level_len(L, l + 1); ++s) {
                    const DynsolveUp u = dynsolve_up(L, adj, l, s);
                    printf("up %ld %d %d %ld %ld %ld %ld\n", K, adj, l, (long)u.a, (long)u.x, (long)u.add, (long)u.out);
                }
            for (int l = L + 1; l >= 1; --l) {
                long live = 0, prod = 0;
                for (long i = 0; i < (long)rollout_items(L, l); ++i) {
                    const DynsolveItem d = dynsolve_item(L, K, adj, l, i);
                    printf("item %ld %d %d %ld %ld %ld %ld %d %d\n", K, adj, l, i, (long)d.node, (long)d.src, (long)d.dst, (int)d.live, (int)d.src_zero);
                    live += d.live;
                    prod += d.live && !d.src_zero;
                }
                printf("count %ld %d %d %ld %ld %ld %ld\n", K, adj, l, live, (long)dynsolve_live_items(L, K, adj, l), prod,
                       (long)dynsolve_product_items(L, K, adj, l));
            }
        }
    }
    printf("bytes %zu %zu\n", dynsolve_offset_bytes(256, 1999, 1), dynsolve_offset_bytes(256, 1999, 256));
    return 0;
}
"""


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("dynsolve_plan")
    src, exe = str(tmp / "plan.cpp"), str(tmp / "plan")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    rows = [l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    by = {}
    for r in rows:
        if r[0] != "bytes":
            by.setdefault((r[0], int(r[1]), int(r[2])), []).append(r[3:])
    by["bytes"] = [int(v) for v in [r for r in rows if r[0] == "bytes"][0][1:]]
    return by


def _plan(output, K, adj):
    """What the program printed for (K, direction), as integers."""
    L, matrices = (int(v) for v in output[("head", K, adj)][0])
    return dict(L=L, matrices=matrices,
                leaf=[tuple(int(v) for v in c.split(":")) for c in output[("leaf", K, adj)][0]],          # (position, knot of B or -1)
                start=tuple(int(v) for v in output[("start", K, adj)][0]),                               # (knot, from)
                up=[tuple(int(v) for v in r) for r in output.get(("up", K, adj), [])],                   # l, a, x, add, out
                items=[tuple(int(v) for v in r) for r in output[("item", K, adj)]],                      # l, i, node, src, dst, live, zero
                counts=[tuple(int(v) for v in r) for r in output[("count", K, adj)]])


def _orthogonal(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _matrix_tree(plan, E):
    """the rollout's product tree, carried out with dynsolve_up's positions for the forward direction (a = right child, x = left)"""
    n = E[0].shape[0]
    T = np.full((plan["matrices"], n, n), np.nan)
    for i, (pos, _knot) in enumerate(plan["leaf"]):
        T[pos] = E[i] if i < len(E) else np.eye(n)
    return T


def _scan(plan_fw, plan, E, B, adj):
    """Loader, up-sweep and descent from the printed indices.  Returns the knots and how often an item wrote each."""
    K, n = len(E), E[0].shape[0]
    T = _matrix_tree(plan_fw, E)
    for _l, a, x, _add, out in plan_fw["up"]:      # the matrix tree: level[l+1][s] = level[l][half+s] level[l][s]
        T[out] = T[a] @ T[x]
    assert not np.isnan(T).any()
    op = (lambda M: M.T) if adj else (lambda M: M)
    F = np.full((plan["matrices"], n), np.nan)
    assert sorted(p for p, _ in plan["leaf"]) == list(range(1 << plan["L"]))
    for pos, knot in plan["leaf"]:
        F[pos] = B[knot] if knot >= 0 else 0.0
    for _l, a, x, add, out in plan["up"]:
        assert not np.isnan(F[x]).any() and not np.isnan(F[add]).any() and np.isnan(F[out]).all()
        F[out] = op(T[a]) @ F[x] + F[add]
    assert not np.isnan(F).any()
    S = np.full((K + 1, n), np.nan)
    writes = np.zeros(K + 1, dtype=int)
    loaded, frm = plan["start"]
    if loaded >= 0:
        S[loaded] = B[frm]
    levels = []
    for l, _i, node, src, dst, live, zero in plan["items"]:      # printed level by level, top down
        levels.append(l)
        assert zero == (bool(adj) and src > K)
        if not live:
            assert dst > K
            continue
        assert 0 <= dst <= K and 0 <= node < plan["matrices"]
        if zero:
            S[dst] = F[node]
        else:
            assert not np.isnan(S[src]).any(), "an item reads a knot nobody wrote"
            S[dst] = op(T[node]) @ S[src] + F[node]
        writes[dst] += 1
    assert levels == sorted(levels, reverse=True)
    return S, writes, loaded


@pytest.mark.parametrize("K", KS)
def test_forward_scan_equals_the_recurrence(output, K):
    rng = np.random.default_rng(K)
    E = [_orthogonal(rng, 3) for _ in range(K)]
    B = rng.standard_normal((K + 1, 3))
    plan = _plan(output, K, 0)
    S, writes, loaded = _scan(plan, plan, E, B, 0)
    ref = [B[0]]
    for k in range(K):
        ref.append(E[k] @ ref[-1] + B[k + 1])
    err = float(np.max(np.abs(S - np.array(ref))))
    print("forward", K, err)
    assert err <= 1e-12
    assert loaded == 0 and writes[0] == 0 and np.array_equal(writes[1:], np.ones(K, dtype=int))   # one writer per knot 1 .. K


@pytest.mark.parametrize("K", KS)
def test_adjoint_scan_equals_the_recurrence(output, K):
    rng = np.random.default_rng(500 + K)
    E = [_orthogonal(rng, 3) for _ in range(K)]
    B = rng.standard_normal((K + 1, 3))
    plan = _plan(output, K, 1)
    S, writes, loaded = _scan(_plan(output, K, 0), plan, E, B, 1)
    ref = np.empty((K + 1, 3))
    ref[K] = B[K]
    for k in range(K - 1, -1, -1):
        ref[k] = E[k].T @ ref[k + 1] + B[k]
    err = float(np.max(np.abs(S - ref)))
    print("adjoint", K, err)
    assert err <= 1e-12
    assert np.array_equal(writes[:K], np.ones(K, dtype=int))       # one writer per knot 0 .. K - 1
    # knot K: an item's when an identity leaf follows it, the loader's when K = 2^L
    assert (writes[K], loaded) == ((0, K) if K == 1 << plan["L"] else (1, -1))
    node, src, dst = plan["items"][0][2:5]
    assert plan["items"][0][0] == plan["L"] + 1 and (node, src, dst) == (plan["matrices"] - 1, 1 << plan["L"], 0)   # FINAL: the root's item


@pytest.mark.parametrize("adj", [0, 1])
def test_item_counts_used_for_the_profile(output, adj):
    for K in KS:
        for _l, live, live_fn, prod, prod_fn in _plan(output, K, adj)["counts"]:
            assert live == live_fn and prod == prod_fn, (K, adj, _l)


def test_offset_tree_bytes(output):
    # 256 states x 2000 knots: 4095 blocks of [16][256] for one column (134 MB), of [256][256] for a full basis (2.15 GB)
    assert output["bytes"] == [4095 * 16 * 256 * 8, 4095 * 256 * 256 * 8]
