"""csrc/dto_rollout_plan.h from plain C++: a stand-alone program is compiled with g++ (address and undefined-behaviour sanitizers on)
against the header alone (no HIP, no engine header), run without a GPU, and prints for K = 1 .. 70 the leaf slots, the level offsets
and lengths and the descent items, and for PATH_KS what rollout_final_path fills.  The tree is then carried out in NumPy with those indices and nothing else, on random 5 x 5
matrices, and compared with the sequential product."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
KS = list(range(1, 71))
PATH_KS = list(range(1, 18)) + [31, 32, 33, 1023, 1024, 1025]   # every K in 1 .. 17, and 2^L, 2^L +- 1 for L = 5 and 10

PROGRAM = r"""
#include <cstdio>
#include "dto_rollout_plan.h"
using namespace dto;

int main() {
    for (long K = 1; K <= 70; ++K) {
        const int L = rollout_levels(K);
        printf("K %ld L %d matrices %ld\n", K, L, (long)rollout_tree_matrices(L));
        printf("leaf %ld", K);
        for (long i = 0; i < (1L << L); ++i) printf(" %ld", (long)rollout_leaf_slot(L, i));
        printf("\n");
        for (int l = 0; l <= L; ++l) printf("level %ld %d %ld %ld\n", K, l, (long)rollout_level_off(L, l), (long)rollout_level_len(L, l));
        for (int l = L + 1; l >= 1; --l)
            for (long i = 0; i < (long)rollout_items(L, l); ++i) {
                const RolloutItem it = rollout_item(L, K, l, i);
                printf("item %ld %d %ld %ld %ld %ld %d\n", K, l, i, (long)it.node, (long)it.start, (long)it.mid, (int)it.live);
            }
        // the items the final state alone needs, from knot K back to knot 0
        printf("chain %ld", K);
        for (long t = K; t > 0;) {
            int l; int64_t i;
            rollout_writer(L, t, l, i);
            printf(" %d:%ld", l, (long)i);
            t = (long)rollout_item(L, K, l, i).start;
        }
        printf("\n");
    }
    // rollout_final_path: the same items in launch order, as (level:index:start:mid)
    const long path_ks[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025};
    for (long K : path_ks) {
        const int L = rollout_levels(K);
        int lv[ROLLOUT_MAX_PATH];
        int64_t ix[ROLLOUT_MAX_PATH];
        const int cnt = rollout_final_path(L, K, lv, ix);
        printf("path %ld %d %d", K, L, cnt);
        for (int c = 0; c < cnt; ++c) {
            const RolloutItem it = rollout_item(L, K, lv[c], ix[c]);
            printf(" %d:%ld:%ld:%ld", lv[c], (long)ix[c], (long)it.start, (long)it.mid);
        }
        printf("\n");
    }
    printf("bytes %zu %zu %zu\n", rollout_tree_bytes(256, 1999), rollout_traj_bytes(256, 1999, 1), rollout_workspace_bytes(256, 15999, 256));
    printf("cols %d %d %d %d %d %d %d %d\n", rollout_col_pad(1), rollout_col_pad(16), rollout_col_pad(17), rollout_col_pad(48), rollout_col_pad(49),
           rollout_col_pad(256), rollout_col_tile(48), rollout_col_tile(49));
    return 0;
}
"""


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    tmp = tmp_path_factory.mktemp("rollout_plan")
    src, exe = str(tmp / "plan.cpp"), str(tmp / "plan")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, src, "-o", exe], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def _plan(output, K):
    """What the program printed for K, as integers."""
    rows = [l.split() for l in output]
    head = [r for r in rows if r[0] == "K" and int(r[1]) == K][0]
    plan = dict(L=int(head[3]), matrices=int(head[5]))
    plan["leaf"] = [int(v) for v in [r for r in rows if r[0] == "leaf" and int(r[1]) == K][0][2:]]
    plan["levels"] = {int(r[2]): (int(r[3]), int(r[4])) for r in rows if r[0] == "level" and int(r[1]) == K}
    plan["items"] = [tuple(int(v) for v in r[2:]) for r in rows if r[0] == "item" and int(r[1]) == K]   # l, i, node, start, mid, live
    plan["chain"] = [tuple(int(v) for v in c.split(":")) for c in [r for r in rows if r[0] == "chain" and int(r[1]) == K][0][2:]]
    return plan


def _carry_out(plan, E, x0):
    """The up-sweep and the descent as the engine runs them, from the printed indices alone.  Returns the states by knot and how
    often each knot was written."""
    L, K, n = plan["L"], len(E), E[0].shape[0]
    tree = np.full((plan["matrices"], n, n), np.nan)
    assert sorted(plan["leaf"]) == list(range(1 << L))          # a permutation of the level's slots
    for i, slot in enumerate(plan["leaf"]):
        tree[plan["levels"][0][0] + slot] = E[i] if i < K else np.eye(n)
    for l in range(L):
        (off, ln), (off1, ln1) = plan["levels"][l], plan["levels"][l + 1]
        assert ln == 2 * ln1 and off1 == off + ln
        for s in range(ln1):                                      # one contiguous batch: second half times first half
            tree[off1 + s] = tree[off + ln1 + s] @ tree[off + s]
    assert plan["levels"][L] == (plan["matrices"] - 1, 1) and not np.isnan(tree).any()
    S = np.full((K + 1, n), np.nan)
    S[0] = x0
    writes = np.zeros(K + 1, dtype=int)
    levels_seen = []
    for l, i, node, start, mid, live in plan["items"]:            # printed level by level, top down
        levels_seen.append(l)
        if not live:
            assert mid > K
            continue
        assert 1 <= mid <= K and 0 <= node < plan["matrices"]
        assert not np.isnan(S[start]).any(), "a state is read before the level that writes it"
        S[mid] = tree[node] @ S[start]
        writes[mid] += 1
    assert levels_seen == sorted(levels_seen, reverse=True)
    return S, writes, tree


@pytest.mark.parametrize("K", KS)
def test_tree_and_descent_equal_the_sequential_product(output, K):
    rng = np.random.default_rng(K)
    E = [rng.standard_normal((5, 5)) / np.sqrt(5.0) for _ in range(K)]
    x0 = rng.standard_normal(5)
    plan = _plan(output, K)
    assert (1 << plan["L"]) >= K and (plan["L"] == 0 or (1 << (plan["L"] - 1)) < K)
    assert plan["matrices"] == (2 << plan["L"]) - 1
    S, writes, _ = _carry_out(plan, E, x0)
    ref = [x0]
    for Ek in E:
        ref.append(Ek @ ref[-1])
    err = max(float(np.max(np.abs(S[k] - ref[k]))) for k in range(K + 1))
    print(K, plan["L"], err)
    assert err <= 1e-12
    # every knot 1 .. K has exactly one writer, no item beyond K is live
    assert np.array_equal(writes[1:], np.ones(K, dtype=int)) and writes[0] == 0
    assert all(mid <= K for (_l, _i, _node, _start, mid, live) in plan["items"] if live)
    assert all(live for (_l, _i, _node, _start, mid, live) in plan["items"] if mid <= K)


@pytest.mark.parametrize("K", KS)
def test_the_final_state_needs_only_its_chain_of_items(output, K):
    """Mode FINAL runs the items on the way from knot K back to knot 0: each is a live item of the full descent, the levels fall
    strictly from knot 0 outwards, and carrying out these alone gives knot K of the full descent bit for bit."""
    rng = np.random.default_rng(1000 + K)
    E = [rng.standard_normal((5, 5)) / np.sqrt(5.0) for _ in range(K)]
    x0 = rng.standard_normal(5)
    plan = _plan(output, K)
    S, _, tree = _carry_out(plan, E, x0)
    items = {(l, i): (node, start, mid, live) for l, i, node, start, mid, live in plan["items"]}
    chain = plan["chain"][::-1]                                   # highest level first, as the engine launches them
    assert 1 <= len(chain) <= plan["L"] + 1
    assert [l for l, _ in chain] == sorted({l for l, _ in chain}, reverse=True)
    F = {0: x0}
    for l, i in chain:
        node, start, mid, live = items[(l, i)]
        assert live and start in F
        F[mid] = tree[node] @ F[start]
    assert np.array_equal(F[K], S[K])


def _follow_start(K):
    """the items from knot K back to knot 0 as (level, index, start, mid), from the header's opening comment alone: knot
    t = 2^(l-1) (2 i + 1) is the midpoint of item (l, i), which starts at i 2^l; knot 2^L comes from the root's item (L + 1, 0)"""
    L = max(K - 1, 0).bit_length()
    items, t = [], K
    while t > 0:
        if t == 1 << L:
            l, i, start = L + 1, 0, 0
        else:
            l = (t & -t).bit_length()
            i = t >> l
            start = i << l
        items.append((l, i, start, t))
        t = start
    return L, items[::-1]


@pytest.mark.parametrize("K", PATH_KS)
def test_rollout_final_path_lists_the_chain_in_launch_order(output, K):
    row = [l.split() for l in output if l.startswith("path %d " % K)][0]
    L, cnt = int(row[2]), int(row[3])
    path = [tuple(int(v) for v in c.split(":")) for c in row[4:]]
    print(K, L, cnt, path)
    L_ref, ref = _follow_start(K)
    assert L == L_ref and cnt == len(path) and 1 <= cnt <= L + 1
    assert path == ref
    assert path[0][2] == 0 and path[-1][3] == K                   # the first item starts at knot 0, the last writes knot K
    assert all(a[3] == b[2] for a, b in zip(path, path[1:]))      # each reads what the one before wrote
    assert [l for l, *_ in path] == sorted({l for l, *_ in path}, reverse=True)   # highest level first, strictly falling


def test_rollout_final_path_is_the_chain_the_writers_give(output):
    """for the K the first program loop covers too: the reverse of the chain printed there"""
    for K in [k for k in PATH_KS if k in KS]:
        row = [l.split() for l in output if l.startswith("path %d " % K)][0]
        assert [tuple(int(v) for v in c.split(":")[:2]) for c in row[4:]] == _plan(output, K)["chain"][::-1]


def test_workspace_and_column_padding(output):
    b = [int(v) for v in [l for l in output if l.startswith("bytes ")][0].split()[1:]]
    # 256 states x 2000 knots: L = 11, 4095 matrices of 512 KiB; one column rounds up to a 16-column tile
    assert b[0] == 4095 * 256 * 256 * 8 and b[1] == 2000 * 16 * 256 * 8
    # 256 x 16000, a full basis: L = 14, 32767 matrices, and a trajectory as large as the caller's own output
    assert b[2] == 32767 * 256 * 256 * 8 + 16000 * 256 * 256 * 8
    assert [l for l in output if l.startswith("cols ")][0].split()[1:] == ["16", "16", "32", "48", "64", "256", "16", "64"]


def test_header_includes_only_the_standard_library():
    with open(os.path.join(CSRC, "dto_rollout_plan.h")) as f:
        includes = sorted(l.split()[1] for l in f if l.lstrip().startswith("#include"))
    assert includes == ["<cstddef>", "<cstdint>"], includes
