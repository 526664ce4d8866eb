"""CPU: the index plan of the solves with the dynamics block (dto_dynamics_solve, csrc/dto_rollout_plan.h) from plain C++.  A
stand-alone program is compiled with g++ (address and undefined-behaviour sanitizers on) against the header alone and prints, for
K = 1 .. 70 and both directions, the loader's leaves and start knot, the up-sweep's triples and the descent's items.  Both affine
scans are then carried out in NumPy with those indices and nothing else, on random orthogonal 3 x 3 E_k, and compared with the direct
recurrences  Y_{k+1} = E_k Y_k + B_{k+1}  and  Lam_k = E_k' Lam_{k+1} + B_k.  The program and the NumPy scans live in tests/scan_cases.py,
which the scan accuracy tests share."""
import numpy as np
import pytest

from scan_cases import plan_of as _plan, plan_output, scan as _scan   # the program and the restatement: one statement for every test

KS = list(range(1, 71))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    return plan_output(tmp_path_factory.mktemp("dynsolve_plan"), sanitize=True)


def _orthogonal(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


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
