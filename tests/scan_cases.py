"""The cases of the scan accuracy tests (tests/test_scan_hp_reference.py, tests/test_gpu_scan_accuracy_budget.py): the rollout
X_{k+1} = E_k X_k and the two solves with the dynamics block, Y_{k+1} = E_k Y_k + B_{k+1} and Lam_k = E_k' Lam_{k+1} + B_k, held to
the 320-bit references tests/hp_reference.py and tests/tdb_hp_reference.py.

Three things live here, so that every test uses one statement of each:

  * the NumPy restatement of the tree scan (`plans`, `matrix_tree`, `scan`, `restated`): loader, up-sweep and descent carried out
    with the indices that csrc/dto_rollout_plan.h prints and nothing else (tests/test_dynamics_solve_plan_header.py checks it
    against the recurrences for K = 1 .. 70); five defects can be built into it one at a time (`DEFECTS`);
  * the exact recurrences (`exact`): the three recurrences on given fp64 E_k in the fixed point of tests/hp_reference.py -- an
    fp64 number converts exactly, a product rounds at 2^-320, one rounding to fp64 at the end;
  * the 320-bit values of the TRUE propagators (`reference`): one `expm_action(A_k, .)` or `flow` per interval, sequentially.

The metric (`knot_errors`): per knot t and quantity, max|a - b| over the knot's block, divided by max|b| over the knots 0 .. t
(X, Y) or t .. K (Lam) -- a small knot of a decaying trajectory does not set its own scale.

Layer A (the scan alone, on the engine's own E_k): bar = 16 rho floored at hp_cases.BAR_NO_SQUARING, rho the worst error over the
knots of the restatement against `exact` on the same E_k; rho itself must stay under the a-priori bound `rho_bound`.
Layer B (end to end): bar at knot t = sum_i alpha(t, i) b_i + 16 rho (`layer_b_bars`), written into the fixture by its generator
beside the error of the sequential fp64 recurrence (`yard`), which must stay under hp_cases.ORACLE_CAP.  Nothing read from the
scan under test sets a bar.

Bilinear cases have seven knots (K = 6, L = 3: two identity leaves and dead items), time-dependent ones four (K = 3, L = 2)."""
import functools
import hashlib
import os
import shutil
import subprocess
import tempfile

import numpy as np
import scipy.linalg

import dto_oracle as O
import hp_cases as HC
import hp_reference as HP
import tdb_hp_reference as T
import tdbhp_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc")
GOLDEN = HC.GOLDEN
BAR_FACTOR = TC.BAR_FACTOR          # 16: MFMA sums four k per step in another order than NumPy -- a small multiple
FLOOR = HC.BAR_NO_SQUARING          # 64 2^-53
OLD_BAR = 1e-10                     # what tests/test_gpu_rollout.py and tests/test_gpu_dynamics_solve.py hold (K <= 16)
QUANTITIES = ("X", "Y", "Lam")
N_COLS = 3
DAMPING = 0.15                      # hp_damped: D = diag(0 .. DAMPING ||G_0||_2)

# `wide`: column counts layer A (and, on its first three columns, layer B) runs besides 3; `bits`: column counts whose columns
# 0, 48 and n - 1 must have the bits of their runs alone
CASES = {
    "hp_small": dict(kind="hp"),                                   # leaves from k_small, tree products on npad 64
    "hp_s64": dict(kind="hp"),                                     # leaves from k_chain64
    "hp_general": dict(kind="hp", wide=(66,)),                     # npad 128, two 64-column tiles (columns 64, 65 in the second)
    "hp_kron": dict(kind="hp"),                                    # structured leaves
    "hp_tile192": dict(kind="hp", wide=(49,)),                     # npad 192; 49: the first count on the wide tile
    "hp_ring256": dict(kind="hp", bits=(49, 250)),                 # ring-kernel tree, 6 dead rows
    "hp_ring384": dict(kind="hp", bits=(49, 330)),                 # ring kernel's 3 x 3 walk, 54 dead rows, six row tiles
    "hp_damped": dict(kind="damped", n=40, m=2, seed=909, ladder_of="hp_s64"),   # S - D: contractive, states decay
    "tdbhp_n4": dict(kind="tdb"),                                  # k_tdb, not skew, ||dt G|| up to 3
    "tdbhp_n16_o0": dict(kind="tdb"),
    "tdbhp_n72": dict(kind="tdb", group=True),                     # integrator 1 of the group of two: pre, x_off != 0
    "tdbhp_n128": dict(kind="tdb"),                                # k_tdb_mfma's 64-row tile
    "tdbhp_kron": dict(kind="tdb"),                                # k_tdb_kron
}
REGENERATED = ("hp_small", "hp_s64", "hp_kron", "hp_damped", "tdbhp_n4", "tdbhp_n16_o0", "tdbhp_kron")   # the others: by hash


def fixture_name(case):
    head, tail = case.split("_", 1)
    return f"{head}_scan_{tail}"


def load(case):
    with np.load(os.path.join(GOLDEN, fixture_name(case) + ".npz")) as f:
        return {k: f[k] for k in f.files}


def engine_kw(case):
    return dict(HC.ENGINE_KW.get(case, {}), **TC.ENGINE_KW.get(case, {}))


# ---- the index plan and the restatement of both scans ----------------------------------------------------------------------------

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


def plan_output(tmp, sanitize):
    """What the stand-alone program prints, compiled with g++ in the directory `tmp` against the header alone (`sanitize`: address
    and undefined-behaviour sanitizers on), keyed by (record, K, direction)."""
    assert shutil.which("g++") is not None, "g++ is needed (the engine's own build needs a C++ compiler too)"
    src, exe = os.path.join(str(tmp), "plan.cpp"), os.path.join(str(tmp), "plan")
    with open(src, "w") as f:
        f.write(PROGRAM)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + ["-I", CSRC, src, "-o", exe], check=True)
    rows = [l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    by = {}
    for r in rows:
        if r[0] != "bytes":
            by.setdefault((r[0], int(r[1]), int(r[2])), []).append(r[3:])
    by["bytes"] = [int(v) for v in [r for r in rows if r[0] == "bytes"][0][1:]]
    return by


def plan_of(output, K, adj):
    """What the program printed for (K, direction), as integers."""
    L, matrices = (int(v) for v in output[("head", K, adj)][0])
    return dict(L=L, matrices=matrices,
                leaf=[tuple(int(v) for v in c.split(":")) for c in output[("leaf", K, adj)][0]],          # (position, knot of B or -1)
                start=tuple(int(v) for v in output[("start", K, adj)][0]),                               # (knot, from)
                up=[tuple(int(v) for v in r) for r in output.get(("up", K, adj), [])],                   # l, a, x, add, out
                items=[tuple(int(v) for v in r) for r in output[("item", K, adj)]],                      # l, i, node, src, dst, live, zero
                counts=[tuple(int(v) for v in r) for r in output[("count", K, adj)]])


@functools.lru_cache(maxsize=None)
def _plain_output():
    with tempfile.TemporaryDirectory() as tmp:
        return plan_output(tmp, sanitize=False)


def plans(K):
    """(forward plan, adjoint plan) of K intervals, from a plain build of the program (the sanitized one is the header test's)."""
    return plan_of(_plain_output(), K, 0), plan_of(_plain_output(), K, 1)


DEFECTS = ("node", "leaf32", "left_offset", "addend_first", "leaf_beyond")


def _affine(M, v, add, defect):
    """M v + add; with the defect "addend_first" the addend joins the product's first k block instead of the finished sum -- the
    same value in exact arithmetic, other roundings."""
    if defect == "addend_first" and M.shape[1] > 4:
        return (M[:, :4] @ v[:4] + add) + M[:, 4:] @ v[4:]
    return M @ v + add


def matrix_tree(plan, E, defect=None, leaf=0):
    """The rollout's product tree before its products: the leaves at dynsolve's positions, identities beyond K.  Defects:
    "leaf32" rounds leaf `leaf` to fp32 and back, "leaf_beyond" puts the last E_k where an identity belongs."""
    n = E[0].shape[0]
    T_ = np.full((plan["matrices"], n, n), np.nan)
    for i, (pos, _knot) in enumerate(plan["leaf"]):
        T_[pos] = E[i] if i < len(E) else (E[-1] if defect == "leaf_beyond" else np.eye(n))
        if defect == "leaf32" and i == leaf:
            T_[pos] = T_[pos].astype(np.float32).astype(np.float64)
    return T_


def tree_products(plan_fw, T_, defect=None):
    """The matrix tree, with dynsolve_up's positions for the forward direction: level[l+1][s] = level[l][half+s] level[l][s]
    (a = right child, x = left).  Defect "node": the first level-1 node times 1 + 1e-11."""
    first = True
    for l, a, x, _add, out in plan_fw["up"]:
        T_[out] = T_[a] @ T_[x]
        if defect == "node" and l == 0 and first:
            T_[out] = T_[out] * (1.0 + 1e-11)
            first = False
    return T_


def scan(plan_fw, plan, E, B, adj, defect=None, leaf=0):
    """Loader, up-sweep and descent from the printed indices.  E: K matrices (n, n); B: (K + 1, n) or (K + 1, n, c).  Returns the
    knots, how often an item wrote each, and the knot the loader wrote.  Defect "left_offset": the adjoint's first up-sweep triple
    multiplies the offset of the left child where the right one belongs."""
    K, n = len(E), E[0].shape[0]
    T_ = tree_products(plan_fw, matrix_tree(plan_fw, E, defect, leaf), defect)
    assert not np.isnan(T_).any()
    op = (lambda M: M.T) if adj else (lambda M: M)
    tail = B.shape[1:]
    F = np.full((plan["matrices"],) + tail, np.nan)
    assert sorted(p for p, _ in plan["leaf"]) == list(range(1 << plan["L"]))
    for pos, knot in plan["leaf"]:
        F[pos] = B[knot] if knot >= 0 else 0.0
    for i, (_l, a, x, add, out) in enumerate(plan["up"]):
        assert not np.isnan(F[x]).any() and not np.isnan(F[add]).any() and np.isnan(F[out]).all()
        src = add if (defect == "left_offset" and adj and i == 0) else x
        F[out] = _affine(op(T_[a]), F[src], F[add], defect)
    assert not np.isnan(F).any()
    S = np.full((K + 1,) + tail, np.nan)
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
            S[dst] = _affine(op(T_[node]), S[src], F[node], defect)
        writes[dst] += 1
    assert levels == sorted(levels, reverse=True)
    return S, writes, loaded


def _cols(A):
    """(N, c, n) rows as the engine takes them -> (N, n, c) columns, and back."""
    return np.ascontiguousarray(np.swapaxes(A, -1, -2))


def restated(E, X0, B, defect=None, leaf=0):
    """{"X", "Y", "Lam"}: (N, c, n) each, the fp64 restatement of the tree scans on the propagators E (K, n, n).  The rollout is
    the forward scan of [X0; 0; ...]."""
    K = len(E)
    fw, ad = plans(K)
    B0 = np.zeros((K + 1,) + X0.shape)
    B0[0] = X0
    out = {}
    for key, rhs, plan, adj in (("X", B0, fw, 0), ("Y", B, fw, 0), ("Lam", B, ad, 1)):
        out[key] = _cols(scan(fw, plan, list(E), _cols(rhs), adj, defect, leaf)[0])
    return out


# ---- exact arithmetic on given fp64 propagators ----------------------------------------------------------------------------------


def exact(E, X0, B):
    """The three recurrences on the fp64 matrices E (K, n, n) in fixed point, rounded to fp64 once at the end: (N, c, n) each."""
    K = len(E)
    Ef = [HP.fx(Ek) for Ek in E]
    Bf = [HP.fx(b.T) for b in B]
    X, Y = [HP.fx(X0.T)], [Bf[0]]
    for k in range(K):
        X.append(HP.mul(Ef[k], X[-1]))
        Y.append(HP.mul(Ef[k], Y[-1]) + Bf[k + 1])
    Lam = [None] * K + [Bf[K]]
    for k in range(K - 1, -1, -1):
        Lam[k] = HP.mul(Ef[k].T, Lam[k + 1]) + Bf[k]
    return {key: np.stack([HP.to_float(v).T for v in seq]) for key, seq in (("X", X), ("Y", Y), ("Lam", Lam))}


# ---- the metric ------------------------------------------------------------------------------------------------------------------


def scales(b, adjoint):
    """max|b| over the knots 0 .. t, or t .. K for the adjoint: (N,)."""
    m = np.abs(b).reshape(b.shape[0], -1).max(axis=1)
    return np.maximum.accumulate(m[::-1])[::-1] if adjoint else np.maximum.accumulate(m)


def knot_errors(a, b, adjoint):
    """(N,): per knot, max|a - b| over the block / the running max|b| (NaN in `a` gives inf: a missing writer must not pass)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    d = np.abs(a - b).reshape(b.shape[0], -1)
    out = d.max(axis=1) / scales(b, adjoint)
    out[~np.all(np.isfinite(d), axis=1)] = np.inf
    return out


def errors(got, ref):
    """{quantity: (N,)} of the dicts `got` and `ref` over the quantities of `got`."""
    return {q: knot_errors(got[q], ref[q], q == "Lam") for q in QUANTITIES if q in got}


def rho(E, X0, B, ex=None):
    """{quantity: worst error over the knots} of the restatement against the exact values on the same E."""
    ex = exact(E, X0, B) if ex is None else ex
    return {q: float(v.max()) for q, v in errors(restated(E, X0, B), ex).items()}


def bar_a(r):
    return max(BAR_FACTOR * r, FLOOR)


def kappa(E):
    """The largest product of node 2-norms along any root-to-knot path of the descent, forward and adjoint (a node and its
    transpose have one norm), in fp64 from E."""
    K = len(E)
    fw, ad = plans(K)
    T_ = tree_products(fw, matrix_tree(fw, list(E)))
    norm = [np.linalg.norm(M, 2) for M in T_]
    worst = 1.0
    for plan in (fw, ad):
        path = {plan["start"][0]: 1.0} if plan["start"][0] >= 0 else {}
        for _l, _i, node, src, dst, live, zero in plan["items"]:
            if live:
                path[dst] = norm[node] * (1.0 if zero else path[src])
                worst = max(worst, path[dst])
    return worst


def rho_bound(E):
    """(2 L + 1) n 2^-53 kappa: L products of the tree, L affine steps of the up-sweep or descent and the final one, each a dot
    product of length n."""
    L = plans(len(E))[0]["L"]
    return (2 * L + 1) * E[0].shape[0] * 2.0 ** -53 * kappa(E)


# ---- the cases' problems, points and fp64 propagators ----------------------------------------------------------------------------


def _damped_problem(case):
    """hp_s64's kind of problem at the case's own seed with the drift G_0 = S_0 - D, D = diag(0 .. DAMPING ||S_0||_2)."""
    c = CASES[case]
    p = O.make_scaled_problem(HC.N_KNOTS, c["n"], c["m"], seed=c["seed"], skew=True)
    p.integrators = p.integrators[:1]
    it = p.integrators[0]
    G = np.array(it.G)
    G[0] = G[0] - np.diag(np.linspace(0.0, DAMPING * np.linalg.norm(G[0], 2), c["n"]))
    it.G = G
    return p


def problem(case):
    """The one-member oracle problem of the case at its seed's point (the ladder not yet set for the bilinear kinds)."""
    kind = CASES[case]["kind"]
    if kind == "hp":
        return HC.problem(case)
    if kind == "damped":
        return _damped_problem(case)
    return TC.problem(case)


def seed_of(case):
    c = CASES[case]
    return c["seed"] if "seed" in c else (HC.CASES[case]["seed"] if c["kind"] == "hp" else TC.CASES[case]["seed"])


def _damped_Z(case):
    p = problem(case)
    it = p.integrators[0]
    Zk = p.Z0.reshape(p.N, p.z).copy()
    rungs = HC.CASES[CASES[case]["ladder_of"]].get("ladder", HC.LADDER)
    perm = np.random.default_rng(CASES[case]["seed"] + 7).permutation(len(rungs))
    for k in range(p.K):
        u = Zk[k, it.u_off:it.u_off + it.u_dim]
        Zk[k, p.dt_idx] = rungs[perm[k]] / np.linalg.norm(it.G[0] + np.tensordot(u, it.G[1:], axes=(0, 0)), 2)
    return Zk.reshape(-1).copy()


def base_inputs(case):
    """(Z, input hash) of the fixture the case extends; hp_damped: its own point and the hash of that."""
    kind = CASES[case]["kind"]
    if kind == "damped":
        Z = _damped_Z(case)
        return Z, hashlib.sha256(Z.tobytes()).hexdigest()
    C = HC if kind == "hp" else TC
    d = C.inputs(case)
    return d["Z"], C.input_hash(d)


def at_point(case, Z):
    p = problem(case)
    p.Z0 = np.asarray(Z, dtype=np.float64).copy()
    return p


def columns(case, N):
    """(X0 (3, n), B (N, 3, n)) from the case's seed + 41."""
    n = problem(case).integrators[0].x_dim
    rng = np.random.default_rng(seed_of(case) + 41)
    return rng.standard_normal((N_COLS, n)), rng.standard_normal((N, N_COLS, n))


def more_columns(case, n_cols, X0, B):
    """X0 and B widened to n_cols columns: the fixture's three first, the rest from the case's seed + 43."""
    rng = np.random.default_rng(seed_of(case) + 43)
    n, N = X0.shape[1], B.shape[0]
    return (np.concatenate([X0, rng.standard_normal((n_cols - N_COLS, n))], axis=0),
            np.concatenate([B, rng.standard_normal((N, n_cols - N_COLS, n))], axis=1))


def oracle_propagators(p):
    """(K, n, n) fp64: scipy.linalg.expm of A_k for a bilinear integrator, the oracle's fixed-step map on the basis columns for
    the time-dependent kind."""
    it = p.integrators[0]
    n, z, N = it.x_dim, p.z, p.N
    Zk = p.Z0.reshape(N, z)
    E = np.empty((N - 1, n, n))
    for k in range(N - 1):
        if isinstance(it, O.TimeDependentBilinearIntegrator):
            zz = np.tile(np.concatenate([Zk[k], Zk[k + 1]]), (n, 1))
            zz[:, it.x_off:it.x_off + n] = np.eye(n)
            zz[:, z + it.x_off:z + it.x_off + n] = 0.0
            E[k] = (-it.f(zz)).T              # row c of the map's output is E_k e_c
        else:
            G = np.asarray(it.G)
            E[k] = scipy.linalg.expm(Zk[k, p.dt_idx] * (G[0] + np.einsum("j,jrc->rc", Zk[k, it.u_off:it.u_off + it.u_dim], G[1:])))
    return E


def sequential(E, X0, B):
    """The three recurrences in fp64, one step after the other: (N, c, n) each."""
    K = len(E)
    X, Y, Lam = np.empty_like(B), np.empty_like(B), np.empty_like(B)
    X[0], Y[0], Lam[K] = X0, B[0], B[K]
    for k in range(K):
        X[k + 1] = X[k] @ E[k].T
        Y[k + 1] = Y[k] @ E[k].T + B[k + 1]
    for k in range(K - 1, -1, -1):
        Lam[k] = Lam[k + 1] @ E[k] + B[k]
    return dict(X=X, Y=Y, Lam=Lam)


# ---- 320-bit values of the true propagators --------------------------------------------------------------------------------------


def _hp_actions(case, p):
    """[(forward action, transposed action)] per interval of a bilinear case: fixed-point (n, c) columns in and out.  A family of
    blocks I_r (x) G acts on the (b, r c) columns of its segments; fx(G) is formed once."""
    it = p.integrators[0]
    n, m = it.x_dim, it.u_dim
    if CASES[case]["kind"] == "hp":
        G, r = HC._block(case, p)
    else:
        G, r = np.asarray(it.G), 1
    b = n // r
    Gf = HP.fx(G)
    Zk = p.Z0.reshape(p.N, p.z)
    seg = lambda V: V.reshape(r, b, -1).transpose(1, 0, 2).reshape(b, -1)          # (n, c) -> (b, r c)
    unseg = lambda W, c: W.reshape(b, r, c).transpose(1, 0, 2).reshape(n, c)
    out = []
    for k in range(p.K):
        Gu = Gf[0] + 0
        for j in range(m):
            Gu = Gu + HP.scale(int(HP.fx(Zk[k, it.u_off + j])), Gf[1 + j])
        A = HP.scale(int(HP.fx(Zk[k, p.dt_idx])), Gu)
        At = A.T.copy()
        out.append((lambda V, A=A: unseg(HP.expm_action(A, seg(V)), V.shape[1]), lambda V, At=At: unseg(HP.expm_action(At, seg(V)), V.shape[1])))
    return out


def tdb_interval_args(p, k):
    it = p.integrators[0]
    Zk = p.Z0.reshape(p.N, p.z)
    m = it.u_dim
    return (T.fx(Zk[k, it.u_off:it.u_off + m]), T.fx(Zk[k + 1, it.u_off:it.u_off + m]), int(T.fx(Zk[k, it.t_off])), int(T.fx(Zk[k, p.dt_idx])))


def transposed_family(fam):
    """The family whose `flow`, run backwards in time, is Phi': every matrix transposed and negated (below)."""
    Bs, kinds, omegas = fam
    return [-np.transpose(Bc, (0, 2, 1)) for Bc in Bs], kinds, omegas


def flow_transposed(fam_t, order, S, uk, uk1, tk, dt, Y):
    """Phi' Y from `flow` alone.  Phi is a product of S step matrices P_i = P(M1, M2, M4) of non-commuting stages, so `flow` on the
    transposed family at the same times is NOT Phi'.  But P(M1, M2, M4)' = P(M4', M2', M1') term by term (the h^2 term
    M2 M1 + M2 M2 + M4 M2 transposes into M1' M2' + M2' M2' + M2' M4', and so on up to h^4), and Phi' = P_1' ... P_S' applies the last
    step first: the scheme run from t_k + dt_k back to t_k with step -dt_k, controls interpolated from u_{k+1} to u_k.  `flow`
    multiplies the family by dt, so the transposed family is negated as well (`transposed_family`): (-dt)(-G') = dt G'."""
    return T.flow(fam_t, order, S, uk1 if order == 1 else uk, uk, tk + dt, -dt, Y)


def _tdb_actions(p):
    it = p.integrators[0]
    fam = T.family(it.G, it.mods)
    fam_t = transposed_family(fam)
    out = []
    for k in range(p.K):
        a = tdb_interval_args(p, k)
        out.append((lambda V, a=a: T.flow(fam, it.spline_order, it.substeps, *a, V),
                    lambda V, a=a: flow_transposed(fam_t, it.spline_order, it.substeps, *a, V)))
    return out


def reference(case, p, X0, B):
    """The 320-bit X, Y and Lam (N, c, n), rounded to fp64 once; sequentially, X and Y as columns of one call per interval.  Also
    `fwd_in` / `adj_in`: per interval the fixed-point columns the action took and gave, for a yardstick of the action alone."""
    acts = _hp_actions(case, p) if CASES[case]["kind"] != "tdb" else _tdb_actions(p)
    K, c = p.K, X0.shape[0]
    Bf = [HP.fx(b.T) for b in B]
    XY = [np.concatenate([HP.fx(X0.T), Bf[0]], axis=1)]
    steps_f, steps_a = [], [None] * K
    for k in range(K):
        out = acts[k][0](XY[-1])
        steps_f.append((HP.to_float(XY[-1]), HP.to_float(out)))
        out[:, c:] = out[:, c:] + Bf[k + 1]
        XY.append(out)
    Lam = [None] * K + [Bf[K]]
    for k in range(K - 1, -1, -1):
        out = acts[k][1](Lam[k + 1])
        steps_a[k] = (HP.to_float(Lam[k + 1]), HP.to_float(out))
        Lam[k] = out + Bf[k]
    XYf = np.stack([HP.to_float(v).T for v in XY])
    return dict(X=XYf[:, :c], Y=XYf[:, c:], Lam=np.stack([HP.to_float(v).T for v in Lam])), steps_f, steps_a


# ---- layer B's bars --------------------------------------------------------------------------------------------------------------


def interval_bars(case, E, steps_f, steps_a):
    """(b forward (K,), b adjoint (K,)): the bar the action of E_i is held to at interval i.  hp_*: BAR_NO_SQUARING on the rung
    inside the chain's radius, BAR elsewhere.  tdbhp_*: the stored bars of the fixture's classes "defect" and "JTw".  hp_damped
    (no callback fixture, no budget claimed for non-skew generators): 16 x the error of the fp64 E_i on the reference's own
    columns against the 320-bit action, floored -- the yardstick of the action alone."""
    kind = CASES[case]["kind"]
    K = len(E)
    if kind == "hp":
        norm2 = HC.load(case)["norm2"]
        b = np.where(np.abs(norm2 - 0.5) < 1e-9, HC.BAR_NO_SQUARING, HC.BAR)
        return b, b.copy()
    if kind == "tdb":
        fix = TC.load(case)
        return np.full(K, TC.bar_for(fix, "defect")), np.full(K, TC.bar_for(fix, "JTw"))
    bf = np.array([max(BAR_FACTOR * HC.nerr(E[i] @ steps_f[i][0], steps_f[i][1]), FLOOR) for i in range(K)])
    ba = np.array([max(BAR_FACTOR * HC.nerr(E[i].T @ steps_a[i][0], steps_a[i][1]), FLOOR) for i in range(K)])
    return bf, ba


def layer_b_bars(E, ref, b_fwd, b_adj, rho_):
    """(3, N): the bar of each quantity at each knot, sum_i alpha(t, i) b_i + 16 rho floored at FLOOR, with
    alpha(t, i) = ||E_{t-1} ... E_{i+1}||_2 max|s_i| / scale_t for the knots i < t that feed a forward quantity (s_i the reference's
    state at knot i), and ||E_{i-1} ... E_t||_2 max|lam_{i+1}| / scale_t over i >= t for the adjoint, from fp64 products of E."""
    K = len(E)
    n = E[0].shape[0]
    bars = np.zeros((3, K + 1))
    for qi, q in enumerate(QUANTITIES):
        adj = q == "Lam"
        s = ref[q]
        size = np.abs(s).reshape(K + 1, -1).max(axis=1)
        scale = scales(s, adj)
        for t in range(K + 1):
            total = 0.0
            if not adj:
                P = np.eye(n)
                for i in range(t - 1, -1, -1):           # P = E_{t-1} ... E_{i+1}
                    total += np.linalg.norm(P, 2) * size[i] / scale[t] * b_fwd[i]
                    P = P @ E[i]
            else:
                P = np.eye(n)
                for i in range(t, K):                    # P = E_{i-1} ... E_t
                    total += np.linalg.norm(P, 2) * size[i + 1] / scale[t] * b_adj[i]
                    P = E[i] @ P
            bars[qi, t] = total + bar_a(rho_[q])
    return bars


def build_fixture(case):
    """The scan fixture's arrays: the hash of the inputs it extends (hp_damped: its own Z too), X0, B, the 320-bit X, Y, Lam, and
    beside them the sequential fp64 recurrence's error (`yard`), rho of the restatement on the oracle's E_k, the interval bars and
    layer B's bars."""
    Z, h = base_inputs(case)
    p = at_point(case, Z)
    X0, B = columns(case, p.N)
    ref, steps_f, steps_a = reference(case, p, X0, B)
    E = oracle_propagators(p)
    yard = errors(sequential(E, X0, B), ref)
    r = rho(E, X0, B)
    b_fwd, b_adj = interval_bars(case, E, steps_f, steps_a)
    out = dict(input_hash=np.array(h), X0=X0, B=B, X=ref["X"], Y=ref["Y"], Lam=ref["Lam"],
               yard=np.stack([yard[q] for q in QUANTITIES]), rho=np.array([r[q] for q in QUANTITIES]), rho_bound=np.array(rho_bound(E)),
               b_fwd=b_fwd, b_adj=b_adj, bars=layer_b_bars(E, ref, b_fwd, b_adj, r))
    if CASES[case]["kind"] == "damped":
        out["Z"] = Z
    return out


def point_of(case, fix=None):
    """(one-member oracle problem at the fixture's point, Z): the point of the fixture the case extends, checked by its hash."""
    fix = load(case) if fix is None else fix
    kind = CASES[case]["kind"]
    if kind == "damped":
        Z = fix["Z"]
        assert hashlib.sha256(np.ascontiguousarray(Z).tobytes()).hexdigest() == str(fix["input_hash"])
    else:
        base = (HC if kind == "hp" else TC).load(case)
        assert str(base["input_hash"]) == str(fix["input_hash"]), case
        Z = base["Z"]
    return at_point(case, Z), Z


def report(case, what, errs, bars, extra=""):
    """One line per quantity: the error at every knot beside its bar."""
    lines = [f"{case} {what} {extra}"]
    for q in errs:
        b = np.broadcast_to(np.asarray(bars[q], dtype=np.float64), errs[q].shape)
        lines.append(f"  {q:3s} " + " ".join(f"{e:.1e}/{bb:.1e}" for e, bb in zip(errs[q], b)) +
                     f"   worst ratio {float(np.max(errs[q] / b)):.3f}")
    return "\n".join(lines)
