"""Shared by the tests of the whole-dynamics solves (dto_dynamics_solve_all, csrc/dto_elim.hip, csrc/dto_elim_plan.h): a NumPy
restatement of the plan and of the block elimination, the dense block MM assembled from the ORACLE's Jacobian, and the cases.

MM (N D x N D, D = the sum of the integrators' state dimensions): per integrator an identity row block for knot 1 and below it its
defect rows of the N - 1 intervals, restricted to the state columns of every integrator at every knot.  Row and column index
k D + pre_i + r for knot k (0-based), integrator i, component r.  Right-hand sides and results are (N, n_cols, D).

`eliminate` is the algorithm the engine runs, stated on the dense Jacobian: levels ascending (adjoint: descending), the coupling
blocks of both knots of an interval, then the integrator's own block by its recurrence.  Its `defect` argument breaks it in one named
way at a time, for the tests that show the bar can fail."""
import functools

import numpy as np

import dto_amd
import dto_oracle as O
from helpers import to_engine
from multi_ket_cases import multi_ket, to_oracle
from test_gpu_block_generators import kron_problem


# ------------------------------------------------------------------------------------------------------------- the plan
def describe(prob):
    """per integrator of an oracle problem: kind, states, inputs, time component (-1: none)"""
    out = []
    for it in prob.integrators:
        if isinstance(it, O.TimeDependentBilinearIntegrator):
            out.append(dict(kind="time_dependent", x_off=it.x_off, x_dim=it.x_dim, in_off=it.u_off, in_dim=it.u_dim, t_off=it.t_off))
        elif it.kind == "bilinear":
            out.append(dict(kind="bilinear", x_off=it.x_off, x_dim=it.x_dim, in_off=it.u_off, in_dim=it.u_dim, t_off=-1))
        else:
            out.append(dict(kind="derivative", x_off=it.x_off, x_dim=it.x_dim, in_off=it.xdot_off, in_dim=it.x_dim, t_off=-1))
    return out


def _meets(lo, ln, lo2, ln2):
    return ln > 0 and ln2 > 0 and lo < lo2 + ln2 and lo2 < lo + ln


def _reads(a, dt_idx, x_off, x_dim):
    return (_meets(a["in_off"], a["in_dim"], x_off, x_dim) or _meets(dt_idx, 1, x_off, x_dim)
            or (a["kind"] == "time_dependent" and _meets(a["t_off"], 1, x_off, x_dim)))


def plan(its, dt_idx, K):
    """levels, processing order, dependencies with their column offsets, dependents, widths and the coupling store's offsets"""
    n = len(its)
    pre = [sum(i["x_dim"] for i in its[:a]) for a in range(n)]
    p = dict(refusal=None, n_states=sum(i["x_dim"] for i in its), pre=pre)
    for a in range(n):
        for b in range(a + 1, n):
            if _meets(its[a]["x_off"], its[a]["x_dim"], its[b]["x_off"], its[b]["x_dim"]):
                return dict(p, refusal=f"the states of integrators {a} and {b} overlap")
    for a in range(n):
        if _reads(its[a], dt_idx, its[a]["x_off"], its[a]["x_dim"]):
            return dict(p, refusal=f"the inputs of integrator {a} meet its own states")
    deps, dependents, width = [[] for _ in its], [[] for _ in its], [0] * n
    for a in range(n):
        for b in range(n):
            if b != a and _reads(its[a], dt_idx, its[b]["x_off"], its[b]["x_dim"]):
                deps[a].append((b, width[a]))
                width[a] += its[b]["x_dim"]
                dependents[b].append(a)
    level = [0] * n
    for rounds in range(n + 2):
        changed = False
        for a in range(n):
            for b, _ in deps[a]:
                if level[a] < level[b] + 1:
                    level[a], changed = level[b] + 1, True
        if not changed:
            break
        if rounds > n:
            return dict(p, refusal="the integrators depend on each other in a cycle")
    order = sorted(range(n), key=lambda a: (level[a], a))
    store = [0]
    for a in range(n):
        store.append(store[-1] + K * 2 * width[a] * its[a]["x_dim"])
    return dict(p, level=level, n_levels=max(level) + 1 if n else 0, order=order, deps=deps, dependents=dependents, width=width, store_off=store)


# --------------------------------------------------------------------------------------------- the oracle's block and the algorithm
def dense_jacobian(prob, Z=None):
    """the dynamics rows of the oracle's Jacobian, dense: (K D, n_vars)"""
    Z = prob.Z0 if Z is None else Z
    return np.vstack([O.integrator_jacobian(it, prob, Z).toarray() for it in prob.integrators])


def _rows(prob, its, pre, a, k):
    return (prob.N - 1) * pre[a] + k * its[a]["x_dim"] + np.arange(its[a]["x_dim"])


def _cols(prob, its, b, k):
    return k * prob.z + its[b]["x_off"] + np.arange(its[b]["x_dim"])


def assemble(Jd, prob):
    its = describe(prob)
    N, K, D = prob.N, prob.N - 1, sum(i["x_dim"] for i in its)
    pre = [sum(i["x_dim"] for i in its[:a]) for a in range(len(its))]
    M = np.zeros((N * D, N * D))
    M[:D, :D] = np.eye(D)
    for a in range(len(its)):
        for k in range(K):
            r = (k + 1) * D + pre[a] + np.arange(its[a]["x_dim"])
            for b in range(len(its)):
                for kn in (k, k + 1):
                    c = kn * D + pre[b] + np.arange(its[b]["x_dim"])
                    M[np.ix_(r, c)] = Jd[np.ix_(_rows(prob, its, pre, a, k), _cols(prob, its, b, kn))]
    return M


def dense_solve(M, B, adjoint):
    N, nc, D = B.shape
    rhs = B.transpose(0, 2, 1).reshape(N * D, nc)
    return np.linalg.solve(M.T if adjoint else M, rhs).reshape(N, D, nc).transpose(0, 2, 1)


def eliminate(Jd, prob, B, adjoint, defect=None):
    """defect: None, "drop_next_half" (the k + 1 half of the coupling blocks), "list_order" (list order instead of levels),
    "adjoint_reads_deps" (the adjoint subtracts over dependencies instead of dependents)"""
    its = describe(prob)
    p = plan(its, prob.dt_idx, prob.N - 1)
    assert p["refusal"] is None, p["refusal"]
    pre, K = p["pre"], prob.N - 1
    sl = [slice(pre[a], pre[a] + its[a]["x_dim"]) for a in range(len(its))]
    order = list(range(len(its))) if defect == "list_order" else list(p["order"])
    Y = np.zeros_like(B)
    for a in (order[::-1] if adjoint else order):
        E = [-Jd[np.ix_(_rows(prob, its, pre, a, k), _cols(prob, its, a, k))] for k in range(K)]
        Bp = B[:, :, sl[a]].copy()
        if not adjoint:
            for k in range(K):
                acc = np.zeros_like(Bp[k + 1])
                for half in (0, 1):
                    if half == 1 and defect == "drop_next_half":
                        continue
                    for b, _ in p["deps"][a]:
                        acc += Y[k + half][:, sl[b]] @ Jd[np.ix_(_rows(prob, its, pre, a, k), _cols(prob, its, b, k + half))].T
                Bp[k + 1] -= acc
            Ya = np.empty_like(Bp)
            Ya[0] = Bp[0]
            for k in range(K):
                Ya[k + 1] = Ya[k] @ E[k].T + Bp[k + 1]
        else:
            users = [b for b, _ in p["deps"][a]] if defect == "adjoint_reads_deps" else p["dependents"][a]
            for k in range(K + 1):
                acc = np.zeros_like(Bp[k])
                for b in users:
                    if k >= 1 and defect != "drop_next_half":
                        acc += Y[k][:, sl[b]] @ Jd[np.ix_(_rows(prob, its, pre, b, k - 1), _cols(prob, its, a, k))]
                    if k < K:
                        acc += Y[k + 1][:, sl[b]] @ Jd[np.ix_(_rows(prob, its, pre, b, k), _cols(prob, its, a, k))]
                Bp[k] -= acc
            Ya = np.empty_like(Bp)
            Ya[K] = Bp[K]
            for k in range(K - 1, -1, -1):
                Ya[k] = Ya[k + 1] @ E[k] + Bp[k]
        Y[:, :, sl[a]] = Ya
    return Y


# ------------------------------------------------------------------------------------------------------------ the cases
def three_level_problem(n=40, N=6, m=2, seed=31):
    """x <- u <- du <- ddu with two kets of DIFFERENT skew generators; list order [ket 1, (u, du), ket 2, (du, ddu)] is not the
    dependency order: levels 2, 1, 2, 0"""
    rng = np.random.default_rng(seed)
    z = 2 * n + 3 * m + 1

    def skew():
        G = rng.standard_normal((m + 1, n, n))
        return (G - G.transpose(0, 2, 1)) / np.sqrt(2.0 * n)

    Zk = rng.standard_normal((N, z))
    Zk[:, 2 * n:2 * n + m] *= 0.1
    Zk[:, z - 1] = 0.1 + 0.05 * rng.random(N)
    integ = [O.BilinearIntegrator(0, n, 2 * n, m, skew()), O.DerivativeIntegrator(2 * n, m, 2 * n + m),
             O.BilinearIntegrator(n, n, 2 * n, m, skew()), O.DerivativeIntegrator(2 * n + m, m, 2 * n + 2 * m)]
    return O.Problem(N=N, z=z, dt_idx=z - 1, integrators=integ, objectives=[O.QuadraticRegularizer(2 * n, m, np.ones(m))],
                     Z0=Zk.reshape(-1).copy())


CASES = ["scaled_12x9", "scaled_40x6", "scaled_70x12", "three_level_40x6", "multi_ket_between", "tdb_order0", "tdb_order1", "tdb_72x5",
         "structured_16x4"]
SMALL_CASES = ["scaled_12x9", "three_level_12x6", "multi_ket_between_6", "tdb_order0", "tdb_order1"]   # what the CPU tests afford


@functools.lru_cache(maxsize=None)
def case(name):
    """oracle problem, engine problem, Evaluator keywords, the oracle's dense Jacobian, MM and a right-hand side of 3 columns with both
    dense solutions: computed once, shared, never written"""
    kw, pe = {}, None
    if name.startswith("scaled_"):
        n, N = (int(v) for v in name[7:].split("x"))
        p = O.make_scaled_problem(N, n, 2, seed=300 + n + N, skew=True)
    elif name.startswith("three_level_"):
        n, N = (int(v) for v in name[12:].split("x"))
        p = three_level_problem(n, N)
    elif name.startswith("multi_ket_between"):
        pe = multi_ket(6 if name.endswith("_6") else 40, 2, 5, derivative_between=True)
        p, kw = to_oracle(pe), dict(shared_generators=True)
    elif name in ("tdb_order0", "tdb_order1"):
        p = O.make_tdb_problem(N=6, n=4, m=2, order=int(name[-1]), substeps=16, with_derivative=True)
    elif name == "tdb_72x5":
        p = O.make_tdb_problem(N=5, n=72, m=2, substeps=4, with_derivative=True)   # (four RK4 steps keep the oracle's Jacobian to seconds)
    elif name == "structured_16x4":
        p, kw = kron_problem(16, 4, 2, 5, seed=3), dict(block_generators=True)
    else:
        raise KeyError(name)
    if pe is None:
        pe = to_engine(p)
    Z = np.ascontiguousarray(p.Z0, dtype=np.float64)
    Jd = dense_jacobian(p, Z)
    M = assemble(Jd, p)
    D = sum(i.x_dim for i in p.integrators)
    B = np.random.default_rng(len(name)).standard_normal((p.N, 3, D))
    ref = (dense_solve(M, B, False), dense_solve(M, B, True))
    for a in (Z, Jd, M, B) + ref:
        a.setflags(write=False)
    return dict(p=p, pe=pe, kw=kw, Z=Z, Jd=Jd, M=M, B=B, ref=ref, D=D, plan=plan(describe(p), p.dt_idx, p.N - 1))


class RawDerivativeHandle:
    """A handle made of DerivativeIntegrators alone, straight through dto_create: layouts the host mirror cannot state (states that
    overlap, an integrator that differentiates itself) and the derivative-only handle.  `integs`: (x_off, x_dim, xdot_off) each; the
    timestep is the last of `z` components.  device -1: structure only."""

    def __init__(self, integs, z, N=4, device=-1, seed=0):
        import ctypes as C
        capi = dto_amd.capi
        self.lib, self.N, self.z, self.D = dto_amd.load_library(), N, z, sum(d for _, d, _ in integs)
        integ = (capi.IntegratorDesc * len(integs))(*[capi.IntegratorDesc(capi.INTEGRATOR_DERIVATIVE, x, d, xd, d, None) for x, d, xd in integs])
        self.Z = np.ascontiguousarray(np.random.default_rng(seed).standard_normal(z * N))
        desc = capi.ProblemDesc(capi.DTO_ABI_VERSION, device, N, z, 0, z - 1, 1, len(integs), 0, 0, 0, integ, None, None,
                                self.Z.ctypes.data_as(capi.c_double_p), 0, 0)
        self.h = capi.H()
        assert self.lib.dto_create(C.byref(desc), C.byref(self.h)) == 0, self.lib.dto_last_error(None).decode()

    def layout(self):
        """None, or the refusal's text"""
        return None if self.lib.dto_dynamics_layout(self.h, None, None, None, None) == 0 else self.lib.dto_last_error(self.h).decode()

    def solve(self, B, adjoint=False):
        """(Y, None) or (None, the refusal's text); B (N, n_cols, D)"""
        dp = dto_amd.capi.c_double_p
        B = np.ascontiguousarray(B, dtype=np.float64)
        Y = np.full(B.shape, np.nan)
        rc = self.lib.dto_dynamics_solve_all(self.h, self.Z.ctypes.data_as(dp), 1 if adjoint else 0, B.ctypes.data_as(dp), B.shape[1],
                                             Y.ctypes.data_as(dp))
        return (Y, None) if rc == 0 else (None, self.lib.dto_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.dto_destroy(self.h)
            self.h = None


REFUSED_LAYOUTS = {   # name -> (integrators, z, text)
    "cycle": ([(0, 2, 2), (2, 2, 0)], 5, "depend on each other in a cycle"),
    "overlap": ([(0, 2, 4), (1, 2, 4)], 7, "the states of integrators 0 and 1 overlap"),
    "own_inputs": ([(0, 2, 1)], 4, "the inputs of integrator 0 meet its own states"),
}


def engine_jacobian_dense(ev, Z):
    """the dynamics rows of the ENGINE's Jacobian, dense, from its structure and values"""
    rows, cols = ev.jacobian_structure()
    vals = np.full(ev.n_jacobian_entries, np.nan)
    ev.eval_constraint_jacobian(vals, Z)
    J = np.zeros((ev.n_constraints, ev.n_variables))
    J[rows - 1, cols - 1] = vals
    return J[:ev.n_dynamics_constraints]
