"""Shared by the long-horizon tests (test_long_reference.py, test_gpu_long_horizon.py): reduced_cases.reduced_pieces / dense_reference
and elim_cases.dense_solve stated again WITHOUT any dense N D matrix, from the ORACLE alone, so that the references follow the engine
to hundreds of knots.

The dynamics rows of the oracle's Jacobian stay sparse; with S and C of reduced_cases.index_sets, J_S is factored once
(scipy.sparse.linalg.splu) and the tangent map is applied as an operator:
    T v  = [v_C ; -J_S^-1 J_C v_C]          T' q = q_C - J_C' J_S^-T q_S          lam = -J_S^-T g_S
H(Z; sigma, [lam; mu_con]) is the oracle's structure and values as a sparse symmetric matrix (reduced_cases.dense_hessian minus the
.toarray()).  The whole-dynamics solves' reference is a sparse factorisation of MM in the index order of elim_cases.assemble.
||T||_2 comes from svds on a LinearOperator, ||H||_2 from eigsh.  The bars are the formulas of reduced_cases (product_bar,
gradient_bar, kappa with KAPPA_CAP) and test_gpu_rollout.bar(K) x levels, unchanged.

Every solve can take one step of iterative refinement with the residual in np.longdouble (`refine`): the difference between a refined
and an unrefined result is the estimate of the reference's own error that test_long_reference.py holds to 1/100 of each bar.

Cases: the names of reduced_cases.problem (scaled_{n}x{N}, three_level_{n}x{N}, +con).  The point is Z0 with the time steps replaced by
3 / (N - 1) (0.75 + 0.5 u_k), u = default_rng(N).random(N): a fixed total span, so that conditioning does not grow with N faster than
it must.  The values tests' directions are SMOOTHED, v = T'T w / ||T'T w|| with w random and T the reference's: at these lengths a
random direction has kappa above the cap (1.6e4 at 40 x 258, 1e5 at 12 x 1026), a smoothed one 3.5e2 .. 7.4e3."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import dto_oracle as O
import reduced_cases as R
from elim_cases import describe, plan
from helpers import to_engine

SPAN = 3.0

C1_CASES = ["scaled_12x2", "scaled_12x3", "scaled_12x65", "scaled_12x66", "scaled_12x258", "three_level_12x66"]   # K = 1, 2, 64, 65, 257
C1_OPERATOR_CASES = C1_CASES + ["scaled_12x66+con"]
C2_CASE = "scaled_40x258"
C3_CASE = "scaled_64x320"                      # Jacobian only: no oracle Hessian is evaluated at this shape
MISTAKE_CASE = "scaled_12x258"
LONG_CASES = C1_OPERATOR_CASES + [C2_CASE]     # every case with the full reference


# ---------------------------------------------------------------------------------------------------------- sparse pieces
def long_point(p):
    """Z0 with the time-step components replaced: a fixed total span"""
    Z = np.array(p.Z0, dtype=np.float64)
    Zk = Z[:p.N * p.z].reshape(p.N, p.z)
    Zk[:, p.dt_idx] = SPAN / (p.N - 1) * (0.75 + 0.5 * np.random.default_rng(p.N).random(p.N))
    return Z


def sparse_jacobian(p, Z):
    """the dynamics rows of the oracle's Jacobian: (K D, n_vars), CSR"""
    return sp.vstack([O.integrator_jacobian(it, p, Z) for it in p.integrators]).tocsr()


def sparse_hessian(ev_o, Z, sigma, mu):
    """reduced_cases.dense_hessian without the .toarray()"""
    r1, c1 = ev_o.hessian_structure1()
    n = ev_o.prob.n_vars
    U = sp.coo_matrix((ev_o.eval_hessian_lagrangian(Z, sigma, mu), (r1 - 1, c1 - 1)), shape=(n, n)).tocsr()   # duplicates summed
    return (U + U.T - sp.diags(U.diagonal())).tocsr()


def constraint_rows(p, Z):
    """the oracle's Jacobian of the non-dynamics rows, sparse: (n_cons - n_dyn, n_vars)"""
    if not p.constraints:
        return sp.csr_matrix((0, p.n_vars))
    return sp.vstack([O.constraint_jacobian(c, p, Z) for c in p.constraints]).tocsr()


class Factor:
    """a sparse square matrix with its LU factors: solves with A or A', one right-hand side or several columns, with or without one
    step of iterative refinement whose residual is formed in np.longdouble"""

    def __init__(self, A):
        self.A = A.tocsc()
        self.lu = spla.splu(self.A)
        coo = self.A.tocoo()
        self._row, self._col, self._val = coo.row, coo.col, coo.data.astype(np.longdouble)

    def residual(self, x, b, trans=False):
        """b - A x (trans: b - A' x), accumulated in np.longdouble, one column"""
        r, c = (self._col, self._row) if trans else (self._row, self._col)
        out = np.asarray(b, dtype=np.longdouble).copy()
        np.subtract.at(out, r, self._val * np.asarray(x, dtype=np.longdouble)[c])
        return out

    def solve(self, b, trans=False, refine=False):
        b = np.asarray(b, dtype=np.float64)
        x = self.lu.solve(b, trans="T" if trans else "N")
        if refine:
            cols = x.reshape(x.shape[0], -1)
            bc = b.reshape(b.shape[0], -1)
            for j in range(cols.shape[1]):
                cols[:, j] += self.lu.solve(self.residual(cols[:, j], bc[:, j], trans).astype(np.float64), trans="T" if trans else "N")
            x = cols.reshape(x.shape)
        return x

    def cond1(self):
        """the 1-norm condition number, estimated (scipy.sparse.linalg.onenormest on the inverse as an operator)"""
        n = self.A.shape[0]
        inv = spla.LinearOperator((n, n), matvec=lambda v: self.lu.solve(np.asarray(v, dtype=np.float64).reshape(-1)),
                                  rmatvec=lambda v: self.lu.solve(np.asarray(v, dtype=np.float64).reshape(-1), trans="T"))
        return float(spla.onenormest(self.A) * spla.onenormest(inv))


def sparse_pieces(p, Z, sigma, mu, Jd=None):
    """g, the factored J_S, J_C, lam: reduced_cases.reduced_pieces with T kept as an operator"""
    S, C, _, _ = R.index_sets(p)
    Jd = sparse_jacobian(p, Z) if Jd is None else Jd
    n_dyn = Jd.shape[0]
    Jc = constraint_rows(p, Z)
    mu_c = np.zeros(Jc.shape[0]) if mu is None else np.asarray(mu)[n_dyn:]
    g = sigma * O.objective_gradient(p, Z) + Jc.T @ mu_c
    Jcsc = Jd.tocsc()
    q = dict(S=S, C=C, g=g, JS=Factor(Jcsc[:, S]), JC=Jcsc[:, C].tocsr(), mu_c=mu_c, n_dyn=n_dyn, n_vars=p.n_vars)
    q["lam"] = -q["JS"].solve(g[S], trans=True)
    return q


def apply_T(q, vC, refine=False):
    """T v as an n_vars vector, from v on C"""
    x = np.zeros(q["n_vars"])
    x[q["C"]] = vC
    x[q["S"]] = -q["JS"].solve(q["JC"] @ vC, refine=refine)
    return x


def apply_Tt(q, x, refine=False):
    """T' x on C, from an n_vars vector"""
    return x[q["C"]] - q["JC"].T @ q["JS"].solve(x[q["S"]], trans=True, refine=refine)


def norm_T(q, seed=0):
    """||T||_2: the largest singular value of the operator"""
    nC = q["C"].size
    op = spla.LinearOperator((q["n_vars"], nC), matvec=lambda v: apply_T(q, np.asarray(v, dtype=np.float64).reshape(-1)),
                             rmatvec=lambda x: apply_Tt(q, np.asarray(x, dtype=np.float64).reshape(-1)))
    if nC <= 2:
        return float(np.linalg.norm(np.column_stack([apply_T(q, e) for e in np.eye(nC)]), 2))
    v0 = np.random.default_rng(seed).standard_normal(nC)
    return float(spla.svds(op, k=1, v0=v0, tol=1e-9, return_singular_vectors=False)[0])


def norm_H(H, seed=0):
    """||H||_2 of a sparse symmetric matrix: the eigenvalue of largest magnitude"""
    if H.shape[0] <= 64:
        return float(np.linalg.norm(H.toarray(), 2))
    v0 = np.random.default_rng(seed).standard_normal(H.shape[0])
    return float(abs(spla.eigsh(H, k=1, which="LM", v0=v0, tol=1e-9, return_eigenvectors=False)[0]))


def sparse_reference(p, Z, sigma, mu, mistake=None, base=None, Jd=None):
    """reduced_cases.dense_reference without a dense matrix: r_ref, the sparse H, the operator's pieces and the norms the bars are made
    of.  mistake: None, "zero", "plus", "shift" as there.  base: a reference at the same point whose pieces and ||T|| are taken over; Jd: the
    sparse Jacobian at the point, if it is at hand."""
    q = sparse_pieces(p, Z, sigma, mu, Jd) if base is None else {k: base[k] for k in ("S", "C", "g", "JS", "JC", "mu_c", "n_dyn", "n_vars", "lam")}
    lam = {None: q["lam"], "zero": 0.0 * q["lam"], "plus": -q["lam"], "shift": R.shift_one_knot(p, q["lam"])}[mistake]
    mut = np.concatenate([lam, q["mu_c"]])
    H = sparse_hessian(O.OracleEvaluator(p), Z, sigma, mut)
    r = np.zeros(p.n_vars)
    r[q["C"]] = apply_Tt(q, q["g"])
    return dict(q, r_ref=r, H=H, nT=norm_T(q) if base is None else base["nT"], nH=norm_H(H), ng=float(np.linalg.norm(q["g"])), mut=mut)


def product_ref(ref, v, refine=False):
    """y_ref = T' H T v as an n_vars vector (zero on S); the S entries of v are not read"""
    y = np.zeros(v.size)
    y[ref["C"]] = apply_Tt(ref, ref["H"] @ apply_T(ref, v[ref["C"]], refine), refine)
    return y


def gradient_ref(ref, refine=False):
    r = np.zeros(ref["n_vars"])
    r[ref["C"]] = apply_Tt(ref, ref["g"], refine)
    return r


product_bar, gradient_bar, KAPPA_CAP = R.product_bar, R.gradient_bar, R.KAPPA_CAP   # the formulas of reduced_cases: they read nT, nH, ng, C


def kappa(ref, v, y=None):
    """reduced_cases.kappa with the sparse product"""
    y = product_ref(ref, v) if y is None else y
    return ref["nT"] ** 2 * ref["nH"] * float(np.linalg.norm(v[ref["C"]])) / float(np.linalg.norm(y))


def smoothed_direction(ref, rng):
    """v = T'T w / ||T'T w|| on C with w random, zero on S: T from the reference, never from the engine"""
    w = rng.standard_normal(ref["C"].size)
    vC = apply_Tt(ref, apply_T(ref, w))
    v = np.zeros(ref["n_vars"])
    v[ref["C"]] = vC / np.linalg.norm(vC)
    return v


# ------------------------------------------------------------------------------------------------ the whole-dynamics block
def sparse_MM(Jd, p):
    """MM of elim_cases.assemble, sparse: identity rows for knot 1, below them every integrator's defect rows in the state columns; row
    and column index k D + pre_i + r"""
    its = describe(p)
    N, K, z = p.N, p.N - 1, p.z
    D = sum(i["x_dim"] for i in its)
    pre = [sum(i["x_dim"] for i in its[:a]) for a in range(len(its))]
    base = np.concatenate([i["x_off"] + np.arange(i["x_dim"]) for i in its])
    cols = (np.arange(N)[:, None] * z + base[None, :]).reshape(-1)
    rows = np.hstack([K * pre[a] + np.arange(K)[:, None] * i["x_dim"] + np.arange(i["x_dim"])[None, :] for a, i in enumerate(its)]).reshape(-1)
    top = sp.hstack([sp.identity(D, format="csr"), sp.csr_matrix((D, K * D))])
    return sp.vstack([top, Jd.tocsr()[rows][:, cols]]).tocsc()


def sparse_solve(F, B, adjoint, refine=False):
    """elim_cases.dense_solve with the factored sparse MM: B and the result (N, n_cols, D)"""
    N, nc, D = B.shape
    rhs = np.ascontiguousarray(B.transpose(0, 2, 1).reshape(N * D, nc))
    return F.solve(rhs, trans=adjoint, refine=refine).reshape(N, D, nc).transpose(0, 2, 1)


# ------------------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def jac_case(name):
    """what needs the oracle's Jacobian alone: the problems, the point, the factored MM, a right-hand side of 3 columns with both sparse
    solutions: computed once, shared, never written"""
    p, kw = R.problem(name)
    Z = long_point(p)
    Jd = sparse_jacobian(p, Z)
    MM = Factor(sparse_MM(Jd, p))
    D = sum(it.x_dim for it in p.integrators)
    B = np.random.default_rng(len(name)).standard_normal((p.N, 3, D))
    ref = (sparse_solve(MM, B, False), sparse_solve(MM, B, True))
    for a in (Z, B) + ref:
        a.setflags(write=False)
    n_dyn = D * (p.N - 1)
    return dict(name=name, p=p, pe=to_engine(p), kw=kw, Z=Z, Jd=Jd, MM=MM, B=B, ref_solve=ref, D=D, plan=plan(describe(p), p.dt_idx, p.N - 1),
                levels=plan(describe(p), p.dt_idx, p.N - 1)["n_levels"], n_dyn=n_dyn,
                n_cons=n_dyn + sum(c.g_dim * len(c.times1) for c in p.constraints))


@functools.lru_cache(maxsize=None)
def case(name):
    """jac_case plus mu (None, or random on the constraint rows), the sparse reference at sigma = reduced_cases.SIGMA and two smoothed
    directions with their reference products"""
    c = dict(jac_case(name))
    p, Z = c["p"], c["Z"]
    mu = None
    if name.endswith("+con"):
        mu = np.zeros(c["n_cons"])
        mu[c["n_dyn"]:] = np.random.default_rng(11).standard_normal(c["n_cons"] - c["n_dyn"])
    ref = sparse_reference(p, Z, R.SIGMA, mu, Jd=c["Jd"])
    rng = np.random.default_rng(len(name))
    vs = [smoothed_direction(ref, rng) for _ in range(2)]
    ys = [product_ref(ref, v) for v in vs]
    for a in vs + ys + ([mu] if mu is not None else []) + [x for x in ref.values() if isinstance(x, np.ndarray)]:
        a.setflags(write=False)
    return dict(c, mu=mu, ref=ref, vs=vs, ys=ys)
