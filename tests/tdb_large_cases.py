"""Reference values for TimeDependentBilinearIntegrator problems of 65 states and more (NumPy only).

`O.OracleEvaluator` differentiates the integrator's Hessian numerically over all 2z inputs of an interval, which does not finish
in minutes at these sizes.  `reference(prob)` keeps the oracle's evaluator -- its structure, its ordering, its scatter and every
other term -- and replaces only the integrator's dense blocks by a fast form of the SAME discrete map (classical RK4 with
`substeps` fixed steps, `O.TimeDependentBilinearIntegrator.f`), using that the state enters linearly:

    d f / d x_k      = -Phi,  Phi = R_S ... R_1 the product of the sub-steps' RK4 step matrices
                       R = I + h/6 (K1 + 2 K2 + 2 K3 + K4),  K1 = M1, K2 = M2 (I + h/2 K1), K3 = M2 (I + h/2 K2), K4 = M4 (I + h K3)
    d f / d theta_b  = -(d Phi / d theta_b) x_k          complex step over theta = [u_k, t_k, dt_k, u_{k+1} (order 1)]
    (x, theta_b)     = -(d Phi / d theta_b)' mu          the same complex step, of Phi' mu
    (theta_a, theta_b) = -mu' d/d theta_b [d (Phi x_k) / d theta_a]   complex step of the analytic first-order forward sensitivity
                       (the scheme applied to y_a' = M y_a + M_a y)

No real-valued finite difference anywhere: every figure is exact to rounding.  tests/test_tdb_large_reference.py pins this helper
to `O.OracleEvaluator` at 8 and 24 states."""
import dataclasses

import numpy as np

import dto_oracle as O

_EPS = 1e-30


class FastTdb(O.TimeDependentBilinearIntegrator):
    """The oracle's integrator with `jac` and `hess` in the fast form above; `f`, `rhs`, `generator` are the oracle's own."""

    def _params(self):
        m = self.u_dim
        z = self.z
        idx = [self.u_off + j for j in range(m)] + [self.t_off, self.dt_idx]
        if self.spline_order == 1:
            idx += [z + self.u_off + j for j in range(m)]
        return idx

    def _split(self, th):
        m = self.u_dim
        uk, tk, dt = th[:m], th[m], th[m + 1]
        uk1 = th[m + 2:] if self.spline_order == 1 else uk
        return uk, tk, dt, uk1

    def _M(self, th, tau):
        uk, tk, dt, uk1 = self._split(th)
        u = uk + tau * (uk1 - uk) if self.spline_order == 1 else uk
        return dt * self.generator(u, tk + tau * dt)

    def _flow(self, th):
        """Phi(theta) (n x n), complex where theta is."""
        n, S = self.x_dim, self.substeps
        h = 1.0 / S
        I = np.eye(n)
        Phi = np.eye(n, dtype=np.result_type(th, np.float64))
        for i in range(S):
            M1, M2, M4 = self._M(th, i * h), self._M(th, (i + 0.5) * h), self._M(th, (i + 1.0) * h)
            K1 = M1
            K2 = M2 @ (I + 0.5 * h * K1)
            K3 = M2 @ (I + 0.5 * h * K2)
            K4 = M4 @ (I + h * K3)
            Phi = (I + (h / 6.0) * (K1 + 2.0 * K2 + 2.0 * K3 + K4)) @ Phi
        return Phi

    def _dM(self, th, tau):
        """[d M / d theta_a] (p, n, n), analytic, complex where theta is."""
        m = self.u_dim
        uk, tk, dt, uk1 = self._split(th)
        order1 = self.spline_order == 1
        u = uk + tau * (uk1 - uk) if order1 else uk
        t = tk + tau * dt
        dtype = np.result_type(th, np.float64)
        ub = np.concatenate([np.ones(1, dtype=dtype), u])
        E = self.G.astype(dtype)                      # E_j = G_j + sum_c phi_c(t) H_cj
        Mt = np.zeros(self.G.shape[1:], dtype=dtype)  # sum_j ubar_j sum_c phi_c'(t) H_cj
        for kind, w, Hc in self.mods:
            phi, dphi = (np.cos(w * t), -w * np.sin(w * t)) if kind == "cos" else (np.sin(w * t), w * np.cos(w * t))
            E = E + phi * Hc
            Mt = Mt + dphi * np.einsum("j,jrc->rc", ub, Hc)
        out = [dt * ((1.0 - tau) if order1 else 1.0) * E[1 + j] for j in range(m)]
        out.append(dt * Mt)
        out.append(np.einsum("j,jrc->rc", ub, E) + dt * tau * Mt)
        if order1:
            out += [dt * tau * E[1 + j] for j in range(m)]
        return np.stack(out)

    def _sens(self, th, x):
        """d (Phi x) / d theta_a (p, n): the scheme applied to y' = M y, y_a' = M y_a + M_a y."""
        S = self.substeps
        h = 1.0 / S
        p = len(th)
        y = x.astype(np.result_type(th, np.float64))
        ya = np.zeros((p, x.size), dtype=y.dtype)

        def F(M, dM, v, va):
            return M @ v, va @ M.T + np.einsum("arc,c->ar", dM, v)

        for i in range(S):
            taus = (i * h, (i + 0.5) * h, (i + 1.0) * h)
            Ms = [self._M(th, t) for t in taus]
            dMs = [self._dM(th, t) for t in taus]
            k1, k1a = F(Ms[0], dMs[0], y, ya)
            k2, k2a = F(Ms[1], dMs[1], y + 0.5 * h * k1, ya + 0.5 * h * k1a)
            k3, k3a = F(Ms[1], dMs[1], y + 0.5 * h * k2, ya + 0.5 * h * k2a)
            k4, k4a = F(Ms[2], dMs[2], y + h * k3, ya + h * k3a)
            y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            ya = ya + (h / 6.0) * (k1a + 2.0 * k2a + 2.0 * k3a + k4a)
        return ya

    def _flows(self, zz):
        """Phi and [d Phi / d theta_b] at the interval's point."""
        idx = self._params()
        th = np.asarray(zz, dtype=np.float64)[idx]
        dPhi = []
        for b in range(len(idx)):
            tc = th.astype(np.complex128)
            tc[b] += 1j * _EPS
            dPhi.append(self._flow(tc).imag / _EPS)
        return idx, th, self._flow(th), dPhi

    def jac(self, zz, k=0):
        zz = np.asarray(zz, dtype=np.float64)
        n, z = self.x_dim, self.z
        idx, th, Phi, dPhi = self._flows(zz)
        x = zz[self.x_off:self.x_off + n]
        J = np.zeros((n, 2 * z))
        J[:, self.x_off:self.x_off + n] += -Phi
        J[:, z + self.x_off:z + self.x_off + n] += np.eye(n)
        for b, col in enumerate(idx):
            J[:, col] += -(dPhi[b] @ x)
        return J

    def hess(self, zz, k, mu):
        zz = np.asarray(zz, dtype=np.float64)
        mu = np.asarray(mu, dtype=np.float64)
        n, z = self.x_dim, self.z
        idx, th, Phi, dPhi = self._flows(zz)
        x = zz[self.x_off:self.x_off + n]
        p = len(idx)
        H = np.zeros((2 * z, 2 * z))
        xs = np.arange(self.x_off, self.x_off + n)
        for b, col in enumerate(idx):
            v = -(dPhi[b].T @ mu)
            H[xs, col] += v
            H[col, xs] += v
        T = np.zeros((p, p))                       # T[a, b] = mu' d/d theta_b [d (Phi x) / d theta_a]
        for b in range(p):
            tc = th.astype(np.complex128)
            tc[b] += 1j * _EPS
            T[:, b] = (self._sens(tc, x).imag / _EPS) @ mu
        T = 0.5 * (T + T.T)
        for a, ca in enumerate(idx):
            for b, cb in enumerate(idx):
                H[ca, cb] += -T[a, b]
        return H


def fast_problem(prob):
    """`prob` with every TimeDependentBilinearIntegrator replaced by its fast form (everything else shared)."""
    integ = []
    for it in prob.integrators:
        if isinstance(it, O.TimeDependentBilinearIntegrator):
            it = FastTdb(**{f.name: getattr(it, f.name) for f in dataclasses.fields(it)})
        integ.append(it)
    return dataclasses.replace(prob, integrators=integ)


_cache = {}


def reference(prob, key, sigma=0.6, mu_seed=1):
    """(evaluator, mu, g, Jacobian values, Hessian-of-Lagrangian values) of `prob` at prob.Z0, in the evaluator's order; computed
    once per `key` and shared (callers leave the arrays unchanged)."""
    if key not in _cache:
        ev = O.OracleEvaluator(fast_problem(prob))
        mu = np.random.default_rng(mu_seed).standard_normal(ev.n_constraints)
        Z = prob.Z0
        out = (ev, mu, ev.eval_constraint(Z), ev.eval_constraint_jacobian(Z), ev.eval_hessian_lagrangian(Z, sigma, mu))
        for a in out[1:]:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]
