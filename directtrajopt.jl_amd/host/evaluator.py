"""``Evaluator`` -- mirror of the reference's ``Solvers.Evaluator <: MOI.AbstractNLPEvaluator``
(src/solvers/evaluator.jl:66-98, 291-456) on top of the C ABI.  Method names follow MOI."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import library_path, load_library  # noqa: F401
from .problem import (BilinearIntegrator, CompositeObjective, DerivativeIntegrator, GlobalKnotPointObjective, HostIntegrator,
                      KnotPointObjective, TimeDependentBilinearIntegrator, LinearRegularizer, MinimumTimeObjective, NonlinearGlobalConstraint,
                      NonlinearKnotPointConstraint, NullObjective, QuadraticRegularizer)


class EngineError(RuntimeError):
    pass


def _dp(a):
    return a.ctypes.data_as(capi.c_double_p)


def _ip(a):
    return a.ctypes.data_as(capi.c_int64_p)


def _out(a, n, what):
    """An output buffer the engine writes `n` doubles into: it must be a C-contiguous float64 ndarray of exactly that
    size (the engine's device-to-host copy would otherwise run past it or land in the wrong bytes)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
        raise ValueError(f"{what}: need a writeable C-contiguous float64 ndarray")
    if a.size != n:
        raise ValueError(f"{what}: length {a.size}, the engine writes {n} (shard-local slab lengths are in Evaluator.shard)")
    return _dp(a)


def _in(a, n, what):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size != n:
        raise ValueError(f"{what}: length {a.size}, expected {n}")
    return a


def _flatten_objective(obj):
    if obj is None or isinstance(obj, NullObjective):
        return []
    if isinstance(obj, CompositeObjective):
        out = []
        for o, w in zip(obj.objectives, obj.weights):
            if isinstance(o, NullObjective):
                continue
            if isinstance(o, CompositeObjective):
                raise ValueError("nested CompositeObjective: `+` flattens them (_objectives.jl:165-176)")
            out.append((o, w))
        return out
    return [(obj, 1.0)]


class Evaluator:
    """Evaluator(prob; eval_hessian=true) -- evaluator.jl:99-288.

    Extra keyword arguments select the device and, for multi-GPU runs, the owned knot range
    ``k_lo..k_hi`` (1-based, inclusive).  Inputs ``Z`` and ``mu`` are always the GLOBAL vectors;
    value outputs are the shard-local slabs described by ``shard`` (whole vectors when unsharded).

    ``shared_generators=True`` (DTO_FLAG_SHARED_GENERATORS) groups integrators driven by one system -- the kets of a multi-state
    problem.  BilinearIntegrators with equal generators and controls share the Jacobian's propagator chain (33 states and up).
    Device TimeDependentBilinearIntegrators with the same family (every G_j and H_cj, modulation kinds and frequencies), controls,
    time component, spline order and sub-steps share one propagation per eval_constraint, Jacobian and Hessian call at 65..256
    states: one launch per group instead of one per integrator.  Values are bit-identical to the unflagged handle's either way;
    ``integrator_share`` tells what was found."""

    # options applied to every new handle (dto_set_option name -> value); the repository's tests switch "host_xfer_check" on here
    default_options = {}

    def __init__(self, prob, eval_hessian=True, device=0, k_lo=0, k_hi=0, verbose=False, general_path_only=False,
                 block_generators=False, shared_generators=False):
        self._lib = load_library()
        self._h = capi.H()
        traj = prob.trajectory
        self.trajectory = traj
        self.eval_hessian = bool(eval_hessian)
        keep = []  # keep numpy buffers alive across dto_create

        self._ext_int = []  # (integrator, first global row)
        integ = (capi.IntegratorDesc * max(1, len(prob.integrators)))()
        for i, it in enumerate(prob.integrators):
            if isinstance(it, BilinearIntegrator):
                # column-major n x n per generator = transpose of numpy's row-major
                G = np.ascontiguousarray(np.transpose(it.G, (0, 2, 1)))
                keep.append(G)
                integ[i] = capi.IntegratorDesc(capi.INTEGRATOR_BILINEAR, it.x_off, it.x_dim, it.u_off, it.u_dim, _dp(G))
            elif isinstance(it, DerivativeIntegrator):
                integ[i] = capi.IntegratorDesc(capi.INTEGRATOR_DERIVATIVE, it.x_off, it.x_dim, it.xdot_off, it.x_dim, None)
            elif isinstance(it, TimeDependentBilinearIntegrator) and it.family is not None:
                fam = it.family
                G = np.ascontiguousarray(np.transpose(fam.G, (0, 2, 1)))  # column-major per matrix
                kinds = np.ascontiguousarray([1 if k == "cos" else 2 for k, _, _ in fam.mods], dtype=np.int32)
                omegas = np.ascontiguousarray([w for _, w, _ in fam.mods], dtype=np.float64)
                Hs = (np.ascontiguousarray(np.stack([np.transpose(Hc, (0, 2, 1)) for _, _, Hc in fam.mods]))
                      if fam.mods else np.zeros(1))
                keep += [G, kinds, omegas, Hs]
                integ[i] = capi.IntegratorDesc(capi.INTEGRATOR_TIME_DEPENDENT_BILINEAR, it.x_off, it.x_dim, it.u_off, it.u_dim, _dp(G),
                                               it.t_off, it.spline_order, it.substeps, len(fam.mods),
                                               kinds.ctypes.data_as(capi.c_int32_p) if fam.mods else None,
                                               _dp(omegas) if fam.mods else None, _dp(Hs) if fam.mods else None)
            elif isinstance(it, HostIntegrator):
                integ[i] = capi.IntegratorDesc(capi.INTEGRATOR_EXTERNAL, 0, it.x_dim, 0, 0, None)
                self._ext_int.append((it, sum(p.dim for p in prob.integrators[:i])))
            else:
                raise NotImplementedError(f"{type(it).__name__}: wrap it in HostIntegrator to have it merged")

        self._integrator_dims = [it.x_dim for it in prob.integrators]
        # per integrator: its first row of g and (device kinds) the position of its states inside a knot
        self._integrator_row0 = [sum(p.dim for p in prob.integrators[:i]) for i in range(len(prob.integrators))]
        self._integrator_x_off = [getattr(it, "x_off", None) for it in prob.integrators]
        self._integrator_list = list(prob.integrators)
        self._ext_con, self._ext_obj, self._ext_keep = [], [], None
        terms = _flatten_objective(prob.objective)
        objs = (capi.ObjectiveDesc * max(1, len(terms)))()
        for i, (o, w) in enumerate(terms):
            d = capi.ObjectiveDesc()
            d.weight = w
            if isinstance(o, MinimumTimeObjective):
                d.kind, d.D = capi.OBJECTIVE_MINTIME, o.D
            elif isinstance(o, (QuadraticRegularizer, LinearRegularizer)):
                d.kind = capi.OBJECTIVE_QUADRATIC if isinstance(o, QuadraticRegularizer) else capi.OBJECTIVE_LINEAR
                d.comp_off, d.comp_dim = o.comp_off, o.comp_dim
                R = np.ascontiguousarray(o.R, dtype=np.float64)
                keep.append(R)
                d.R = _dp(R)
                if getattr(o, "baseline", None) is not None:
                    b = np.ascontiguousarray(o.baseline.T, dtype=np.float64)  # column-major comp_dim x N
                    keep.append(b)
                    d.baseline = _dp(b)
                if o.times is not None:
                    t = np.ascontiguousarray(o.times, dtype=np.int64)
                    keep.append(t)
                    d.times, d.n_times = _ip(t), t.size
            elif isinstance(o, GlobalKnotPointObjective):  # incl. GlobalObjective
                d.kind = capi.OBJECTIVE_EXTERNAL_GLOBAL
                comps = np.ascontiguousarray(o.comps, dtype=np.int32)
                gcomps = np.ascontiguousarray(o.gcomps, dtype=np.int32)
                t = np.ascontiguousarray(o.times, dtype=np.int64)
                keep += [comps, gcomps, t]
                if comps.size:
                    d.comps, d.n_comps = comps.ctypes.data_as(capi.c_int32_p), comps.size
                d.gcomps, d.n_gcomps = gcomps.ctypes.data_as(capi.c_int32_p), gcomps.size
                if t.size:
                    d.times, d.n_times = _ip(t), t.size
                self._ext_obj.append(o)
            elif isinstance(o, KnotPointObjective) and o.external:
                d.kind = capi.OBJECTIVE_EXTERNAL_KNOT
                comps = np.ascontiguousarray(o.comps, dtype=np.int32)
                t = np.ascontiguousarray(o.times, dtype=np.int64)
                keep += [comps, t]
                d.comps, d.n_comps = comps.ctypes.data_as(capi.c_int32_p), comps.size
                d.times, d.n_times = _ip(t), t.size
                self._ext_obj.append(o)
            elif isinstance(o, KnotPointObjective):
                d.kind = KnotPointObjective.KINDS[o.kind]
                comps = np.ascontiguousarray(o.comps, dtype=np.int32)
                t = np.ascontiguousarray(o.times, dtype=np.int64)
                Qs = np.ascontiguousarray(o.Qs, dtype=np.float64)
                keep += [comps, t, Qs]
                d.comps, d.n_comps = comps.ctypes.data_as(capi.c_int32_p), comps.size
                d.times, d.n_times = _ip(t), t.size
                d.Qs = _dp(Qs)
                if getattr(o, "A", None) is not None:
                    A = np.ascontiguousarray(o.A.T, dtype=np.float64)  # column-major k x n_comps
                    keep.append(A)
                    d.R, d.comp_dim = _dp(A), o.A.shape[0]
                if o.params is not None:
                    P = np.ascontiguousarray(o.params, dtype=np.float64)  # rows = times: column-major n_comps x n_times
                    keep.append(P)
                    d.params = _dp(P)
            else:
                raise NotImplementedError(f"{type(o).__name__} stays on the host (closure-based objective)")
            objs[i] = d

        nl = [c for c in prob.constraints if isinstance(c, (NonlinearKnotPointConstraint, NonlinearGlobalConstraint))]
        self._nl_constraints = nl
        cons = (capi.ConstraintDesc * max(1, len(nl)))()
        for i, c in enumerate(nl):
            if isinstance(c, NonlinearGlobalConstraint):
                gcomps = np.ascontiguousarray(c.gcomps, dtype=np.int32)
                _, jac0, hess0 = c.external_blocks(None, 2, mu=np.ones(c.g_dim), g=traj.global_data)  # patterns at Z0, mu = ones
                jac0, hess0 = np.ascontiguousarray(jac0), np.ascontiguousarray(hess0)
                keep += [gcomps, jac0, hess0]
                cons[i] = capi.ConstraintDesc(capi.CONSTRAINT_EXTERNAL_GLOBAL, int(c.equality), gcomps.size, c.g_dim,
                                              gcomps.ctypes.data_as(capi.c_int32_p), 0.0, None, 0, _dp(jac0), _dp(hess0))
                self._ext_con.append(c)
                continue
            comps = np.ascontiguousarray(c.comps, dtype=np.int32)
            t = np.ascontiguousarray(c.times, dtype=np.int64)
            keep += [comps, t]
            if c.external:
                # pattern = the closure's Jacobian at Z0, as the reference takes it (evaluator.jl:136)
                Zk0 = traj.vec()[:traj.dim * traj.N].reshape(traj.N, traj.dim)
                jac0 = np.ascontiguousarray(c.external_blocks(Zk0, 1)[1])
                keep.append(jac0)
                cons[i] = capi.ConstraintDesc(capi.CONSTRAINT_EXTERNAL, int(c.equality), comps.size, c.g_dim,
                                              comps.ctypes.data_as(capi.c_int32_p), 0.0, _ip(t), t.size, _dp(jac0), None)
                self._ext_con.append(c)
                continue
            M = None
            if c.kind == "quadform":  # the matrix rides in hess0, column-major
                M = np.ascontiguousarray(c.M.T, dtype=np.float64)
                keep.append(M)
            cons[i] = capi.ConstraintDesc(NonlinearKnotPointConstraint.KINDS[c.kind], int(c.equality), comps.size, 1,
                                          comps.ctypes.data_as(capi.c_int32_p), c.c, _ip(t), t.size, None,
                                          None if M is None else _dp(M))

        Z0 = np.ascontiguousarray(traj.vec(), dtype=np.float64)
        desc = capi.ProblemDesc(capi.DTO_ABI_VERSION, device, traj.N, traj.dim, traj.global_dim,
                                traj.components[traj.timestep][0], int(eval_hessian), len(prob.integrators),
                                len(terms), len(nl), (capi.FLAG_GENERAL_PATH_ONLY if general_path_only else 0) |
                                (capi.FLAG_BLOCK_GENERATORS if block_generators else 0) |
                                (capi.FLAG_SHARED_GENERATORS if shared_generators else 0), integ, objs, cons,
                                _dp(Z0), k_lo, k_hi)
        if self._lib.dto_create(C.byref(desc), C.byref(self._h)) != 0:
            raise EngineError(self._lib.dto_last_error(None).decode())
        v = C.c_int64()
        self._lib.dto_num_vars(self._h, C.byref(v)); self.n_variables = v.value
        self._lib.dto_num_cons(self._h, C.byref(v)); self.n_constraints = v.value
        self._lib.dto_num_dynamics_cons(self._h, C.byref(v)); self.n_dynamics_constraints = v.value
        self.n_nonlinear_constraints = self.n_constraints - self.n_dynamics_constraints
        self._lib.dto_jac_nnz(self._h, C.byref(v)); self.n_jacobian_entries = v.value
        self._lib.dto_hess_nnz(self._h, C.byref(v)); self.n_hessian_entries = v.value
        self.shard = capi.ShardInfo()
        self._lib.dto_get_shard_info(self._h, C.byref(self.shard))
        for name, value in self.default_options.items():
            self.set_option(name, value)

    # ---- plumbing
    def _check(self, rc):
        if rc != 0:
            raise EngineError(self._lib.dto_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.dto_destroy(self._h)
            self._h = capi.H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def integrator_blocks(self, i):
        """(block_dim, reps, active) of integrator i (0-based): the finest replicated-block structure G_j = I_reps (x) B_j found
        at create with ``block_generators=True`` -- for a TimeDependentBilinearIntegrator the structure shared by every G_j and
        carrier matrix H_cj -- and whether the structured path serves it; (x_dim, 1, 0) otherwise."""
        b, r, a = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.dto_integrator_blocks(self._h, int(i), C.byref(b), C.byref(r), C.byref(a)))
        return b.value, r.value, a.value

    def integrator_share(self, i):
        """(leader, group_size, active) of integrator i (0-based): the group of bilinear integrators with the same generators and
        controls -- or of time-dependent bilinear integrators with the same family, controls, time component and scheme -- found at
        create with ``shared_generators=True``, its first member in list order, and whether the group shares: one propagator chain
        in eval_constraint_jacobian (bilinear), one propagation per callback (time-dependent, 65..256 states on the dense path);
        (i, 1, 0) otherwise.  The two kinds are never grouped with each other."""
        l, n, a = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.dto_integrator_share(self._h, int(i), C.byref(l), C.byref(n), C.byref(a)))
        return l.value, n.value, a.value

    # ---- MOI surface (host vectors)
    def initialize(self, features=None):  # MOI.initialize, evaluator.jl:291
        return None

    def features_available(self):  # evaluator.jl:293-299
        return ["Grad", "Jac", "Hess"] if self.eval_hessian else ["Grad", "Jac"]

    def _Z(self, Z):
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.size != self.n_variables:
            raise ValueError("Z has the wrong length")
        return Z

    def _stage_external(self, Z, con_need=-1, obj_need=-1, mu=None):
        """Evaluate the closure-based knot terms on the host (what the Julia shim does with the reference's
        ForwardDiff code) and hand the blocks to the engine: need 0 = values, 1 = + first derivatives,
        2 = + second derivatives; -1 = this callback does not read that family."""
        if not (self._ext_int or self._ext_con or self._ext_obj):
            return
        if Z is None:
            raise EngineError("closure-based terms need the host copy of Z (pass Z_host to the *_dev call)")
        traj = self.trajectory
        Zk = np.asarray(Z, dtype=np.float64)[:traj.dim * traj.N].reshape(traj.N, traj.dim)
        gdat = np.asarray(Z, dtype=np.float64)[traj.dim * traj.N:]
        ni = len(self._ext_int)
        vals = (capi.ExternalValues * (ni + len(self._ext_con) + len(self._ext_obj)))()
        keep = []
        for i, (it, row0) in enumerate(self._ext_int):  # integrators ride with the constraint-side callbacks
            if con_need < 0:
                continue
            m = None if mu is None else np.asarray(mu, dtype=np.float64)[row0:row0 + it.dim]
            for name, b in zip(("values", "first", "second"), it.external_blocks(Zk, con_need, m)):
                if b is not None:
                    b = np.ascontiguousarray(b, dtype=np.float64)
                    keep.append(b)
                    setattr(vals[i], name, _dp(b))
        row = self.n_dynamics_constraints
        rows = {}
        for c in self._nl_constraints:
            rows[id(c)] = row
            row += c.dim
        for i, c in enumerate(self._ext_con):
            if con_need < 0:
                continue
            m = None if mu is None else np.asarray(mu, dtype=np.float64)[rows[id(c)]:rows[id(c)] + c.dim]
            blocks = (c.external_blocks(Zk, con_need, m, g=gdat) if isinstance(c, NonlinearGlobalConstraint)
                      else c.external_blocks(Zk, con_need, m))
            for name, b in zip(("values", "first", "second"), blocks):
                if b is not None:
                    b = np.ascontiguousarray(b, dtype=np.float64)
                    keep.append(b)
                    setattr(vals[ni + i], name, _dp(b))
        for j, o in enumerate(self._ext_obj):
            if obj_need < 0:
                continue
            blocks = (o.external_blocks(Zk, obj_need, g=gdat) if isinstance(o, GlobalKnotPointObjective)
                      else o.external_blocks(Zk, obj_need))
            for name, b in zip(("values", "first", "second"), blocks):
                if b is not None:
                    b = np.ascontiguousarray(b, dtype=np.float64)
                    keep.append(b)
                    setattr(vals[ni + len(self._ext_con) + j], name, _dp(b))
        self._ext_keep = (vals, keep)  # the engine reads these host buffers during the next callbacks
        self._check(self._lib.dto_set_external(self._h, len(vals), vals))

    def eval_objective(self, Z):  # evaluator.jl:304
        Z = self._Z(Z)
        f = C.c_double()
        self._stage_external(Z, obj_need=0)
        self._check(self._lib.dto_eval_objective(self._h, _dp(Z), C.byref(f)))
        return f.value

    def eval_objective_gradient(self, grad, Z):  # evaluator.jl:310
        Z = self._Z(Z)
        self._stage_external(Z, obj_need=1)
        self._check(self._lib.dto_eval_gradient(self._h, _dp(Z), _out(grad, self.shard.grad_len, "grad")))

    def eval_constraint(self, g, Z):  # evaluator.jl:323
        Z = self._Z(Z)
        self._stage_external(Z, con_need=0)
        self._check(self._lib.dto_eval_constraint(self._h, _dp(Z), _out(g, self.shard.cons_len, "g")))

    def jacobian_structure(self, first=0, count=None):  # evaluator.jl:364 (1-based pairs)
        count = self.n_jacobian_entries - first if count is None else count
        r = np.empty(count, dtype=np.int64)
        c = np.empty(count, dtype=np.int64)
        self._check(self._lib.dto_jacobian_structure(self._h, first, count, _ip(r), _ip(c)))
        return r, c

    def eval_constraint_jacobian(self, vals, Z):  # evaluator.jl:368
        Z = self._Z(Z)
        self._stage_external(Z, con_need=1)
        self._check(self._lib.dto_eval_jacobian(self._h, _dp(Z), _out(vals, self.shard.jac_len, "vals")))

    def hessian_lagrangian_structure(self, first=0, count=None):  # evaluator.jl:385
        count = self.n_hessian_entries - first if count is None else count
        r = np.empty(count, dtype=np.int64)
        c = np.empty(count, dtype=np.int64)
        self._check(self._lib.dto_hessian_structure(self._h, first, count, _ip(r), _ip(c)))
        return r, c

    def eval_hessian_lagrangian(self, H, Z, sigma, mu):  # evaluator.jl:389
        Z = self._Z(Z)
        mu = _in(mu, self.n_constraints, "mu")
        self._stage_external(Z, con_need=2, obj_need=2 if sigma != 0.0 else -1, mu=mu)
        self._check(self._lib.dto_eval_hessian(self._h, _dp(Z), float(sigma), _dp(mu), _out(H, self.shard.hess_len, "H")))

    def eval_hessian_lagrangian_product(self, y, Z, v, sigma, mu):  # MOI.eval_hessian_lagrangian_product (y = H v)
        """y = H(Z; sigma, mu) v with H symmetric (its upper triangle is what eval_hessian_lagrangian returns).  Products at the
        same (Z, sigma, mu) reuse the Hessian the first one assembled on the device -- unless external blocks are staged again,
        which closure-based problems do on every call."""
        Z = self._Z(Z)
        mu = _in(mu, self.n_constraints, "mu")
        v = _in(v, self.n_variables, "v")
        self._stage_external(Z, con_need=2, obj_need=2 if sigma != 0.0 else -1, mu=mu)
        self._check(self._lib.dto_eval_hessian_product(self._h, _dp(Z), float(sigma), _dp(mu), _dp(v), _out(y, self.n_variables, "y")))

    @staticmethod
    def _columns(V, n, what):
        """V as a C-contiguous (n_cols, n) float64 array"""
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[1] != n:
            raise ValueError(f"{what}: shape {V.shape}, expected (n_cols, {n})")
        return V

    def eval_hessian_lagrangian_products(self, Y, Z, V, sigma, mu):
        """Y[c] = H(Z; sigma, mu) V[c] for every row of V (``dto_eval_hessian_products``): ``V`` and ``Y`` are (n_cols, n_variables),
        row c one vector.  Bit for bit ``eval_hessian_lagrangian_product`` of every row, at the same kept point; the Hessian copy is
        read once per tile of columns instead of once per vector (one launch per chunk of ``reduced_block_width`` columns)."""
        Z = self._Z(Z)
        mu = _in(mu, self.n_constraints, "mu")
        V = self._columns(V, self.n_variables, "V")
        self._stage_external(Z, con_need=2, obj_need=2 if sigma != 0.0 else -1, mu=mu)
        self._check(self._lib.dto_eval_hessian_products(self._h, _dp(Z), float(sigma), _dp(mu), V.shape[0], _dp(V),
                                                        _out(Y, V.size, "Y")))

    def eval_constraint_jacobian_product(self, y, Z, w):  # evaluator.jl:406 (y = J w)
        Z = self._Z(Z)
        w = _in(w, self.n_variables, "w")
        self._stage_external(Z, con_need=1)
        self._check(self._lib.dto_eval_jacobian_product(self._h, _dp(Z), _dp(w), _out(y, self.n_constraints, "y")))

    def eval_constraint_jacobian_transpose_product(self, y, Z, w):  # evaluator.jl:432 (y = J' w)
        Z = self._Z(Z)
        w = _in(w, self.n_constraints, "w")
        self._stage_external(Z, con_need=1)
        self._check(self._lib.dto_eval_jacobian_transpose_product(self._h, _dp(Z), _dp(w), _out(y, self.n_variables, "y")))

    def rollout(self, Z, integrator=0, X0=None, all_knots=True):
        """Open-loop rollout X_{k+1} = E_k(Z) X_k of integrator ``integrator`` (0-based position in the integrator list) on the
        device: the states its dynamics reach from X0 under the controls, timesteps and times of Z, whatever states Z holds -- what
        the reference's rollout-fidelity callbacks score.  ``X0``: (n_cols, x_dim), one start state per row (or a single vector),
        1 <= n_cols <= x_dim; None takes the integrator's state at knot 1 of Z.  Returns (N, n_cols, x_dim), knot 1 a copy of X0, or
        with ``all_knots=False`` the (n_cols, x_dim) states at knot N (bit for bit the last block)."""
        Z = self._Z(Z)
        x0 = None
        n_cols = 1
        if X0 is not None:
            x0 = np.ascontiguousarray(np.atleast_2d(np.asarray(X0, dtype=np.float64)))
            n_cols = x0.shape[0]
        its = self._integrator_dims
        if not 0 <= integrator < len(its):
            x_dim = 1   # (the engine refuses the index with text)
        else:
            x_dim = its[integrator]
            if x0 is not None and x0.shape[1] != x_dim:
                raise ValueError(f"X0: rows of length {x0.shape[1]}, the integrator has {x_dim} states")
        N = self.trajectory.N
        X = np.full((N, n_cols, x_dim) if all_knots else (n_cols, x_dim), np.nan)
        self._stage_external(Z, con_need=1)
        self._check(self._lib.dto_rollout(self._h, int(integrator), _dp(Z), None if x0 is None else _dp(x0), n_cols,
                                          capi.ROLLOUT_ALL if all_knots else capi.ROLLOUT_FINAL, _dp(X)))
        return X

    def _solve_shape(self, B, integrator):
        B = np.ascontiguousarray(B, dtype=np.float64)
        N = self.trajectory.N
        if B.ndim == 2 and B.shape[0] == N:
            B = B.reshape(N, 1, B.shape[1])
        if B.ndim != 3 or B.shape[0] != N:
            raise ValueError(f"B: (N, n_cols, x_dim) or (N, x_dim) with N = {N} expected, got {B.shape}")
        its = self._integrator_dims
        if 0 <= integrator < len(its) and B.shape[2] != its[integrator]:
            raise ValueError(f"B: rows of length {B.shape[2]}, the integrator has {its[integrator]} states")
        return B

    def dynamics_solve(self, Z, B, integrator=0, adjoint=False, all_knots=True):
        """Solve with the dynamics block M of integrator ``integrator`` at Z (I on the diagonal, -E_k(Z) below it), on the device.
        Forward: M Y = B, the linearised rollout Y_1 = B_1, Y_{k+1} = E_k Y_k + B_{k+1}.  ``adjoint=True``: M' L = B, the costate
        recursion L_N = B_N, L_k = E_k' L_{k+1} + B_k.  ``B``: (N, n_cols, x_dim), or (N, x_dim) for one column.  Returns
        (N, n_cols, x_dim), or with ``all_knots=False`` the (n_cols, x_dim) block at knot N (forward) or knot 1 (adjoint), bit for bit
        that block.  A second solve at the same Z, in either direction, reuses the product tree of the first."""
        Z = self._Z(Z)
        B = self._solve_shape(B, integrator)
        N, n_cols, x_dim = B.shape
        Y = np.full((N, n_cols, x_dim) if all_knots else (n_cols, x_dim), np.nan)
        self._stage_external(Z, con_need=1)
        self._check(self._lib.dto_dynamics_solve(self._h, int(integrator), _dp(Z), capi.SOLVE_ADJOINT if adjoint else capi.SOLVE_FORWARD,
                                                 _dp(B), n_cols, capi.ROLLOUT_ALL if all_knots else capi.ROLLOUT_FINAL, _dp(Y)))
        return Y

    def rollout_gradient(self, Z, C, integrator=0):
        """Gradient of a loss phi of the ROLLED-OUT states of integrator ``integrator`` (``rollout(Z)``: start state = knot 1 of Z)
        with respect to everything but that integrator's states: controls, timesteps, times.  ``C``: (N, x_dim), row k the
        derivative of phi with respect to the rolled-out state of knot k + 1.  One adjoint solve L = M'^{-1} C, then -J' w with
        L_2 .. L_N in the integrator's rows of a zero w; the integrator's state components of the result are set to zero.  J' w is
        taken at Z with the ROLLED-OUT states in the integrator's components (d(E_k x_k)/du acts on the state the loss saw, whatever
        states Z holds): they come from a forward solve with B = [x_1; 0; ...], the rollout's bits, which also leaves the tree for
        the adjoint solve.  Host vectors; returns (n_variables,)."""
        Z = self._Z(Z)
        N, dim = self.trajectory.N, self.trajectory.dim
        Cm = np.ascontiguousarray(C, dtype=np.float64)
        x_dim = self._integrator_dims[integrator]
        if Cm.shape != (N, x_dim):
            raise ValueError(f"C: ({N}, {x_dim}) expected, got {Cm.shape}")
        row0, x_off = self._integrator_row0[integrator], self._integrator_x_off[integrator]
        B = np.zeros((N, 1, x_dim))
        if x_off is not None:
            B[0, 0] = Z[x_off:x_off + x_dim]
        X = self.dynamics_solve(Z, B, integrator=integrator)[:, 0]
        lam = self.dynamics_solve(Z, Cm.reshape(N, 1, x_dim), integrator=integrator, adjoint=True)[:, 0]
        Zr = Z.copy()
        Zr[:N * dim].reshape(N, dim)[:, x_off:x_off + x_dim] = X
        w = np.zeros(self.n_constraints)
        w[row0:row0 + (N - 1) * x_dim] = lam[1:].reshape(-1)
        y = np.full(self.n_variables, np.nan)
        self.eval_constraint_jacobian_transpose_product(y, Zr, w)
        grad = -y
        grad[:N * dim].reshape(N, dim)[:, x_off:x_off + x_dim] = 0.0
        return grad

    def dynamics_layout(self):
        """(n_states, n_levels, offset, level) of the whole-dynamics solves: D = the sum of the integrators' state dimensions, the
        number of dependency levels, and per integrator (list order) its offset on the D axis and its level -- 0 for an integrator
        that reads no other integrator's states, else 1 + the highest level among those it reads.  Needs no device."""
        n = len(self._integrator_dims)
        ns, nl = C.c_int32(), C.c_int32()
        off, lev = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        self._check(self._lib.dto_dynamics_layout(self._h, C.byref(ns), C.byref(nl), off.ctypes.data_as(capi.c_int32_p),
                                                  lev.ctypes.data_as(capi.c_int32_p)))
        return ns.value, nl.value, off[:n].copy(), lev[:n].copy()

    def _solve_all_shape(self, B):
        B = np.ascontiguousarray(B, dtype=np.float64)
        N, D = self.trajectory.N, sum(self._integrator_dims)
        if B.ndim == 2 and B.shape[0] == N:
            B = B.reshape(N, 1, B.shape[1])
        if B.ndim != 3 or B.shape[0] != N or B.shape[2] != D:
            raise ValueError(f"B: (N, n_cols, n_states) or (N, n_states) with N = {N}, n_states = {D} expected, got {B.shape}")
        return B

    def dynamics_solve_all(self, Z, B, adjoint=False):
        """Solve with the Jacobian block of ALL integrators' rows and ALL their state columns at Z (identity rows for knot 1 on top),
        on the device, by block elimination in dependency order.  Forward: the linearised rollout of the whole trajectory under
        fixed controls (B = -defect with zero knot-1 rows: the Newton state correction).  ``adjoint=True``: the costates of all
        dynamics rows; block 1 is the derivative with respect to the initial states.  ``B``: (N, n_cols, n_states), or
        (N, n_states) for one column, the last axis listing the integrators in list order (``dynamics_layout``).  Returns
        (N, n_cols, n_states).  A second call at the same Z, in either direction, launches no Jacobian, gather or tree kernel."""
        Z = self._Z(Z)
        B = self._solve_all_shape(B)
        Y = np.full(B.shape, np.nan)
        self._stage_external(Z, con_need=1)
        self._check(self._lib.dto_dynamics_solve_all(self._h, _dp(Z), capi.SOLVE_ADJOINT if adjoint else capi.SOLVE_FORWARD, _dp(B),
                                                     B.shape[1], _dp(Y)))
        return Y

    def feasible_trajectory(self, Z):
        """Z with every integrator's states replaced by what its dynamics reach from the states of knot 1 under the controls,
        timesteps and times of Z: levels ascending (``dynamics_layout``), a DerivativeIntegrator by its exact recurrence
        x_{k+1} = x_k + dt_k xdot_k, the others by ``rollout`` at the Z updated so far.  Host vectors; returns a copy."""
        Z = self._Z(Z).copy()
        N, dim = self.trajectory.N, self.trajectory.dim
        dt = self.trajectory.components[self.trajectory.timestep][0]
        Zk = Z[:N * dim].reshape(N, dim)
        _, n_levels, _, level = self.dynamics_layout()
        for lv in range(n_levels):
            for i, it in enumerate(self._integrator_list):
                if level[i] != lv:
                    continue
                if isinstance(it, DerivativeIntegrator):
                    for k in range(N - 1):
                        Zk[k + 1, it.x_off:it.x_off + it.x_dim] = (Zk[k, it.x_off:it.x_off + it.x_dim]
                                                                   + Zk[k, dt] * Zk[k, it.xdot_off:it.xdot_off + it.x_dim])
                else:
                    Zk[:, it.x_off:it.x_off + it.x_dim] = self.rollout(Z, integrator=i)[:, 0]
        return Z

    def feasible_trajectory_engine(self, Z):
        """``feasible_trajectory`` as ONE engine call (``dto_feasible_trajectory``): the levels, the DerivativeIntegrators'
        recurrences, one Jacobian evaluation per level that holds a propagator (not one per integrator), the rollouts and the
        scatter into the Z layout all run on the device.  Host vectors; returns a copy with the bits of ``feasible_trajectory``."""
        Z = self._Z(Z)
        Zf = np.full(self.n_variables, np.nan)
        self._stage_external(Z, con_need=1)
        self._check(self._lib.dto_feasible_trajectory(self._h, _dp(Z), _dp(Zf)))
        return Zf

    def feasible_merit(self, Z, sigma=1.0, mu=None, trajectory=False, constraints=False):
        """phi = sigma f(Zf) + sum over the non-dynamics rows of mu_r g_r(Zf) at Zf = ``feasible_trajectory_engine(Z)``, in one engine
        call (``dto_feasible_merit``): the function ``reduced_lagrangian_gradient`` and ``reduced_hessian_product`` are derivatives
        of, what a line search evaluates per trial step.  ``mu``: (n_constraints,) or None for zeros (phi = sigma f); its
        dynamics-row entries are not read.  The sum has a fixed order (include/dto_engine.h), so repeated calls return the same
        bits.  Returns phi; with ``trajectory=True`` and / or ``constraints=True`` a tuple (phi[, Zf][, g]): Zf (n_variables,) and g
        (n_constraints,), every row at Zf -- the dynamics rows are the defects the rollout leaves.  It keeps the points of the
        reduced operators: a line search between two ``reduced_hessian_product`` calls costs them nothing."""
        Z = self._Z(Z)
        if mu is not None:
            mu = _in(mu, self.n_constraints, "mu")
        phi = C.c_double(np.nan)
        Zf = np.full(self.n_variables, np.nan) if trajectory else None
        g = np.full(self.n_constraints, np.nan) if constraints else None
        self._check(self._lib.dto_feasible_merit(self._h, _dp(Z), float(sigma), None if mu is None else _dp(mu), C.byref(phi),
                                                 None if Zf is None else _dp(Zf), None if g is None else _dp(g)))
        out = (phi.value,) + (() if Zf is None else (Zf,)) + (() if g is None else (g,))
        return out if len(out) > 1 else phi.value

    def reduced_gradient(self, Z):
        """Gradient of the objective along the dynamically feasible manifold at a FEASIBLE Z (``feasible_trajectory``'s result):
        the derivative of f(feasible_trajectory(.)) with respect to everything the states of knots 2 .. N are a function of.  One
        objective gradient, one adjoint whole-dynamics solve L = MM'^{-1} df/ds, one J' w with L_2 .. L_N in the dynamics rows of a
        zero w.  Entries of controls, timesteps, times and globals: df/dc - (J' w)_c; state entries of knot 1: L_1; the other state
        entries: 0.  Host vectors; returns (n_variables,)."""
        Z = self._Z(Z)
        N, dim = self.trajectory.N, self.trajectory.dim
        D, _, offset, _ = self.dynamics_layout()
        g = np.full(self.n_variables, np.nan)
        self.eval_objective_gradient(g, Z)
        gk = g[:N * dim].reshape(N, dim)
        B = np.zeros((N, 1, D))
        for i, it in enumerate(self._integrator_list):
            B[:, 0, offset[i]:offset[i] + it.x_dim] = gk[:, it.x_off:it.x_off + it.x_dim]
        lam = self.dynamics_solve_all(Z, B, adjoint=True)[:, 0]
        w = np.zeros(self.n_constraints)
        for i, it in enumerate(self._integrator_list):
            row0 = self._integrator_row0[i]
            w[row0:row0 + (N - 1) * it.x_dim] = lam[1:, offset[i]:offset[i] + it.x_dim].reshape(-1)
        y = np.full(self.n_variables, np.nan)
        self.eval_constraint_jacobian_transpose_product(y, Z, w)
        grad = g - y
        rk = grad[:N * dim].reshape(N, dim)
        for i, it in enumerate(self._integrator_list):
            rk[:, it.x_off:it.x_off + it.x_dim] = 0.0
            rk[0, it.x_off:it.x_off + it.x_dim] = lam[0, offset[i]:offset[i] + it.x_dim]
        return grad

    def reduced_lagrangian_gradient(self, Z, sigma=1.0, mu=None, costates=False):
        """Reduced-space gradient on the device (``dto_reduced_gradient``): with the states of knots 2 .. N (the set S) eliminated by
        the dynamics, the gradient of phi = sigma f + sum over the non-dynamics rows of mu_r g_r.  g = sigma grad f + J' w1 (w1 = mu
        with its dynamics rows zeroed; ``mu=None``: zeros, the product is skipped), MM' Lam = g_S, t = J' w2 (Lam_2 .. Lam_N in the
        dynamics rows).  Returns (n_variables,): g - t on controls, timesteps, times and globals, Lam_1 on the states of knot 1, 0 on
        S; with ``costates=True`` also Lam as (N, n_states) (``dynamics_layout``).  With sigma = 1 and mu = None the bits of
        ``reduced_gradient``.  The point -- costates, multipliers, gradient -- is kept per (Z, sigma, mu) for
        ``reduced_hessian_product``; a repeated call copies the kept result."""
        Z = self._Z(Z)
        if mu is not None:
            mu = _in(mu, self.n_constraints, "mu")
        grad = np.full(self.n_variables, np.nan)
        lam = np.full((self.trajectory.N, sum(self._integrator_dims)), np.nan) if costates else None
        self._check(self._lib.dto_reduced_gradient(self._h, _dp(Z), float(sigma), None if mu is None else _dp(mu), _dp(grad),
                                                   None if lam is None else _dp(lam)))
        return (grad, lam) if costates else grad

    def reduced_hessian_product(self, Z, v, sigma=1.0, mu=None):
        """y = T' H(Z; sigma, mu~) T v on the device (``dto_reduced_hessian_product``): the Hessian-vector product of the reduced
        problem, T the tangent map of the feasible manifold and mu~ = mu on the non-dynamics rows, minus the costates of
        ``reduced_lagrangian_gradient`` on the dynamics rows.  ``v``: (n_variables,), its entries at the states of knots 2 .. N are
        not read.  Returns (n_variables,), zero at those entries.  At a dynamically feasible Z (``feasible_trajectory``) this is the
        Hessian of phi(feasible_trajectory(.)); symmetric at any Z.  Products at the (Z, sigma, mu) of the last call run one J w, one
        J' w, two whole-dynamics scans and one H v: no Jacobian chain, tree build or Hessian assembly."""
        Z = self._Z(Z)
        v = _in(v, self.n_variables, "v")
        if mu is not None:
            mu = _in(mu, self.n_constraints, "mu")
        y = np.full(self.n_variables, np.nan)
        self._check(self._lib.dto_reduced_hessian_product(self._h, _dp(Z), float(sigma), None if mu is None else _dp(mu), _dp(v), _dp(y)))
        return y

    def reduced_hessian_products(self, Z, V, sigma=1.0, mu=None):
        """Y[c] = T' H(Z; sigma, mu~) T V[c] for every row of V on the device (``dto_projected_hessian_products``): ``V`` is
        (n_cols, n_variables), its entries at the states of knots 2 .. N are not read; returns (n_cols, n_variables), zero at those
        entries.  Bit for bit ``reduced_hessian_product`` of every row with the same ``reduced_input_store`` setting, at the same
        kept points.  The columns run in chunks (``reduced_block_width``; at most the column limit of ``dynamics_solve_all``): per
        chunk the solves' node matrices, the input blocks and the Hessian copy are read once, not once per vector.  With
        ``reduced_input_store`` = 0, J v^ and J' w still run once per column."""
        Z = self._Z(Z)
        V = self._columns(V, self.n_variables, "V")
        if mu is not None:
            mu = _in(mu, self.n_constraints, "mu")
        Y = np.full(V.shape, np.nan)
        self._check(self._lib.dto_projected_hessian_products(self._h, _dp(Z), float(sigma), None if mu is None else _dp(mu), V.shape[0],
                                                             _dp(V), _dp(Y)))
        return Y

    def reduced_newton_step(self, Z, sigma=1.0, mu=None, free=None, radius=0.0, shift=0.0, rtol=1e-6, atol=0.0, max_iter=50, trace=False):
        """The truncated-Newton step of the reduced problem in ONE engine call (``dto_projected_newton_step``): Steihaug-Toint CG on
        (M T'HT M + shift M) p = -M g from p = 0, g the ``reduced_lagrangian_gradient`` and T'HT the ``reduced_hessian_product`` at
        (Z, sigma, mu), M zeroing the states of knots 2 .. N and the entries whose ``free`` value is 0.0 (``free``: (n_variables,) or
        None for all free).  ``radius`` > 0 is a trust region (0: none); the iteration stops at ``sqrt(r.r) <= max(atol, rtol ||g||)``,
        at the boundary, at non-positive curvature or after ``max_iter`` products.  The kept points are checked once, every dot has
        a fixed order and every decision is made on the device (include/dto_engine.h, "Truncated-Newton step"): the same loop written
        in NumPy around ``reduced_hessian_product`` gives the same bits.  Returns (p, info) -- p (n_variables,), info a dict with
        ``status`` (``capi.NEWTON_*``), ``iterations``, ``gnorm``, ``rnorm``, ``pnorm``, ``pg`` = p.g, ``predicted`` = -(g'p + p'Ap / 2),
        ``curvature`` (the last d'Ad / d'd) and ``raw`` (the eight doubles) -- and with ``trace=True`` also (iterations, 4): kappa,
        d.d, the step along d and r.r behind it, per iteration."""
        Z = self._Z(Z)
        if mu is not None:
            mu = _in(mu, self.n_constraints, "mu")
        if free is not None:
            free = _in(free, self.n_variables, "free")
        max_iter = int(max_iter)
        p = np.full(self.n_variables, np.nan)
        raw = np.full(8, np.nan)
        tr = np.full((max(max_iter, 0), 4), np.nan) if trace else None
        self._check(self._lib.dto_projected_newton_step(self._h, _dp(Z), float(sigma), None if mu is None else _dp(mu),
                                                        None if free is None else _dp(free), float(radius), float(shift), float(rtol),
                                                        float(atol), max_iter, _dp(p), _dp(raw), None if tr is None else _dp(tr)))
        info = dict(status=int(raw[0]), iterations=int(raw[1]), gnorm=raw[2], rnorm=raw[3], pnorm=raw[4], pg=raw[5], predicted=raw[6],
                    curvature=raw[7], raw=raw)
        return (p, info, tr[:info["iterations"]]) if trace else (p, info)

    def reduced_newton_step_box(self, Z, sigma=1.0, mu=None, lo=None, hi=None, free=None, radius=0.0, shift=0.0, rtol=1e-6, atol=0.0,
                                max_iter=50, trace=False, states=False, trajectory=False):
        """``reduced_newton_step`` with simple bounds ``lo <= Z + p <= hi`` on the independent entries, in ONE engine call
        (``dto_projected_newton_step_box``).  ``lo``, ``hi``: (n_variables,) or None for none (``Problem.bounds_vectors`` expands
        per-component bounds); their values at the states of knots 2 .. N and at masked entries are not read.  An entry on a bound whose
        gradient points outward is held from the start; a step that would leave the box stops at the face, the entries that reached it
        are fixed there and the solve restarts on the face; a direction of non-positive curvature is followed to the face
        (include/dto_engine.h, "Bound-constrained truncated-Newton step": the same loop written in NumPy around
        ``reduced_hessian_product`` gives the same bits, and without bounds the bits of ``reduced_newton_step``).  Returns (p, info
        [, trace][, states][, Zp]): info as ``reduced_newton_step``'s with ``held``, ``hit``, ``restarts``, ``n_free`` and ``raw`` (twelve
        doubles); ``trace=True`` adds (iterations, 6): kappa, d.d, s, r.r over the free set, tau_box, entries hit; ``states=True`` the
        codes ``capi.BOX_*`` per entry as doubles (usable as the next call's ``free``); ``trajectory=True`` Zp = Z + p with the entries
        that hit a bound holding it exactly -- the point to give ``feasible_merit`` next."""
        Z = self._Z(Z)
        if mu is not None:
            mu = _in(mu, self.n_constraints, "mu")
        if free is not None:
            free = _in(free, self.n_variables, "free")
        if lo is not None:
            lo = _in(lo, self.n_variables, "lo")
        if hi is not None:
            hi = _in(hi, self.n_variables, "hi")
        max_iter = int(max_iter)
        opt = lambda a: None if a is None else _dp(a)
        p = np.full(self.n_variables, np.nan)
        raw = np.full(12, np.nan)
        tr = np.full((max(max_iter, 0), 6), np.nan) if trace else None
        es = np.full(self.n_variables, np.nan) if states else None
        zp = np.full(self.n_variables, np.nan) if trajectory else None
        self._check(self._lib.dto_projected_newton_step_box(self._h, _dp(Z), float(sigma), opt(mu), opt(free), opt(lo), opt(hi), float(radius),
                                                            float(shift), float(rtol), float(atol), max_iter, _dp(p), _dp(raw), opt(tr),
                                                            opt(es), opt(zp)))
        info = dict(status=int(raw[0]), iterations=int(raw[1]), gnorm=raw[2], rnorm=raw[3], pnorm=raw[4], pg=raw[5], predicted=raw[6],
                    curvature=raw[7], held=int(raw[8]), hit=int(raw[9]), restarts=int(raw[10]), n_free=int(raw[11]), raw=raw)
        out = (p, info)
        if trace:
            out += (tr[:info["iterations"]],)
        if states:
            out += (es,)
        if trajectory:
            out += (zp,)
        return out

    # ---- augmented-Lagrangian terms (include/dto_engine.h, "Augmented-Lagrangian terms"): the calls above with a penalty rho_r on the
    # non-dynamics rows.  ``rho``: (n_constraints,) or None for no penalties (the call is then the one it extends, bit for bit and
    # launch for launch); ``Problem.penalty_vector`` expands a value per constraint over the rows.
    def _mu_rho(self, mu, rho):
        mu = None if mu is None else _in(mu, self.n_constraints, "mu")
        rho = None if rho is None else _in(rho, self.n_constraints, "rho")
        return mu, rho

    @staticmethod
    def _al_info(raw):
        return dict(P=raw[0], active=int(raw[1]), max_viol=raw[2], sum_viol2=raw[3], max_dmult=raw[4], penalised=int(raw[5]), raw=raw)

    def auglag_rows(self, Z, mu=None, rho=None):
        """The row pass at Z (``dto_auglag_rows``): per non-dynamics row the Powell-Hestenes-Rockafellar multiplier
        ``mult = mu + rho g`` (0 on an inactive inequality row, ``mu`` where ``rho`` is 0) and weight (``rho`` on active rows).
        Returns (mu_eff, weight, info): (n_constraints,) each with zeros in the dynamics rows -- ``mu_eff`` is the first-order
        multiplier update -- and info a dict with ``P`` (the sum of the rows' terms psi), ``active``, ``max_viol``, ``sum_viol2``,
        ``max_dmult``, ``penalised`` and ``raw`` (eight doubles)."""
        Z = self._Z(Z)
        mu, rho = self._mu_rho(mu, rho)
        opt = lambda a: None if a is None else _dp(a)
        mu_eff = np.full(self.n_constraints, np.nan)
        weight = np.full(self.n_constraints, np.nan)
        raw = np.full(8, np.nan)
        self._check(self._lib.dto_auglag_rows(self._h, _dp(Z), opt(mu), opt(rho), _dp(mu_eff), _dp(weight), _dp(raw)))
        return mu_eff, weight, self._al_info(raw)

    def auglag_merit(self, Z, sigma=1.0, mu=None, rho=None, trajectory=False, constraints=False, info=False):
        """Phi = sigma f(Zf) + sum over the non-dynamics rows of psi_r(g_r(Zf)) at the feasible trajectory Zf of Z
        (``dto_auglag_merit``): ``feasible_merit`` with the rows' augmented-Lagrangian terms.  Returns Phi, or a tuple
        (Phi[, Zf][, g][, info]); ``info`` as ``auglag_rows`` returns it (with ``rho=None`` its values are NaN: no row pass runs)."""
        Z = self._Z(Z)
        mu, rho = self._mu_rho(mu, rho)
        opt = lambda a: None if a is None else _dp(a)
        phi = C.c_double(np.nan)
        Zf = np.full(self.n_variables, np.nan) if trajectory else None
        g = np.full(self.n_constraints, np.nan) if constraints else None
        raw = np.full(8, np.nan) if info else None
        self._check(self._lib.dto_auglag_merit(self._h, _dp(Z), float(sigma), opt(mu), opt(rho), C.byref(phi), opt(Zf), opt(g), opt(raw)))
        out = (phi.value,) + (() if Zf is None else (Zf,)) + (() if g is None else (g,)) + (() if raw is None else (self._al_info(raw),))
        return out if len(out) > 1 else phi.value

    def auglag_gradient(self, Z, sigma=1.0, mu=None, rho=None, costates=False, multipliers=False):
        """The reduced gradient of Phi (``dto_auglag_gradient``): ``reduced_lagrangian_gradient`` at ``mu_eff``, bit for bit.
        Returns grad, or (grad[, Lam][, mu_eff])."""
        Z = self._Z(Z)
        mu, rho = self._mu_rho(mu, rho)
        opt = lambda a: None if a is None else _dp(a)
        grad = np.full(self.n_variables, np.nan)
        lam = np.full((self.trajectory.N, sum(self._integrator_dims)), np.nan) if costates else None
        mu_eff = np.full(self.n_constraints, np.nan) if multipliers else None
        self._check(self._lib.dto_auglag_gradient(self._h, _dp(Z), float(sigma), opt(mu), opt(rho), _dp(grad), opt(lam), opt(mu_eff)))
        out = (grad,) + (() if lam is None else (lam,)) + (() if mu_eff is None else (mu_eff,))
        return out if len(out) > 1 else grad

    def auglag_hessian_products(self, Z, V, sigma=1.0, mu=None, rho=None):
        """Y[c] = T'(H(Z; sigma, mu~_eff) + J_c' W J_c) T V[c] (``dto_auglag_hessian_products``): ``reduced_hessian_products`` at
        ``mu_eff`` with the Gauss-Newton term of the penalised rows, W = diag(weight).  Every row has the bits of the call with that
        row alone."""
        Z = self._Z(Z)
        V = self._columns(V, self.n_variables, "V")
        mu, rho = self._mu_rho(mu, rho)
        opt = lambda a: None if a is None else _dp(a)
        Y = np.full(V.shape, np.nan)
        self._check(self._lib.dto_auglag_hessian_products(self._h, _dp(Z), float(sigma), opt(mu), opt(rho), V.shape[0], _dp(V), _dp(Y)))
        return Y

    def auglag_hessian_product(self, Z, v, sigma=1.0, mu=None, rho=None):
        """``auglag_hessian_products`` of one vector; returns (n_variables,)."""
        return self.auglag_hessian_products(Z, _in(v, self.n_variables, "v")[None, :], sigma, mu, rho)[0]

    def auglag_newton_step(self, Z, sigma=1.0, mu=None, rho=None, lo=None, hi=None, free=None, radius=0.0, shift=0.0, rtol=1e-6, atol=0.0,
                           max_iter=50, trace=False, states=False, trajectory=False):
        """``reduced_newton_step_box`` on the augmented Lagrangian (``dto_auglag_newton_step``): the gradient is ``auglag_gradient``,
        the operator ``auglag_hessian_product``; arguments and results as there."""
        Z = self._Z(Z)
        mu, rho = self._mu_rho(mu, rho)
        if free is not None:
            free = _in(free, self.n_variables, "free")
        if lo is not None:
            lo = _in(lo, self.n_variables, "lo")
        if hi is not None:
            hi = _in(hi, self.n_variables, "hi")
        max_iter = int(max_iter)
        opt = lambda a: None if a is None else _dp(a)
        p = np.full(self.n_variables, np.nan)
        raw = np.full(12, np.nan)
        tr = np.full((max(max_iter, 0), 6), np.nan) if trace else None
        es = np.full(self.n_variables, np.nan) if states else None
        zp = np.full(self.n_variables, np.nan) if trajectory else None
        self._check(self._lib.dto_auglag_newton_step(self._h, _dp(Z), float(sigma), opt(mu), opt(rho), opt(free), opt(lo), opt(hi),
                                                     float(radius), float(shift), float(rtol), float(atol), max_iter, _dp(p), _dp(raw),
                                                     opt(tr), opt(es), opt(zp)))
        info = dict(status=int(raw[0]), iterations=int(raw[1]), gnorm=raw[2], rnorm=raw[3], pnorm=raw[4], pg=raw[5], predicted=raw[6],
                    curvature=raw[7], held=int(raw[8]), hit=int(raw[9]), restarts=int(raw[10]), n_free=int(raw[11]), raw=raw)
        out = (p, info)
        if trace:
            out += (tr[:info["iterations"]],)
        if states:
            out += (es,)
        if trajectory:
            out += (zp,)
        return out

    # ---- L-BFGS preconditioner of the truncated-Newton step (include/dto_engine.h, "Preconditioned truncated-Newton step")
    def newton_pairs_push(self, s, y):
        """Append one pair (s, y), (n_variables,) each and finite, to the pair store (``dto_newton_pairs_push``); the oldest pair drops
        at capacity.  The capacity is the option ``newton_pairs`` (``set_option("newton_pairs", m)``, 0 .. 16, default 0 = off)."""
        s, y = _in(s, self.n_variables, "s"), _in(y, self.n_variables, "y")
        self._check(self._lib.dto_newton_pairs_push(self._h, _dp(s), _dp(y)))

    def newton_pairs_clear(self):
        """Empty the pair store (``dto_newton_pairs_clear``); the capacity stays."""
        self._check(self._lib.dto_newton_pairs_clear(self._h))

    def newton_pairs_info(self):
        """(count, capacity) of the pair store (``dto_newton_pairs_info``)."""
        a, b = C.c_int32(), C.c_int32()
        self._check(self._lib.dto_newton_pairs_info(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def newton_precondition(self, r, free=None):
        """z = P H P r with the store's pairs (``dto_newton_precondition``): the compact L-BFGS inverse restricted to the independent
        entries that ``free`` (None: all) leaves, zero elsewhere.  r (n_variables,) or (n_cols, n_variables); z has r's shape, and
        every row has the bits of the call with that row alone.  With an empty store, or no admitted pair, z = r on those entries."""
        r = np.asarray(r, dtype=np.float64)
        single = r.ndim == 1
        r = self._columns(r[None, :] if single else r, self.n_variables, "r")
        if free is not None:
            free = _in(free, self.n_variables, "free")
        z = np.full(r.shape, np.nan)
        self._check(self._lib.dto_newton_precondition(self._h, None if free is None else _dp(free), r.shape[0], _dp(r), _dp(z)))
        return z[0] if single else z

    def preconditioned_newton_step(self, Z, sigma=1.0, mu=None, rho=None, lo=None, hi=None, free=None, radius=0.0, shift=0.0, rtol=1e-6,
                                   atol=0.0, max_iter=50, harvest=False, trace=False, states=False, trajectory=False):
        """``auglag_newton_step`` (``rho=None``: ``reduced_newton_step_box``) preconditioned with the L-BFGS inverse of the pair store
        (``dto_preconditioned_newton_step``).  ``harvest=True`` keeps the CG pairs (d, A d) of this call -- the last ``newton_pairs`` of
        them -- as the store of the next call.  Arguments and results as there; info also has ``admitted``, ``harvested``,
        ``fallbacks`` and ``rz0``, raw has 16 entries and the trace 8 columns (the box step's, rz, preconditioner on / off).  With an
        empty store the step is the unpreconditioned one bit for bit."""
        Z = self._Z(Z)
        mu, rho = self._mu_rho(mu, rho)
        if free is not None:
            free = _in(free, self.n_variables, "free")
        if lo is not None:
            lo = _in(lo, self.n_variables, "lo")
        if hi is not None:
            hi = _in(hi, self.n_variables, "hi")
        max_iter = int(max_iter)
        opt = lambda a: None if a is None else _dp(a)
        p = np.full(self.n_variables, np.nan)
        raw = np.full(16, np.nan)
        tr = np.full((max(max_iter, 0), 8), np.nan) if trace else None
        es = np.full(self.n_variables, np.nan) if states else None
        zp = np.full(self.n_variables, np.nan) if trajectory else None
        self._check(self._lib.dto_preconditioned_newton_step(self._h, _dp(Z), float(sigma), opt(mu), opt(rho), opt(free), opt(lo), opt(hi),
                                                             float(radius), float(shift), float(rtol), float(atol), max_iter, int(bool(harvest)),
                                                             _dp(p), _dp(raw), opt(tr), opt(es), opt(zp)))
        info = dict(status=int(raw[0]), iterations=int(raw[1]), gnorm=raw[2], rnorm=raw[3], pnorm=raw[4], pg=raw[5], predicted=raw[6],
                    curvature=raw[7], held=int(raw[8]), hit=int(raw[9]), restarts=int(raw[10]), n_free=int(raw[11]), admitted=int(raw[12]),
                    harvested=int(raw[13]), fallbacks=int(raw[14]), rz0=raw[15], raw=raw)
        out = (p, info)
        if trace:
            out += (tr[:info["iterations"]],)
        if states:
            out += (es,)
        if trajectory:
            out += (zp,)
        return out

    # ---- reduced-space minimize (include/dto_engine.h, "Reduced-space minimize")
    @staticmethod
    def _minimize_options(options):
        unknown = sorted(set(options) - set(capi.MINIMIZE_OPTIONS))
        if unknown:
            raise TypeError(f"reduced_minimize: unknown option(s) {unknown}; the options are {list(capi.MINIMIZE_OPTIONS)}")
        return np.array([float(options.get(k, d)) for k, d in zip(capi.MINIMIZE_OPTIONS, capi.MINIMIZE_DEFAULTS)], dtype=np.float64)

    @staticmethod
    def _minimize_info(raw):
        return dict(status=int(raw[0]), outer=int(raw[1]), trials=int(raw[2]), accepted=int(raw[3]), phi_first=raw[4], phi=raw[5], delta=raw[6],
                    gnorm=raw[7], max_viol_first=raw[8], max_viol=raw[9], grew=int(raw[10]), iterations=int(raw[11]), harvested=int(raw[12]),
                    fallbacks=int(raw[13]), raw=raw)

    def reduced_minimize(self, Z, sigma=1.0, mu=None, rho=None, lo=None, hi=None, free=None, outer=1, trials=10, harvest=False, history=False,
                         states=False, **options):
        """The trust-region loop around the step and the merit -- and with ``rho`` the outer multiplier / penalty loop around it -- as
        one device-resident call (``dto_projected_minimize``): the README's loops with the rules of csrc/dto_minimize_plan.h.  The step is
        ``preconditioned_newton_step`` where the option ``newton_pairs`` is above 0, else ``auglag_newton_step``; the merit is
        ``auglag_merit``, the row pass ``auglag_rows``.  The inputs are copied.  ``options``: ``radius0``, ``eta_accept``,
        ``eta_shrink``, ``eta_grow``, ``shrink_div``, ``grow_mul``, ``radius_max``, ``radius_min``, ``gtol``, ``ctol``, ``viol_div``,
        ``rho_mul`` and the step's ``shift``, ``rtol``, ``atol``, ``max_iter`` (defaults: ``capi.MINIMIZE_DEFAULTS``).
        Returns (Z, info[, mu, rho][, history, outer_history][, states]): mu and rho where ``rho`` is given; info a dict with
        ``status`` (``capi.MINIMIZE_*``), ``outer``, ``trials``, ``accepted``, ``phi_first``, ``phi``, ``delta``, ``gnorm``,
        ``max_viol_first``, ``max_viol``, ``grew``, ``iterations`` (the steps' CG iterations, summed), ``harvested``, ``fallbacks`` and
        ``raw``; history (trials run, 8): ratio, accepted, delta, phi_t, predicted, the step's status, iterations, ||g||;
        outer_history (outer iterations run, 4): max viol, grew, active rows, P; states: the last step's entry states."""
        Z = np.array(self._Z(Z), dtype=np.float64)
        mu, rho = self._mu_rho(mu, rho)
        mu = None if mu is None else np.array(mu, dtype=np.float64)
        rho = None if rho is None else np.array(rho, dtype=np.float64)
        if free is not None:
            free = _in(free, self.n_variables, "free")
        if lo is not None:
            lo = _in(lo, self.n_variables, "lo")
        if hi is not None:
            hi = _in(hi, self.n_variables, "hi")
        outer, trials = int(outer), int(trials)
        opts = self._minimize_options(options)
        opt = lambda a: None if a is None else _dp(a)
        raw = np.full(16, np.nan)
        hist = np.full((max(outer, 0) * max(trials, 0), 8), np.nan) if history else None
        ohist = np.full((max(outer, 0), 4), np.nan) if history else None
        es = np.full(self.n_variables, np.nan) if states else None
        self._check(self._lib.dto_projected_minimize(self._h, _dp(Z), float(sigma), opt(mu), opt(rho), opt(free), opt(lo), opt(hi), _dp(opts), outer,
                                                   trials, int(bool(harvest)), _dp(raw), opt(hist), opt(ohist), opt(es)))
        info = self._minimize_info(raw)
        out = (Z, info)
        if rho is not None:
            out += (mu, rho)
        if history:
            passes = 0 if rho is None else info["outer"] - (info["status"] == capi.MINIMIZE_NOT_FINITE)   # NOT_FINITE: no row pass behind it
            out += (hist[:info["trials"]], ohist[:passes])
        if states:
            out += (es,)
        return out

    def independent_entries(self):
        """C: the entries of Z that are no state of a knot 2 .. N (controls, timesteps, times, the states of knot 1, globals),
        ascending, 0-based -- the variables of the reduced problem."""
        N, dim = self.trajectory.N, self.trajectory.dim
        free = np.ones(self.n_variables, dtype=bool)
        fk = free[:N * dim].reshape(N, dim)
        for it in self._integrator_list:
            fk[1:, it.x_off:it.x_off + it.x_dim] = False
        return np.flatnonzero(free)

    def reduced_hessian_matrix(self, Z, sigma=1.0, mu=None, block=64):
        """The dense reduced Hessian T' H(Z; sigma, mu~) T on the independent entries: returns (Hr, C), Hr (|C|, |C|) and C =
        ``independent_entries()``; column i of Hr is the product with the unit vector of entry C[i], ``block`` unit vectors per
        ``reduced_hessian_products`` call.  For control spaces of a few hundred entries (a direct Newton step, a preconditioner)."""
        Cidx = self.independent_entries()
        nC = Cidx.size
        Hr = np.empty((nC, nC))
        for i0 in range(0, nC, block):
            i1 = min(nC, i0 + block)
            V = np.zeros((i1 - i0, self.n_variables))
            V[np.arange(i1 - i0), Cidx[i0:i1]] = 1.0
            Hr[:, i0:i1] = self.reduced_hessian_products(Z, V, sigma, mu)[:, Cidx].T
        return Hr, Cidx

    def constraint_bounds(self):  # get_nonlinear_constraints, src/solvers/solve.jl:30-65
        lo = np.empty(self.n_constraints)
        hi = np.empty(self.n_constraints)
        self._check(self._lib.dto_constraint_bounds(self._h, _dp(lo), _dp(hi)))
        return lo, hi

    def shard_rows(self):
        n = self.shard.n_row_segments
        s = np.empty(n, dtype=np.int64)
        ln = np.empty(n, dtype=np.int64)
        self._check(self._lib.dto_shard_rows(self._h, _ip(s), _ip(ln)))
        return s, ln

    # ---- device-resident forms (pointers are integers, e.g. torch.Tensor.data_ptr())
    # (closure-based terms are evaluated on the host: pass the host copy of Z -- and of mu -- as well)
    def eval_objective_dev(self, dZ, df, stream=0, Z_host=None):
        self._stage_external(Z_host, obj_need=0)
        self._check(self._lib.dto_eval_objective_dev(self._h, dZ, df, stream))

    def eval_gradient_dev(self, dZ, dgrad, stream=0, Z_host=None):
        self._stage_external(Z_host, obj_need=1)
        self._check(self._lib.dto_eval_gradient_dev(self._h, dZ, dgrad, stream))

    def eval_constraint_dev(self, dZ, dg, stream=0, Z_host=None):
        self._stage_external(Z_host, con_need=0)
        self._check(self._lib.dto_eval_constraint_dev(self._h, dZ, dg, stream))

    def eval_jacobian_dev(self, dZ, dvals, stream=0, Z_host=None):
        self._stage_external(Z_host, con_need=1)
        self._check(self._lib.dto_eval_jacobian_dev(self._h, dZ, dvals, stream))

    def eval_hessian_dev(self, dZ, sigma, dmu, dvals, stream=0, Z_host=None, mu_host=None):
        self._stage_external(Z_host, con_need=2, obj_need=2 if sigma != 0.0 else -1, mu=mu_host)
        self._check(self._lib.dto_eval_hessian_dev(self._h, dZ, float(sigma), dmu, dvals, stream))

    def eval_hessian_product_dev(self, dZ, sigma, dmu, dv, dy, stream=0, Z_host=None, mu_host=None):
        self._stage_external(Z_host, con_need=2, obj_need=2 if sigma != 0.0 else -1, mu=mu_host)
        self._check(self._lib.dto_eval_hessian_product_dev(self._h, dZ, float(sigma), dmu, dv, dy, stream))

    def eval_hessian_products_dev(self, dZ, sigma, dmu, n_cols, dV, dY, stream=0, Z_host=None, mu_host=None):
        """``eval_hessian_lagrangian_products`` on device pointers: dV and dY (n_cols, n_variables), not overlapping; enqueued on
        `stream`, errors deferred as for every `_dev` call.  Same bits as the host form."""
        self._stage_external(Z_host, con_need=2, obj_need=2 if sigma != 0.0 else -1, mu=mu_host)
        self._check(self._lib.dto_eval_hessian_products_dev(self._h, dZ, float(sigma), dmu or None, int(n_cols), dV or None, dY or None, stream))

    def eval_jacobian_product_dev(self, dZ, dw, dy, stream=0, Z_host=None):  # y = J w, dw [n_variables], dy [n_constraints]
        self._stage_external(Z_host, con_need=1)
        self._check(self._lib.dto_eval_jacobian_product_dev(self._h, dZ, dw, dy, stream))

    def eval_jacobian_transpose_product_dev(self, dZ, dw, dy, stream=0, Z_host=None):  # y = J' w, dw [n_constraints], dy [n_variables]
        self._stage_external(Z_host, con_need=1)
        self._check(self._lib.dto_eval_jacobian_transpose_product_dev(self._h, dZ, dw, dy, stream))

    def rollout_dev(self, dZ, dX0, n_cols, dX, integrator=0, all_knots=True, stream=0, Z_host=None):
        """``rollout`` on device pointers: dX0 (n_cols, x_dim) or 0 / None (the state of knot 1 of dZ, n_cols = 1), dX
        (N, n_cols, x_dim) or, with ``all_knots=False``, (n_cols, x_dim); enqueued on `stream`, errors deferred as for every `_dev`
        call.  Same bits as ``rollout``."""
        self._stage_external(Z_host, con_need=1)
        self._check(self._lib.dto_rollout_dev(self._h, int(integrator), dZ, dX0 or None, int(n_cols),
                                              capi.ROLLOUT_ALL if all_knots else capi.ROLLOUT_FINAL, dX, stream))

    def dynamics_solve_dev(self, dZ, dB, n_cols, dY, integrator=0, adjoint=False, all_knots=True, stream=0, Z_host=None):
        """``dynamics_solve`` on device pointers: dB (N, n_cols, x_dim), dY (N, n_cols, x_dim) or, with ``all_knots=False``,
        (n_cols, x_dim); enqueued on `stream`, errors deferred as for every `_dev` call.  Same bits as ``dynamics_solve``."""
        self._stage_external(Z_host, con_need=1)
        self._check(self._lib.dto_dynamics_solve_dev(self._h, int(integrator), dZ, capi.SOLVE_ADJOINT if adjoint else capi.SOLVE_FORWARD,
                                                     dB or None, int(n_cols), capi.ROLLOUT_ALL if all_knots else capi.ROLLOUT_FINAL, dY, stream))

    def dynamics_solve_all_dev(self, dZ, dB, n_cols, dY, adjoint=False, stream=0, Z_host=None):
        """``dynamics_solve_all`` on device pointers: dB and dY (N, n_cols, n_states), not overlapping; enqueued on `stream`, errors
        deferred as for every `_dev` call.  Same bits as ``dynamics_solve_all``."""
        self._stage_external(Z_host, con_need=1)
        self._check(self._lib.dto_dynamics_solve_all_dev(self._h, dZ, capi.SOLVE_ADJOINT if adjoint else capi.SOLVE_FORWARD, dB or None,
                                                         int(n_cols), dY, stream))

    def feasible_trajectory_dev(self, dZ, dZf, stream=0, Z_host=None):
        """``feasible_trajectory_engine`` on device pointers: dZ and dZf (n_variables); dZf may equal dZ (in place), otherwise they
        must not overlap; enqueued on `stream`, errors deferred as for every `_dev` call.  Same bits as the host form."""
        self._stage_external(Z_host, con_need=1)
        self._check(self._lib.dto_feasible_trajectory_dev(self._h, dZ or None, dZf or None, stream))

    def feasible_merit_dev(self, dZ, sigma, dmu, dphi, dZf=0, dg=0, stream=0):
        """``feasible_merit`` on device pointers: dmu (n_constraints) or 0 / None for zeros, dphi one double, dZf (n_variables) and
        dg (n_constraints) or 0 / None; enqueued on `stream`, errors deferred as for every `_dev` call.  Same bits as the host
        form."""
        self._check(self._lib.dto_feasible_merit_dev(self._h, dZ or None, float(sigma), dmu or None, dphi or None, dZf or None,
                                                     dg or None, stream))

    def reduced_gradient_dev(self, dZ, sigma, dmu, dgrad, dlam=0, stream=0):
        """``reduced_lagrangian_gradient`` on device pointers: dmu (n_constraints) or 0 / None for zeros, dgrad (n_variables), dlam
        (N, n_states) or 0 / None; enqueued on `stream`, errors deferred as for every `_dev` call.  Same bits as the host form."""
        self._check(self._lib.dto_reduced_gradient_dev(self._h, dZ, float(sigma), dmu or None, dgrad or None, dlam or None, stream))

    def reduced_hessian_product_dev(self, dZ, sigma, dmu, dv, dy, stream=0):
        """``reduced_hessian_product`` on device pointers: dmu (n_constraints) or 0 / None for zeros, dv and dy (n_variables), not
        overlapping; enqueued on `stream`, errors deferred as for every `_dev` call.  Same bits as the host form."""
        self._check(self._lib.dto_reduced_hessian_product_dev(self._h, dZ, float(sigma), dmu or None, dv or None, dy or None, stream))

    def reduced_hessian_products_dev(self, dZ, sigma, dmu, n_cols, dV, dY, stream=0):
        """``reduced_hessian_products`` on device pointers: dmu (n_constraints) or 0 / None for zeros, dV and dY
        (n_cols, n_variables), not overlapping; enqueued on `stream`, errors deferred as for every `_dev` call.  Same bits as the host
        form."""
        self._check(self._lib.dto_projected_hessian_products_dev(self._h, dZ, float(sigma), dmu or None, int(n_cols), dV or None,
                                                                 dY or None, stream))

    def reduced_newton_step_dev(self, dZ, sigma, dmu, dfree, radius, shift, rtol, atol, max_iter, dp, dinfo, dtrace=0, stream=0):
        """``reduced_newton_step`` on device pointers: dmu (n_constraints), dfree (n_variables) and dtrace (max_iter, 4) or 0 / None,
        dp (n_variables), dinfo (8 doubles); works on `stream` and waits on one 16-byte readback per iteration, errors deferred as
        for every `_dev` call.  Same bits as the host form."""
        self._check(self._lib.dto_projected_newton_step_dev(self._h, dZ or None, float(sigma), dmu or None, dfree or None, float(radius),
                                                            float(shift), float(rtol), float(atol), int(max_iter), dp or None,
                                                            dinfo or None, dtrace or None, stream))

    def reduced_newton_step_box_dev(self, dZ, sigma, dmu, dfree, dlo, dhi, radius, shift, rtol, atol, max_iter, dp, dinfo, dtrace=0,
                                    dstates=0, dZp=0, stream=0):
        """``reduced_newton_step_box`` on device pointers: dmu (n_constraints), dfree, dlo, dhi, dstates and dZp (n_variables) and
        dtrace (max_iter, 6) or 0 / None, dp (n_variables), dinfo (12 doubles); works on `stream` and waits on one 16-byte readback
        per iteration, errors deferred as for every `_dev` call.  Same bits as the host form."""
        self._check(self._lib.dto_projected_newton_step_box_dev(self._h, dZ or None, float(sigma), dmu or None, dfree or None, dlo or None,
                                                                dhi or None, float(radius), float(shift), float(rtol), float(atol),
                                                                int(max_iter), dp or None, dinfo or None, dtrace or None, dstates or None,
                                                                dZp or None, stream))

    def auglag_rows_dev(self, dZ, dmu, drho, dmu_eff=0, dweight=0, dinfo=0, stream=0):
        """``auglag_rows`` on device pointers: dmu, drho, dmu_eff, dweight (n_constraints) and dinfo (8 doubles), any but dZ may be 0."""
        self._check(self._lib.dto_auglag_rows_dev(self._h, dZ or None, dmu or None, drho or None, dmu_eff or None, dweight or None,
                                                  dinfo or None, stream))

    def auglag_merit_dev(self, dZ, sigma, dmu, drho, dphi, dZf=0, dg=0, dinfo=0, stream=0):
        """``auglag_merit`` on device pointers (dphi one double, dinfo 8 doubles); drho = 0: ``feasible_merit_dev``."""
        self._check(self._lib.dto_auglag_merit_dev(self._h, dZ or None, float(sigma), dmu or None, drho or None, dphi or None, dZf or None,
                                                   dg or None, dinfo or None, stream))

    def auglag_gradient_dev(self, dZ, sigma, dmu, drho, dgrad, dlam=0, dmu_eff=0, stream=0):
        """``auglag_gradient`` on device pointers; drho = 0: ``reduced_gradient_dev``."""
        self._check(self._lib.dto_auglag_gradient_dev(self._h, dZ or None, float(sigma), dmu or None, drho or None, dgrad or None,
                                                      dlam or None, dmu_eff or None, stream))

    def auglag_hessian_products_dev(self, dZ, sigma, dmu, drho, n_cols, dV, dY, stream=0):
        """``auglag_hessian_products`` on device pointers, dV and dY (n_cols, n_variables); drho = 0: ``reduced_hessian_products_dev``."""
        self._check(self._lib.dto_auglag_hessian_products_dev(self._h, dZ or None, float(sigma), dmu or None, drho or None, int(n_cols),
                                                              dV or None, dY or None, stream))

    def auglag_newton_step_dev(self, dZ, sigma, dmu, drho, dfree, dlo, dhi, radius, shift, rtol, atol, max_iter, dp, dinfo, dtrace=0,
                               dstates=0, dZp=0, stream=0):
        """``auglag_newton_step`` on device pointers, arguments as ``reduced_newton_step_box_dev`` with drho behind dmu."""
        self._check(self._lib.dto_auglag_newton_step_dev(self._h, dZ or None, float(sigma), dmu or None, drho or None, dfree or None,
                                                         dlo or None, dhi or None, float(radius), float(shift), float(rtol), float(atol),
                                                         int(max_iter), dp or None, dinfo or None, dtrace or None, dstates or None,
                                                         dZp or None, stream))

    def newton_pairs_push_dev(self, ds, dy, stream=0):
        """``newton_pairs_push`` on device pointers, copied on ``stream`` (no finiteness check)."""
        self._check(self._lib.dto_newton_pairs_push_dev(self._h, ds or None, dy or None, stream))

    def newton_precondition_dev(self, dfree, n_cols, dr, dz, stream=0):
        """``newton_precondition`` on device pointers: dr and dz (n_cols, n_variables), dfree (n_variables) or 0."""
        self._check(self._lib.dto_newton_precondition_dev(self._h, dfree or None, int(n_cols), dr or None, dz or None, stream))

    def preconditioned_newton_step_dev(self, dZ, sigma, dmu, drho, dfree, dlo, dhi, radius, shift, rtol, atol, max_iter, harvest, dp, dinfo,
                                       dtrace=0, dstates=0, dZp=0, stream=0):
        """``preconditioned_newton_step`` on device pointers, arguments as ``auglag_newton_step_dev`` with harvest behind max_iter;
        dinfo 16 doubles, dtrace (max_iter, 8)."""
        self._check(self._lib.dto_preconditioned_newton_step_dev(self._h, dZ or None, float(sigma), dmu or None, drho or None, dfree or None,
                                                                 dlo or None, dhi or None, float(radius), float(shift), float(rtol),
                                                                 float(atol), int(max_iter), int(bool(harvest)), dp or None, dinfo or None,
                                                                 dtrace or None, dstates or None, dZp or None, stream))

    def reduced_minimize_dev(self, dZ, sigma, dmu, drho, dfree, dlo, dhi, outer, trials, harvest, dinfo, dhistory=0, douter_history=0, dstates=0,
                             stream=0, **options):
        """``reduced_minimize`` on device pointers: dZ, dmu and drho are updated in place on ``stream`` (dmu may be 0 only where drho
        is); dinfo 16 doubles, dhistory (outer * trials, 8), douter_history (outer, 4), dstates (n_variables) or 0.  The call waits on
        ``stream`` for its own mailbox after every trial; ``options`` as ``reduced_minimize`` (they are read on the host)."""
        opts = self._minimize_options(options)
        self._check(self._lib.dto_projected_minimize_dev(self._h, dZ or None, float(sigma), dmu or None, drho or None, dfree or None, dlo or None,
                                                       dhi or None, opts.ctypes.data, int(outer), int(trials), int(bool(harvest)), dinfo or None,
                                                       dhistory or None, douter_history or None, dstates or None, stream))

    # ---- multi-GPU: the engine's own collectives (RCCL over xGMI behind the C ABI; include/dto_engine.h, "Multi-GPU")
    @staticmethod
    def comm_unique_id():
        """128 bytes from ncclGetUniqueId: call on ONE rank and hand them to the others (e.g. torch.distributed's
        broadcast_object_list, MPI, a file)."""
        lib = load_library()
        buf = C.create_string_buffer(capi.COMM_ID_BYTES)
        if lib.dto_comm_unique_id(buf) != 0:
            raise EngineError(lib.dto_last_error(None).decode())
        return buf.raw

    def comm_create(self, unique_id, rank, world):
        """Collective over the ranks: ncclCommInitRank on this handle's device + exchange of the ranks' knot ranges."""
        buf = C.create_string_buffer(bytes(unique_id), capi.COMM_ID_BYTES)
        self._check(self._lib.dto_comm_create(self._h, buf, rank, world))

    def comm_set_ranges(self, rank, ranges):
        """The layout bookkeeping without a communicator (works on structure-only handles): ranges = [(k_lo, k_hi)] per rank."""
        lo = np.ascontiguousarray([a for a, _ in ranges], dtype=np.int64)
        hi = np.ascontiguousarray([b for _, b in ranges], dtype=np.int64)
        self._check(self._lib.dto_comm_set_ranges(self._h, rank, len(ranges), _ip(lo), _ip(hi)))

    def comm_destroy(self):
        self._check(self._lib.dto_comm_destroy(self._h))

    def gather_layout(self, vector):
        """dto_get_gather_layout: how to allocate one value vector (capi.VECTOR_*) so that the gather moves every slab in place."""
        L = capi.GatherLayout()
        self._check(self._lib.dto_get_gather_layout(self._h, vector, C.byref(L)))
        return L

    def gather_slabs(self, vector):
        """[(lo, len)] of every rank's slab of one value vector."""
        w = self.gather_layout(vector).world
        lo, ln = np.empty(w, dtype=np.int64), np.empty(w, dtype=np.int64)
        self._check(self._lib.dto_gather_slabs(self._h, vector, _ip(lo), _ip(ln)))
        return list(zip(lo.tolist(), ln.tolist()))

    def gather_dev(self, vector, dbuf, stream=0):
        """All ranks: fill in the other ranks' slabs of the vector allocated per gather_layout (dbuf = the allocation)."""
        fn = {capi.VECTOR_JACOBIAN: self._lib.dto_gather_jacobian_dev, capi.VECTOR_HESSIAN: self._lib.dto_gather_hessian_dev,
              capi.VECTOR_GRADIENT: self._lib.dto_gather_gradient_dev}[vector]
        self._check(fn(self._h, dbuf, stream))

    def gather_constraint_dev(self, dg_local, dg_full, stream=0):
        self._check(self._lib.dto_gather_constraint_dev(self._h, dg_local, dg_full, stream))

    def allreduce_objective_dev(self, df, stream=0):
        self._check(self._lib.dto_allreduce_objective_dev(self._h, df, stream))

    def bind_output_dev(self, vector, dptr):
        """dto_bind_output_dev: declare a device value vector (capi.VECTOR_JACOBIAN / VECTOR_HESSIAN) that later `*_dev` calls are
        handed again and again; its call-invariant entries are then written once.  dptr = 0 unbinds."""
        self._check(self._lib.dto_bind_output_dev(self._h, vector, dptr))

    def set_option(self, name, value):
        """dto_set_option: ``reuse_forward_sweep`` (solver loops evaluate g, J, H at the same point), ``expm_form``
        (0 = by cost, 2 / 3 = two- / three-product form of the Jacobian's matrix exponential), ``tdb_matrix_free_products`` (0 | 1,
        default 0: 1 evaluates J w / J' w of device TimeDependentBilinearIntegrators, on the dense paths and on the structured
        path of ``block_generators`` alike, without forming a Jacobian -- the scheme applied to two vectors, or to 1 + p forward
        vectors and one adjoint vector; column groups of the b x b map on the structured path), ``tdb_share_members`` (members per launch of a
        shared group of time-dependent integrators, 1 = one launch per member), ``tdb_resident`` (cap on the persistent grid of the
        k_tdb_mfma / k_tdb_kron launches and of their product forms, 0 = the default grid; for tests and measurements, the results do not depend on it),
        ``reduced_input_store`` (0 | 1, default 0: 1 makes ``reduced_lagrangian_gradient`` / ``reduced_hessian_product`` and their
        ``_dev`` forms take J v^ and J' w from the input blocks kept with ``dynamics_solve_all``'s point -- two small launches instead
        of a J w and a J' w per product; another summation order, so values agree with the default route to rounding, not in bits),
        ``reduced_block_width`` (0 = the engine's choice, or 1 .. 64: the most columns per chunk of ``eval_hessian_lagrangian_products``
        / ``reduced_hessian_products`` and their ``_dev`` forms; for tests and measurements, the results do not depend on it),
        ``newton_pairs`` (0 .. 16, default 0 = off: the capacity of the pair store of ``preconditioned_newton_step``; setting it
        clears the store); include/dto_engine.h lists every option."""
        self._check(self._lib.dto_set_option(self._h, name.encode(), int(value)))

    # ---- measurement
    def profile_enable(self, on=True):
        self._check(self._lib.dto_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._check(self._lib.dto_profile_reset(self._h))

    def interval_costs(self, Z, first=0, count=None):
        """Flop model of one eval_constraint_jacobian per interval (dto_interval_costs): input of cost-balanced sharding."""
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        K = self.trajectory.N - 1
        count = K - first if count is None else count
        out = np.empty(count)
        self._check(self._lib.dto_interval_costs(self._h, Z.ctypes.data_as(capi.c_double_p), first, count, out.ctypes.data_as(capi.c_double_p)))
        return out

    def profile_get(self, name):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        self._check(self._lib.dto_profile_get(self._h, name.encode(), C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value

    def last_stats(self):
        a, b = C.c_int32(), C.c_int32()
        self._check(self._lib.dto_last_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value
