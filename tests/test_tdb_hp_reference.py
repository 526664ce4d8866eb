"""CPU: the 320-bit reference of the time-dependent discrete map (tests/tdb_hp_reference.py) is pinned, the fixtures
tests/golden/tdbhp_*.npz come out of their generator, the fp64 yardstick (tests/tdb_large_cases.py) sits within 1e-13 of every
fixture in the normwise metric per interval and quantity class (tests/tdbhp_cases.py), every stored bar is 16 x the yardstick's
worst error floored at 64 2^-53, and five defects of the kind the bars are there for each land over one of them.

The oracle's own Hessian (Richardson-extrapolated differences of a complex-step gradient) is measured here as well: DESIGN section
4.11 records the figures."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import dto_oracle as O
import hp_cases as HC
import hp_reference as HP
import tdb_hp_reference as T
import tdb_large_cases as L
import tdbhp_cases as C

NAMES = list(C.CASES)


# ---- sin and cos ----------------------------------------------------------------------------------------------------------------

ARGS = [0.0, 1e-9, 0.5, -0.5, 1.7 * 2.6, -3.0, 6.283185307179586, 8.0, -8.0]


def test_sin_and_cos_satisfy_their_identities_to_300_bits():
    tol = 1 << (T.FRAC_BITS - 300)
    for a in ARGS:
        af = int(T.fx(a))
        s, c = T.sincos(af)
        assert abs(T.smul(s, s) + T.smul(c, c) - T.ONE) <= tol, a
        s2, c2 = T.sincos(2 * af)
        assert abs(s2 - 2 * T.smul(s, c)) <= tol and abs(c2 - (T.smul(c, c) - T.smul(s, s))) <= tol, a
    assert T.sincos(0) == (0, T.ONE)


def test_sin_and_cos_agree_with_mpmath():
    mp = pytest.importorskip("mpmath")
    with mp.workdps(110):
        for a in ARGS:
            s, c = T.sincos(int(T.fx(a)))
            x = mp.mpf(a)
            assert abs(mp.mpf(s) / mp.mpf(T.ONE) - mp.sin(x)) <= mp.mpf(2) ** -300, a
            assert abs(mp.mpf(c) / mp.mpf(T.ONE) - mp.cos(x)) <= mp.mpf(2) ** -300, a


# ---- the map against the oracle's statement of it, 4 states --------------------------------------------------------------------


def test_flow_is_the_oracles_f_and_a_finer_step_count_converges_at_fourth_order():
    """The defect of tdbhp_n4 from `flow` against O.TimeDependentBilinearIntegrator.f in fp64, interval by interval; and the map
    itself: halving h divides the distance to a 64-step solution by about 16 (a scheme of any other order, or a wrong weight,
    does not)."""
    name = "tdbhp_n4"
    d = C.inputs(name)
    p, _ = C.at_point(name, d["Z"])
    it = p.integrators[0]
    n, m, z = it.x_dim, it.u_dim, p.z
    Zk = d["Z"].reshape(p.N, z)
    fam = T.family(it.G, it.mods)
    for k in range(p.K):
        u, t, dt, u1 = (T.fx(Zk[k, n:n + m]), int(T.fx(Zk[k, it.t_off])), int(T.fx(Zk[k, p.dt_idx])), T.fx(Zk[k + 1, n:n + m]))
        x = T.fx(Zk[k, :n]).reshape(n, 1)
        y = {S: T.to_float(T.flow(fam, 1, S, u, u1, t, dt, x))[:, 0] for S in (3, 6, 12, 64)}
        f = it.f(np.concatenate([Zk[k], Zk[k + 1]]))
        assert np.abs((Zk[k + 1, :n] - y[3]) - f).max() <= 1e-14 * max(1.0, np.abs(y[3]).max())
        e = [np.abs(y[S] - y[64]).max() for S in (3, 6, 12)]
        if e[0] > 1e-9:       # (the interval at ||dt G|| = 0.05 is converged to rounding at 3 steps)
            assert 10.0 < e[0] / e[1] < 24.0 and 10.0 < e[1] / e[2] < 24.0, (k, e)


@functools.lru_cache(maxsize=None)
def oracle_errors(name):
    """The oracle's own evaluator (complex-step Jacobian, differenced Hessian) against the fixture."""
    fix = C.load(name)
    p, ev_o = C.at_point(name, fix["Z"])
    errs = C.errors(name, fix, C.callbacks_of(ev_o, fix))
    print(C.report(name, fix, errs, "O.OracleEvaluator vs fixture"))
    return errs


@pytest.mark.parametrize("name", ["tdbhp_n4", "tdbhp_n16"])
def test_reference_agrees_with_the_oracle_to_fp64_accuracy(name):
    """Values, Jacobian classes and products: the oracle computes them exactly to rounding (1e-13, the cap the yardstick is held
    to).  Its Hessian is a Richardson-extrapolated difference at h = 2e-3: a truncation of h^4 = 1.6e-11 times a ratio of
    derivatives of the map (of order one at ||dt G|| <= 3) on top of rounding / h = 6e-14, so 1e-10 is allowed here -- a hundred
    times inside the 1e-8 of the fp64-oracle tests; the figure is printed."""
    errs = oracle_errors(name)
    for (cls, k), v in errs.items():
        if cls in C.EXACT:
            assert v == 0.0, (cls, k)
        elif cls != "hess":
            assert v <= HC.ORACLE_CAP, (name, cls, k, v)
    h = {k: v for (cls, k), v in errs.items() if cls == "hess"}
    print(name, "oracle Hessian, normwise per interval window:", {k: f"{v:.1e}" for k, v in sorted(h.items())})
    assert all(v <= 1e-10 for v in h.values()), h


# ---- fixtures -------------------------------------------------------------------------------------------------------------------


def _generator():
    spec = importlib.util.spec_from_file_location("make_tdbhp_golden", os.path.join(C.GOLDEN, "make_tdbhp_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["tdbhp_n4", "tdbhp_n16"])
def test_one_interval_regenerates_bit_for_bit(name):
    """Interval 0 alone: its rows of g, J and J w, and the Hessian entries with a row in knot 0 (to which no other interval adds)."""
    fresh, stored = _generator().build(name, intervals=[0]), C.load(name)
    for key in C.INPUT_KEYS:
        if key in stored:
            assert np.array_equal(fresh[key], stored[key]), key
    assert np.allclose(fresh["norm2"], stored["norm2"], rtol=1e-12, atol=0)
    assert str(fresh["input_hash"]) == str(stored["input_hash"])
    p, ev_o = C.at_point(name, stored["Z"])
    n = C.CASES[name]["n"]
    assert np.array_equal(fresh["cons"][:n], stored["cons"][:n]) and np.array_equal(fresh["Jw"][:n], stored["Jw"][:n])
    rows = ev_o.jac_rows < n
    assert rows.sum() == n * 2 * p.z and np.array_equal(fresh["jac"][rows], stored["jac"][rows])
    rows = ev_o.hess_rows < p.z
    assert np.count_nonzero(stored["hess"][rows]) > 0 and np.array_equal(fresh["hess"][rows], stored["hess"][rows])
    assert np.array_equal(fresh["JTw"][:p.z], stored["JTw"][:p.z])


@pytest.mark.parametrize("name", NAMES)
def test_fixture_inputs_are_the_seeds_and_the_ladder(name):
    fix = C.load(name)
    c = C.CASES[name]
    d = C.inputs(name)
    assert C.input_hash(d) == str(fix["input_hash"]) == C.input_hash(fix)
    largest_hp = max(os.path.getsize(os.path.join(C.GOLDEN, f)) for f in os.listdir(C.GOLDEN) if f.startswith("hp_"))
    assert os.path.getsize(os.path.join(C.GOLDEN, name + ".npz")) < largest_hp
    assert np.allclose(np.sort(fix["norm2"]), C.RUNGS, rtol=1e-12, atol=0)
    p, ev_o = C.at_point(name, fix["Z"])
    it = p.integrators[0]
    assert (it.x_dim, it.u_dim, it.spline_order, len(it.mods), it.substeps) == (c["n"], c["m"], c["order"], c["n_mods"], c["S"])
    Zk = fix["Z"].reshape(p.N, p.z)
    t_end = Zk[:p.K, it.t_off] + Zk[:p.K, p.dt_idx]
    assert Zk[:, it.t_off].max() <= 2.0 and all(abs(w) * t_end.max() <= 8.0 for _, w, _ in it.mods)
    for G in [it.G] + [H for _, _, H in it.mods]:           # random, not skew
        assert np.abs(G + G.transpose(0, 2, 1)).max() > 0.1
    if "b" in c:
        assert c["b"] * c["r"] == c["n"] and np.array_equal(it.G[0], np.kron(np.eye(c["r"]), it.G[0][:c["b"], :c["b"]]))
    finite = lambda key: np.isfinite(fix[key])
    assert finite("cons").all() and finite("Jw").all()
    if "sample" not in c:
        assert c["n"] <= 64 and all(finite(k).all() for k in ("jac", "JTw", "hess"))
    else:
        cols = C.columns(name)
        assert len(cols) == 16 and np.array_equal(fix["cols"], cols) and {0, 31, 32, 63, 64, c["n"] - 1} <= set(cols.tolist())
        for key in ("jac", "JTw", "hess"):
            assert fix[key + "_known"].dtype == bool and np.array_equal(finite(key), fix[key + "_known"]), key
        unknown_cols = np.unique((ev_o.jac_cols[~fix["jac_known"]] % p.z) - it.x_off)
        assert np.array_equal(unknown_cols, np.setdiff1d(np.arange(c["n"]), cols))
        assert np.count_nonzero(~fix["jac_known"]) == p.K * c["n"] * (c["n"] - 16)
        assert np.count_nonzero(~fix["JTw_known"]) == p.K * (c["n"] - 16)
        pth = c["m"] + 2 + (c["m"] if c["order"] else 0)
        assert np.count_nonzero(~fix["hess_known"]) == p.K * (c["n"] - 16) * pth
    if c.get("group"):
        for key in ("cons_b", "jac_b", "Jw_b", "JTw_b", "hess_b", "JTw_g", "hess_g", "x_b", "mu_b", "wx_b", "wt_b"):
            assert key in fix, key
        # what both members add to differs from either member's own, what one member owns does not
        assert not np.array_equal(fix["hess_g"][fix["hess_known"]], fix["hess"][fix["hess_known"]])
        assert np.array_equal(fix["JTw_g"][:c["n"]][cols], fix["JTw"][:c["n"]][cols])


def test_the_metric_reads_known_entries_and_lets_no_nan_through():
    name = "tdbhp_n128"
    fix = C.load(name)
    for key in ("jac", "JTw", "hess"):
        got = np.where(fix[key + "_known"], fix[key], 123.0)       # exact where known, anything finite elsewhere
        assert all(v == 0.0 for v in C.errors(name, fix, {key: got}).values()), key
        got[np.flatnonzero(~fix[key + "_known"])[3]] = np.nan
        assert np.inf in C.errors(name, fix, {key: got}).values(), key
        got = np.where(fix[key + "_known"], fix[key], 123.0)
        i = int(np.argmax(np.where(fix[key + "_known"] & (np.abs(fix[key]) != 1.0), np.abs(fix[key]), 0.0)))
        got[i] *= 1.0 + 1e-9                                       # the largest known entry off by 1e-9 relative shows
        assert max(C.errors(name, fix, {key: got}).values()) > 1e-12, key
    # a structural zero that is written as something else fails "const" whatever its size
    got = fix["jac"].copy()
    got[np.flatnonzero(fix["jac"] == 0.0)[0]] = 1e-300
    assert max(v for (cls, k), v in C.errors(name, fix, dict(jac=got)).items() if cls == "const") == np.inf


# ---- the yardstick and the bars ---------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def yardstick(name):
    fix = C.load(name)
    errs = C.yardstick_errors(name, fix)
    print(C.report(name, fix, errs, "yardstick (tests/tdb_large_cases.py) vs fixture"))
    return fix, errs


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_stays_within_its_cap_and_the_bars_are_derived_from_it(name):
    fix, errs = yardstick(name)
    classes, yard, bars = C.bars_from(errs)
    assert list(classes) == list(fix["classes"])
    c = C.CASES[name]
    want = {"defect", "Phi", "t", "dt", "const", "Jw", "JTw", "hess", "hess_outside_blocks"} | {f"u{j}" for j in range(c["m"])}
    want |= {f"un{j}" for j in range(c["m"])} if c["order"] == 1 else set()
    assert set(classes) == want
    # measured again here and as stored: under the cap, class by class and interval by interval
    for (cls, k), v in errs.items():
        assert v <= (0.0 if cls in C.EXACT else HC.ORACLE_CAP), (name, cls, k, v)
    stored = fix["yard"]
    assert stored.shape == (len(classes), C.N_KNOTS) and np.nanmax(stored) <= HC.ORACLE_CAP
    assert np.array_equal(np.isnan(stored), np.isnan(yard))
    # the stored bars are the rule applied to the stored measurement, and no bar passes 16 x the cap
    for i, cls in enumerate(classes):
        rule = 0.0 if cls in C.EXACT else max(C.BAR_FACTOR * np.nanmax(stored[i]), HC.BAR_NO_SQUARING)
        assert fix["bars"][i] == rule == C.bar_for(fix, cls), cls
        assert fix["bars"][i] <= C.BAR_FACTOR * HC.ORACLE_CAP
        # measured again (another BLAS or thread count may sum in another order) the yardstick itself stays under the stored bar
        assert np.nanmax(yard[i]) <= fix["bars"][i], (cls, yard[i], stored[i])
    print(name, "bars:", {str(cls): f"{b:.2e}" for cls, b in zip(classes, fix["bars"])})


# ---- the bars discriminate --------------------------------------------------------------------------------------------------------


def defective(weight2=1.0, fewer_steps=0, carrier_at_tk=False, hold_u=False, drop_dt=False):
    """tests/tdb_large_cases.FastTdb with one defect built in.  The first four change the map (its step matrices, hence g, Phi and
    every first derivative, which FastTdb takes as complex steps of the step-matrix product); the last one changes the analytic
    d M / d t_k that only the (theta, theta) Hessian's sensitivity recursion reads."""

    class Defective(L.FastTdb):
        def _M(self, th, tau):
            uk, tk, dt, uk1 = self._split(th)
            u = uk + tau * (uk1 - uk) if self.spline_order == 1 and not hold_u else uk
            return dt * self.generator(u, tk if carrier_at_tk else tk + tau * dt)

        def _flow(self, th):
            n, S = self.x_dim, self.substeps - fewer_steps
            h = 1.0 / S
            I = np.eye(n)
            Phi = np.eye(n, dtype=np.result_type(th, np.float64))
            for i in range(S):
                M1, M2, M4 = self._M(th, i * h), self._M(th, (i + 0.5) * h), self._M(th, (i + 1.0) * h)
                K1 = M1
                K2 = M2 @ (I + 0.5 * h * K1)
                K3 = M2 @ (I + 0.5 * h * K2)
                K4 = M4 @ (I + h * K3)
                Phi = (I + (h / 6.0) * (K1 + K4) + (h / 3.0) * weight2 * K2 + (h / 3.0) * K3) @ Phi
            return Phi

        def f(self, zz, k=0):
            zz = np.asarray(zz, dtype=np.float64)
            n, z = self.x_dim, self.z
            return zz[z + self.x_off:z + self.x_off + n] - self._flow(zz[self._params()]) @ zz[self.x_off:self.x_off + n]

        def _dM(self, th, tau):
            out = super()._dM(th, tau)
            if drop_dt:
                out[self.u_dim] = out[self.u_dim] / self._split(th)[2]
            return out

    return Defective


DEFECTS = [("one h/3 weight times 1 + 1e-9", dict(weight2=1.0 + 1e-9), "Phi"),
           ("S - 1 steps", dict(fewer_steps=1), "defect"),
           ("carrier at t_k, not t_k + tau dt_k", dict(carrier_at_tk=True), "dt"),
           ("u held under order 1", dict(hold_u=True), "un0"),
           ("dt factor dropped from the carrier's t-derivative", dict(drop_dt=True), "hess")]


def test_a_defect_free_restatement_stays_under_every_bar():
    """The class the defects are built into, with none switched on: its f goes through the step-matrix product."""
    name = "tdbhp_n16"
    fix = C.load(name)
    errs = C.yardstick_errors(name, fix, defective())
    assert all(v <= C.bar_for(fix, cls) for (cls, k), v in errs.items()), errs


@pytest.mark.parametrize("what,knobs,cls", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_each_defect_lands_over_a_stored_bar(what, knobs, cls):
    name = "tdbhp_n16"       # order 1, cos + sin, four steps
    fix = C.load(name)
    errs = C.yardstick_errors(name, fix, defective(**knobs))
    over = sorted({c for (c, k), v in errs.items() if not v <= C.bar_for(fix, c)})
    worst = max(v for (c, k), v in errs.items() if c == cls)
    print(f"{what}: class {cls} at {worst:.2e} against its bar {C.bar_for(fix, cls):.2e}; every class over its bar: {over}")
    assert worst > C.bar_for(fix, cls), (what, cls, worst)
    assert worst > 100.0 * C.bar_for(fix, cls), (what, cls, worst)     # not by a hair: orders, as the bars' derivation says
